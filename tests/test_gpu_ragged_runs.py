"""Ragged decode runs (decoder.hip: mergeable / generate_run): concurrent generate() calls whose prompts differ in LENGTH —
the sequential path with condition_on_previous_text prepends up to 223 tokens of previous text — share one decode run, every
chunk at its own position in the text context and with its own budget.  As for every merged run, each caller must get
EXACTLY what it gets alone: ids, scores, no-speech probability and per-token log-probabilities bit for bit.  One call with
prompts of different lengths stays a ValueError."""
import threading

import numpy as np
import pytest

from conftest import bench_audio

pytestmark = pytest.mark.gpu

GEOMETRIES = [("micro", "float16"), ("tiny.en", "float16"), ("micro", "int8_float16")]
N_PREV = (0, 1, 17, 35)      # previous-text tokens: none (the plain prompt), inside one 16-position block, across a block
                             # boundary, over three blocks
CHUNKS = (3, 3, 2, 3)


def _model(name, workers, compute_type="float16", max_batch=3):
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config(name)
    w = synthetic_weights(cfg, seed=21)
    m = Whisper(f"synthetic:{name}", device="cuda", files={"config": cfg, "weights": w}, compute_type=compute_type,
                max_batch_size=max_batch, max_beam_size=5, inter_threads=workers)
    return cfg, m


def _batches(sizes):
    return [[bench_audio(480000 if (i + j) % 3 else 250000, seed=50 + 10 * i + j) for j in range(n)]
            for i, n in enumerate(sizes)]


def _prompt(cfg, n_prev, timestamps=False):
    """[sot_prev] + n previous tokens + sot_sequence (+ [no_timestamps]); n_prev = 0: the plain prompt"""
    tail = list(cfg.sot_sequence) + ([] if timestamps else [cfg.no_timestamps])
    if n_prev == 0:
        return tail
    return [cfg.sot_prev] + [10 + (7 * i) % 200 for i in range(n_prev)] + tail


def _same(got, want, what=""):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.sequences_ids == b.sequences_ids, what
        assert a.scores == b.scores, what
        assert a.no_speech_prob == b.no_speech_prob, what
        assert a.token_logprobs == b.token_logprobs, what
        assert a.end_logprobs == b.end_logprobs, what


def _concurrent(model, batches, prompts, kws, order=None):
    """one host thread (one worker replica) per call: encode, meet at a barrier, generate together, while one more thread keeps
    an encode in flight so that the leader of the run waits for the others.  order: the calls enter generate() in this
    order, each only after its predecessor has gone into its call"""
    n = len(batches)
    out, errs = [None] * n, []
    bar = threading.Barrier(n)
    gone = [threading.Event() for _ in range(n)]
    before = {} if order is None else {i: (order[k - 1] if k else None) for k, i in enumerate(order)}

    def work(i):
        try:
            enc = model.encode_pcm(batches[i])
            bar.wait()
            if before.get(i) is not None:
                gone[before[i]].wait()
            gone[i].set()
            out[i] = model.generate(enc, [prompts[i]] * len(batches[i]), **kws[i])
        except Exception as e:   # noqa: BLE001
            errs.append(e)
            gone[i].set()
            bar.abort()

    stop = threading.Event()

    def keep_encoding():
        while not stop.is_set():
            model.encode_pcm(batches[0][:1])

    ts = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    bg = threading.Thread(target=keep_encoding)
    for t in ts:
        t.start()
    bg.start()
    for t in ts:
        t.join()
    stop.set()
    bg.join()
    assert not errs, errs
    return out


def _solo(model, batches, prompts, kws):
    return [model.generate(model.encode_pcm(b), [p] * len(b), **kw) for b, p, kw in zip(batches, prompts, kws)]


@pytest.mark.parametrize("name,compute_type", GEOMETRIES)
def test_ragged_merged_runs_equal_solo_runs(name, compute_type):
    """four calls of 3, 3, 2 and 3 chunks whose prompts carry 0, 1, 17 and 35 tokens of previous text share runs.  Before
    calls of different prompt lengths could meet in a run every one of them ran alone: the run-size assertion failed."""
    cfg, model = _model(name, 4, compute_type)
    prompts = [_prompt(cfg, n) for n in N_PREV]
    assert len({len(p) for p in prompts}) == 4
    kw = dict(beam_size=5, patience=1.0, length_penalty=1.0, max_length=len(prompts[-1]) + 10,
              suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_scores=True, return_no_speech_prob=True,
              return_token_logprobs=True)
    batches = _batches(CHUNKS)
    solo = _solo(model, batches, prompts, [kw] * 4)
    assert all(r.no_speech_prob > 0 and len(r.sequences_ids[0]) > 0 for s in solo for r in s)
    runs0 = model.decode_stats()["runs"]
    out = _concurrent(model, batches, prompts, [kw] * 4)
    st = model.decode_stats()
    print(f"[{name} {compute_type}] 4 ragged calls -> {st['runs'] - runs0} decode runs, largest {st['max_run_chunks']} chunks")
    assert st["max_run_chunks"] > 3                   # at least two calls shared a run
    for i in range(4):
        _same(out[i], solo[i], f"call {i}")


@pytest.mark.parametrize("name,compute_type", GEOMETRIES)
def test_early_finisher_between_neighbours(name, compute_type):
    """max_length = P_max + 6: the chunks of the longest prompt are cut at their budget after 6 tokens while the chunks of the
    short prompts decode at least 20 more steps beside them — in the middle of the run, where a position that walked on
    past the chunk's cache slot would land in a neighbour's.  Arrival order decides the order in the run: the calls enter
    generate() one after the other, once with the long-prompt call second and once with it third."""
    cfg, model = _model(name, 4, compute_type)
    model.set_decode_lanes(1)                         # one run at a time: the four calls meet in one
    prompts = [_prompt(cfg, n) for n in N_PREV]
    kw = dict(beam_size=5, max_length=len(prompts[3]) + 6, min_new_tokens=20,
              suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_scores=True, return_no_speech_prob=True,
              return_token_logprobs=True)
    batches = _batches(CHUNKS)
    solo = _solo(model, batches, prompts, [kw] * 4)
    assert all(len(ids) == 6 for r in solo[3] for ids in r.sequences_ids)        # cut at the budget
    assert all(len(ids) >= 20 for s in solo[:3] for r in s for ids in r.sequences_ids)
    for order in ([0, 3, 1, 2], [1, 2, 3, 0]):
        out = _concurrent(model, batches, prompts, [kw] * 4, order=order)
        for i in range(4):
            _same(out[i], solo[i], f"order {order} call {i}")
    assert model.decode_stats()["max_run_chunks"] > 3


@pytest.mark.parametrize("name,compute_type", GEOMETRIES)
def test_ragged_runs_with_timestamps(name, compute_type):
    cfg, model = _model(name, 4, compute_type)
    prompts = [_prompt(cfg, n, timestamps=True) for n in N_PREV]
    kw = dict(beam_size=5, max_length=len(prompts[-1]) + 10, max_initial_timestamp_index=30,
              suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_scores=True, return_no_speech_prob=True,
              return_token_logprobs=True)
    batches = _batches(CHUNKS)
    solo = _solo(model, batches, prompts, [kw] * 4)
    out = _concurrent(model, batches, prompts, [kw] * 4)
    assert model.decode_stats()["max_run_chunks"] > 3
    for i in range(4):
        _same(out[i], solo[i], f"call {i}")


def test_what_still_does_not_merge():
    """max_length and the timestamp mode must agree, a sampling call runs alone: none of these four calls may share a run
    with another one, and each returns its solo result.  Ragged prompts inside ONE call stay a ValueError."""
    cfg, model = _model("micro", 4)
    ml = len(_prompt(cfg, 35)) + 8
    base = dict(beam_size=5, max_length=ml, return_scores=True, return_no_speech_prob=True, return_token_logprobs=True)
    prompts = [_prompt(cfg, 1), _prompt(cfg, 17), _prompt(cfg, 35, timestamps=True), _prompt(cfg, 0)]
    kws = [base, dict(base, max_length=ml + 2), base,
           dict(base, beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=0.7, seed=5)]
    batches = _batches((3, 3, 3, 2))
    solo = _solo(model, batches, prompts, kws)
    out = _concurrent(model, batches, prompts, kws)
    for i in range(4):
        _same(out[i], solo[i], f"call {i}")
    assert model.decode_stats()["max_run_chunks"] == 3          # every call ran alone
    enc = model.encode_pcm(batches[0])
    with pytest.raises(ValueError, match="same length"):
        model.generate(enc, [prompts[0], prompts[1], prompts[0]], **base)


def test_uniform_run_after_ragged_run():
    """a cached step graph captured its kernel arguments by value: a uniform run (one prompt length) that follows a ragged run
    of the same size on the same model must not be answered with the ragged run's graph, nor the other way round"""
    cfg, model = _model("micro", 2)
    model.set_decode_lanes(1)
    plain = _prompt(cfg, 0)
    ragged = [_prompt(cfg, 17), _prompt(cfg, 35)]
    kw = dict(beam_size=5, max_length=len(ragged[1]) + 12, return_scores=True, return_no_speech_prob=True,
              return_token_logprobs=True)
    batches = _batches((3, 3))
    solo_u = _solo(model, batches, [plain] * 2, [kw] * 2)
    solo_r = _solo(model, batches, ragged, [kw] * 2)
    for round_ in range(2):
        out_u = _concurrent(model, batches, [plain] * 2, [kw] * 2)
        out_r = _concurrent(model, batches, ragged, [kw] * 2)
        for i in range(2):
            _same(out_u[i], solo_u[i], f"uniform, round {round_}, call {i}")
            _same(out_r[i], solo_r[i], f"ragged, round {round_}, call {i}")
    after = _solo(model, batches, [plain] * 2, [kw] * 2)
    for i in range(2):
        _same(after[i], solo_u[i], f"uniform solo after, call {i}")
    assert model.decode_stats()["max_run_chunks"] > 3


def test_transcribe_many_sequential_end_to_end():
    """WhisperModel.transcribe_many: three recordings through the sequential path on three worker threads, previous text in
    every later window's prompt and an initial prompt on one recording — the result is that of three separate transcribe()
    calls, and windows of different recordings shared decode runs"""
    from faster_whisper_amd import WhisperModel, get_config, synthetic_weights
    from oracle import micro_tokenizer
    cfg = get_config("micro")
    tok = micro_tokenizer.build()
    model = WhisperModel("synthetic:micro", device="cuda", compute_type="float16", num_workers=3,
                         files={"config": cfg, "weights": synthetic_weights(cfg, seed=33),
                                "tokenizer.json": tok.to_str().encode()},
                         max_batch_size=1, max_beam_size=5)
    audios = [bench_audio(16000 * s, seed=70 + s) for s in (36, 44, 52)]
    kw = dict(language="en", condition_on_previous_text=True, temperature=0.0)
    prompts = [None, None, "hello there how are you"]
    want = []
    for audio, ip in zip(audios, prompts):
        segs, info = model.transcribe(audio, initial_prompt=ip, **kw)
        want.append((list(segs), info))
    st0 = model.model.decode_stats()
    assert st0["requests"] >= 6 and st0["max_run_chunks"] == 1                   # two windows or more each, each alone
    got = model.transcribe_many(audios, initial_prompt=prompts, **kw)
    st = model.model.decode_stats()
    print(f"transcribe_many: {st['requests'] - st0['requests']} generate calls in {st['runs'] - st0['runs']} decode runs, "
          f"largest {st['max_run_chunks']} chunks")
    assert len(got) == 3
    for (gs, gi), (ws, wi) in zip(got, want):
        assert gs == ws
        assert (gi.language, gi.duration, gi.duration_after_vad) == (wi.language, wi.duration, wi.duration_after_vad)
    assert st["max_run_chunks"] > 1
