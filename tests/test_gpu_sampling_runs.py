"""Sampling generate() calls (beam_size=1, sampling_topk=0, num_hypotheses=best_of: what the temperature fallback of the
sequential path issues at temperature > 0) share decode runs among themselves (decoder.hip: mergeable / generate_run).  Each
call keeps its own temperature and seed: every decode row reads them, and the first row of its call, from a per-row device
table, and draws its Gumbel noise as the row of its call that it is in a run of that call alone.  So, as for every merged
run, each caller must get EXACTLY what it gets alone: ids, scores, no-speech probability and per-token log-probabilities bit
for bit — also when the prompts differ in length (ragged runs), and a sampling run's step graph is reused whatever the
seeds and temperatures of its calls.

A sampling leader does not wait for workers that are still encoding, so the calls are queued behind a BLOCKER run that holds
the only lane (the pattern of tests/test_gpu_token_logprobs.py): the next run takes every queued call that may share it."""
import ctypes as C
import dataclasses
import os
import threading
import time

import numpy as np
import pytest

from conftest import bench_audio

pytestmark = pytest.mark.gpu

GEOMETRIES = [("micro", "float16"), ("tiny.en", "float16"), ("micro", "int8_float16")]
N_PREV = (0, 1, 17, 35)      # previous-text tokens: none, inside one 16-position block, across a block boundary, three blocks
CHUNKS = (2, 1, 3, 1)        # (call 2 sits at row 9 of the run behind calls of 2 and 1 chunks x 3 hypotheses)
TEMPS = (0.2, 0.6, 1.0, 0.6)
SEEDS = (7, 7, 11, 12)       # calls 0 / 1: same seed, other temperature; calls 1 / 3: same temperature, other seed


def _model(name, workers, compute_type="float16", max_batch=3):
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config(name)
    w = synthetic_weights(cfg, seed=21)
    m = Whisper(f"synthetic:{name}", device="cuda", files={"config": cfg, "weights": w}, compute_type=compute_type,
                max_batch_size=max_batch, max_beam_size=5, inter_threads=workers)
    m.set_decode_lanes(1)                             # one run at a time: what is queued behind the blocker meets in one
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


def _sampling(cfg, i, max_length, nh=3, **more):
    return dict(beam_size=1, num_hypotheses=nh, sampling_topk=0, sampling_temperature=TEMPS[i], seed=SEEDS[i],
                max_length=max_length, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_scores=True,
                return_no_speech_prob=True, return_token_logprobs=True, **more)


def _same(got, want, what=""):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.sequences_ids == b.sequences_ids, what
        assert a.scores == b.scores, what
        assert a.no_speech_prob == b.no_speech_prob, what
        assert a.token_logprobs == b.token_logprobs, what
        assert a.end_logprobs == b.end_logprobs, what


def _solo(model, batches, prompts, kws):
    return [model.generate(model.encode_pcm(b), [p] * len(b), **kw) for b, p, kw in zip(batches, prompts, kws)]


def _behind_blocker(model, cfg, batches, prompts, kws, order=None):
    """one host thread (one worker replica) per call: encode, then wait until a run that none of them can share (beam 2, <eot>
    suppressed: it decodes its whole text context) holds the only lane, then generate.  order: the calls enter generate()
    in this order, each only after its predecessor has gone into its call.  -> results, decode runs it took"""
    n = len(batches)
    out, errs = [None] * n, []
    encoded, go = threading.Barrier(n + 1), threading.Event()
    gone = [threading.Event() for _ in range(n)]
    before = {} if order is None else {i: (order[k - 1] if k else None) for k, i in enumerate(order)}

    def work(i):
        try:
            enc = model.encode_pcm(batches[i])
            encoded.wait(timeout=120)
            assert go.wait(timeout=120)
            if before.get(i) is not None:
                assert gone[before[i]].wait(timeout=120)
            gone[i].set()
            out[i] = model.generate(enc, [prompts[i]] * len(batches[i]), **kws[i])
        except Exception as e:   # noqa: BLE001
            errs.append(e)
            gone[i].set()

    plain = _prompt(cfg, 0)
    blocker_enc = model.encode_pcm(batches[0][:1] * 3)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in ts:
        t.start()
    encoded.wait(timeout=120)
    st0 = model.decode_stats()
    tb = threading.Thread(target=lambda: model.generate(blocker_enc, [plain] * 3, beam_size=2, max_length=cfg.n_text_ctx,
                                                        suppress_tokens=[cfg.eot]))
    tb.start()
    t_end = time.time() + 30
    while model.decode_stats()["runs"] == st0["runs"] and time.time() < t_end:
        pass                                   # until the blocker's run has started
    go.set()
    for t in ts + [tb]:
        t.join()
    assert not errs, errs
    st = model.decode_stats()
    assert st["requests"] - st0["requests"] == n + 1
    return out, st["runs"] - st0["runs"] - 1


@pytest.mark.parametrize("name,compute_type", GEOMETRIES)
def test_sampling_calls_share_a_run_and_equal_solo(name, compute_type):
    """four sampling calls of 2, 1, 3 and 1 chunks x 3 hypotheses with their own temperatures and seeds.  Before sampling
    calls could meet in a run every one of them ran alone: the run-size assertion failed."""
    cfg, model = _model(name, 5, compute_type)
    prompt = _prompt(cfg, 0)
    kws = [_sampling(cfg, i, len(prompt) + 10) for i in range(4)]
    batches = _batches(CHUNKS)
    batches[3] = batches[1]                            # calls 1 and 3: the same audio, the same temperature, another seed
    solo = _solo(model, batches, [prompt] * 4, kws)
    # the solo results are not degenerate: the seed matters, and nothing else does
    assert solo[1][0].sequences_ids != solo[3][0].sequences_ids
    _same(_solo(model, batches[1:2], [prompt], kws[1:2])[0], solo[1], "the same call again")
    assert all(len(r.sequences_ids) == 3 and r.no_speech_prob > 0 for s in solo for r in s)
    out, runs = _behind_blocker(model, cfg, batches, [prompt] * 4, kws)
    st = model.decode_stats()
    print(f"[{name} {compute_type}] 4 sampling calls -> {runs} decode runs, largest {st['max_run_chunks']} chunks")
    assert st["max_run_chunks"] > 3                   # at least two calls shared a run (the largest call has 3 chunks)
    for i in range(4):
        _same(out[i], solo[i], f"call {i}")


@pytest.mark.parametrize("name,compute_type", GEOMETRIES)
def test_ragged_sampling_runs_equal_solo(name, compute_type):
    """the prompts carry 0, 1, 17 and 35 tokens of previous text (condition_on_previous_text): a RAGGED sampling run, whose
    num_hypotheses x chunks decode chunks each sit at their own position — without and with the timestamp rules"""
    cfg, model = _model(name, 5, compute_type)
    batches = _batches(CHUNKS)
    for timestamps in (False, True):
        prompts = [_prompt(cfg, n, timestamps) for n in N_PREV]
        assert len({len(p) for p in prompts}) == 4
        more = dict(max_initial_timestamp_index=30) if timestamps else {}
        kws = [_sampling(cfg, i, len(prompts[-1]) + 10, **more) for i in range(4)]
        kws[1]["seed"] = 8                            # distinct seeds and temperatures
        kws[3]["sampling_temperature"] = 0.8
        solo = _solo(model, batches, prompts, kws)
        if timestamps:
            assert all(ids[0] >= cfg.timestamp_begin for s in solo for r in s for ids in r.sequences_ids)
        out, runs = _behind_blocker(model, cfg, batches, prompts, kws)
        print(f"[{name} {compute_type}] timestamps={timestamps}: 4 ragged sampling calls -> {runs} decode runs")
        assert runs < 4                               # calls shared a run
        for i in range(4):
            _same(out[i], solo[i], f"timestamps={timestamps} call {i}")
    assert model.decode_stats()["max_run_chunks"] > 3


def test_sampled_early_finisher_between_neighbours():
    """max_length = P_max + 6: the rows of the longest prompt are cut at their budget after 6 tokens while the rows of the
    short prompts sample at least 20 more steps beside them — in the middle of the run, where a position that walked on past
    the row's cache slot would land in a neighbour's.  Arrival order decides the order in the run."""
    cfg, model = _model("micro", 5)
    prompts = [_prompt(cfg, n) for n in N_PREV]
    kws = [_sampling(cfg, i, len(prompts[3]) + 6, min_new_tokens=20) for i in range(4)]
    batches = _batches(CHUNKS)
    solo = _solo(model, batches, prompts, kws)
    assert all(len(ids) == 6 for r in solo[3] for ids in r.sequences_ids)        # cut at the budget
    assert all(len(ids) >= 20 for s in solo[:3] for r in s for ids in r.sequences_ids)
    for order in ([0, 3, 1, 2], [1, 2, 3, 0]):
        out, _ = _behind_blocker(model, cfg, batches, prompts, kws, order=order)
        for i in range(4):
            _same(out[i], solo[i], f"order {order} call {i}")
    assert model.decode_stats()["max_run_chunks"] > 3


def test_sampling_graph_is_reused(monkeypatch):
    """temperature and seed are not part of a step graph's key: solo sampling calls of one size replay ONE graph (each of them
    used to capture and instantiate its own).  And no run is answered with another mode's graph: beam, greedy and sampling
    calls of the same size give what a model that launches every step eagerly gives."""
    if os.environ.get("FWAMD_NO_GRAPH") == "1":
        pytest.skip("step graphs are disabled (FWAMD_NO_GRAPH=1)")
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    files = {"config": cfg, "weights": synthetic_weights(cfg, seed=21)}
    prompt = _prompt(cfg, 0)
    batch = _batches((3,))[0]
    base = dict(max_length=len(prompt) + 12, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_scores=True,
                return_no_speech_prob=True, return_token_logprobs=True)
    calls = {f"sampling {i}": dict(base, beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=t, seed=s)
             for i, (t, s) in enumerate(((0.7, 5), (0.3, 6), (1.0, 7), (0.5, (9 << 32) | 8)))}
    calls["beam"] = dict(base, beam_size=3, num_hypotheses=3)
    calls["greedy"] = dict(base, beam_size=1, sampling_topk=1)
    # the reference: the same model with every step launched eagerly (the switch is read when the workspace is built, at
    # the first generate call)
    monkeypatch.setenv("FWAMD_NO_GRAPH", "1")
    eager = Whisper("synthetic:micro", device="cuda", files=files, max_batch_size=3, max_beam_size=5)
    want = {k: eager.generate(eager.encode_pcm(batch), [prompt] * 3, **kw) for k, kw in calls.items()}
    assert eager.graph_captures() == 0
    monkeypatch.delenv("FWAMD_NO_GRAPH")
    model = Whisper("synthetic:micro", device="cuda", files=files, max_batch_size=3, max_beam_size=5)
    enc = model.encode_pcm(batch)
    _same(model.generate(enc, [prompt] * 3, **calls["sampling 0"]), want["sampling 0"], "warm-up")
    c0 = model.graph_captures()
    assert c0 == 1
    for k in ("sampling 1", "sampling 2", "sampling 3"):
        _same(model.generate(enc, [prompt] * 3, **calls[k]), want[k], k)
    assert model.graph_captures() == c0               # (three more before: one per seed and temperature)
    for k in ("beam", "greedy", "sampling 2", "beam", "greedy", "sampling 0"):
        _same(model.generate(enc, [prompt] * 3, **calls[k]), want[k], k)
    assert model.graph_captures() == c0 + 2           # one for the beam calls, one for the greedy calls


def test_which_sampling_calls_do_not_merge():
    """num_hypotheses and max_length must agree, and a greedy call (beam_size=1, sampling_topk=1) is no sampling call: each of
    these pairs runs as two runs, each call returning its solo result"""
    cfg, model = _model("micro", 3)
    prompt = _prompt(cfg, 0)
    ml = len(prompt) + 10
    greedy = dict(beam_size=1, sampling_topk=1, max_length=ml, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2],
                  return_scores=True, return_no_speech_prob=True, return_token_logprobs=True)
    pairs = {"num_hypotheses": [_sampling(cfg, 0, ml, nh=2), _sampling(cfg, 1, ml, nh=3)],
             "greedy": [_sampling(cfg, 0, ml), greedy],
             "max_length": [_sampling(cfg, 0, ml), _sampling(cfg, 1, ml + 2)]}
    batches = _batches((3, 2))
    for what, kws in pairs.items():
        solo = _solo(model, batches, [prompt] * 2, kws)
        out, runs = _behind_blocker(model, cfg, batches, [prompt] * 2, kws)
        assert runs == 2, what
        for i in range(2):
            _same(out[i], solo[i], f"{what}, call {i}")
    assert model.decode_stats()["max_run_chunks"] == 3          # every call ran alone


# ------------------------------------------------------------------------------------------------ the kernel alone
TAB_R = 5
TAB_GROUPS = [(7, 0.2, 0), (7, 0.2, 0), ((7 << 32) | 99, 0.6, 2), ((7 << 32) | 99, 0.6, 2), (11, 1.0, 4)]   # (seed, T, row0)
TAB_DEAD_ROW = 3             # every logit -inf: nothing to draw
TAB_LOGITS_SEED = 40
TIE = 1e-4                   # the margin tests/test_gpu_logits_rules.py::test_gumbel_sampling_draw asks of its data


def _vocab_cfg(vocab):
    """the vocabulary of `vocab` on a micro-sized network (the rules kernel only reads the token ids)"""
    from faster_whisper_amd import get_config
    micro = get_config("micro")
    if vocab == "micro":
        return micro
    keep = ("name", "n_mels", "d_model", "n_heads", "n_enc_layers", "n_dec_layers")
    return dataclasses.replace(get_config(vocab), **{k: getattr(micro, k) for k in keep})


def _table_case(cfg, step):
    """logits [5][V] (distinct multiples of 1/8192 per row, one row all -inf), histories of `step` tokens, cum, suppress list"""
    rng = np.random.default_rng(TAB_LOGITS_SEED + step)
    V = cfg.n_vocab
    base = rng.permutation(65536)[:V].astype(np.float32) / np.float32(8192.0)
    logits = np.ascontiguousarray(np.stack([rng.permutation(base) for _ in range(TAB_R)]), dtype=np.float32)
    logits[TAB_DEAD_ROW] = -np.inf
    hist = [[11 + r, 12, 13 + r][:step] for r in range(TAB_R)]
    cum = -rng.random(TAB_R).astype(np.float32)
    sup = sorted({cfg.sot, cfg.sot_prev, cfg.no_speech, 1, 2, 7, 63, 64, cfg.n_vocab - 1})
    return logits, hist, cum, sup


def _table_reference(cfg, oracle, step):
    """per live row: (drawn token, its log-prob, gap between the two best keys)"""
    from oracle.whisper import _gumbel
    logits, hist, cum, sup = _table_case(cfg, step)
    mask = np.zeros(cfg.n_vocab, dtype=bool)
    mask[sup] = True
    out = {}
    for r, (seed, T, row0) in enumerate(TAB_GROUPS):
        if r == TAB_DEAD_ROW:
            continue
        lp = oracle._process_logits(logits[r], hist[r], False, mask, True, 50, 1.0, 0, 0)
        inv = np.float32(1.0) / np.float32(T)
        key = np.where(np.isfinite(lp), lp * inv + _gumbel(seed, r - row0, step, cfg.n_vocab), -np.inf)
        top2 = np.sort(key)[-2:]
        out[r] = (int(np.argmax(key)), float(lp[int(np.argmax(key))]), float(top2[1] - top2[0]))
    return out


@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("vocab", ["micro", "tiny.en"])
def test_sampling_table_kernel(vocab, step):
    """one launch of the sampling instantiation over five rows of three calls: row r draws arg-max of logp * inv_temp[r] +
    gumbel(seed[r], r - row0[r], step, token) — oracle/whisper.py::_gumbel, the row counted from the first row of its call"""
    from faster_whisper_amd import Whisper, _lib, synthetic_weights
    from oracle.whisper import OracleWhisper
    cfg = _vocab_cfg(vocab)
    w = synthetic_weights(cfg, seed=5)
    model = Whisper("synthetic:rules", device="cuda", files={"config": cfg, "weights": w}, max_batch_size=2, max_beam_size=5)
    logits, hist, cum, sup = _table_case(cfg, step)
    ref = _table_reference(cfg, OracleWhisper(cfg, w), step)
    o = _lib.FwGenOpts()
    o.beam_size, o.patience, o.num_hypotheses, o.length_penalty, o.repetition_penalty = 1, 1.0, 1, 1.0, 1.0
    o.max_length, o.max_initial_timestamp_index, o.suppress_blank = 448, 50, 1
    sup_a = np.asarray(sup, dtype=np.int32)
    o.suppress_tokens, o.n_suppress_tokens = _lib.as_i32p(sup_a), int(sup_a.size)
    o.sampling_topk, o.sampling_temperature, o.seed = 0, 123.0, 999        # (neither is read: the table holds the rows' own)
    h = np.ascontiguousarray(np.asarray(hist, dtype=np.int32).reshape(TAB_R, step)) if step else np.zeros((TAB_R, 1), np.int32)
    inv = np.asarray([np.float32(1.0) / np.float32(T) for _, T, _ in TAB_GROUPS], dtype=np.float32)
    seeds = np.asarray([s for s, _, _ in TAB_GROUPS], dtype=np.uint64)
    row0 = np.asarray([r0 for _, _, r0 in TAB_GROUPS], dtype=np.int32)
    cv, ct, cl = np.zeros((TAB_R, 1), np.float32), np.zeros((TAB_R, 1), np.int32), np.zeros((TAB_R, 1), np.float32)
    _lib.check(model._lib.fw_test_logits_rules_smp_tab(
        model._replicas[0].handle, _lib.ptr(logits), TAB_R, _lib.ptr(h), step, _lib.ptr(cum), C.byref(o), 0, _lib.ptr(inv),
        _lib.ptr(seeds), _lib.ptr(row0), _lib.ptr(cv), _lib.ptr(ct), _lib.ptr(cl)))
    assert np.isneginf(cv[TAB_DEAD_ROW, 0]) and np.isneginf(cl[TAB_DEAD_ROW, 0]) and ct[TAB_DEAD_ROW, 0] == 0
    skipped = 0
    for r, (tok, lp, gap) in ref.items():
        print(f"[{vocab} step {step}] row {r}: token {ct[r, 0]} (reference {tok}), log-prob {cl[r, 0]:.6f} (reference {lp:.6f}), "
              f"key gap {gap:.3e}")
        if gap <= TIE:
            skipped += 1
            continue
        assert ct[r, 0] == tok
        assert abs(cl[r, 0] - lp) < 2e-5 and abs(cv[r, 0] - (cum[r] + lp)) < 2e-5
        assert cv[r, 0] == np.float32(cum[r] + cl[r, 0])          # the recorded value is cum + the recorded log-prob
    assert skipped <= 1


def test_sampling_table_reference_has_no_near_tie():
    """(no GPU needed, but it belongs to the test above) the logits seed was chosen so that the reference alone skips no row"""
    from faster_whisper_amd import synthetic_weights
    from oracle.whisper import OracleWhisper
    for vocab in ("micro", "tiny.en"):
        cfg = _vocab_cfg(vocab)
        oracle = OracleWhisper(cfg, synthetic_weights(cfg, seed=5))
        for step in (0, 3):
            assert all(gap > TIE for _, _, gap in _table_reference(cfg, oracle, step).values())


# ------------------------------------------------------------------------------------------------ end to end
def test_transcribe_many_fallback_is_reproducible():
    """a temperature ladder without a zero rung and a log-prob threshold no decode passes: every generate() call samples and
    every window climbs both rungs.  With sampling_seed, transcribe_many returns what three separate transcribe() calls
    return, twice, although the sampled attempts of different recordings now share decode runs"""
    from faster_whisper_amd import WhisperModel, get_config, synthetic_weights
    from faster_whisper_amd.backend import recording_seed
    from oracle import micro_tokenizer
    cfg = get_config("micro")
    tok = micro_tokenizer.build()
    model = WhisperModel("synthetic:micro", device="cuda", compute_type="float16", num_workers=3,
                         files={"config": cfg, "weights": synthetic_weights(cfg, seed=33),
                                "tokenizer.json": tok.to_str().encode()},
                         max_batch_size=1, max_beam_size=5)
    audios = [bench_audio(16000 * s, seed=70 + s) for s in (36, 44, 52)]
    kw = dict(language="en", condition_on_previous_text=True, temperature=[0.4, 0.8], log_prob_threshold=0.0, best_of=3)
    want = []
    for i, audio in enumerate(audios):
        segs, info = model.transcribe(audio, sampling_seed=recording_seed(5, i), **kw)
        want.append((list(segs), info))
    st0 = model.model.decode_stats()
    print(f"three transcribe() calls: {st0['requests']} sampling calls")
    assert st0["requests"] >= 6 and st0["max_run_chunks"] == 1                   # two windows or more each, each alone
    assert all(len(s) >= 1 for s, _ in want)
    for round_ in range(2):
        got = model.transcribe_many(audios, sampling_seed=5, **kw)
        assert len(got) == 3
        for (gs, gi), (ws, wi) in zip(got, want):
            assert gs == ws, round_
            assert (gi.language, gi.duration, gi.duration_after_vad) == (wi.language, wi.duration, wi.duration_after_vad)
    st = model.model.decode_stats()
    print(f"transcribe_many x 2: {st['requests'] - st0['requests']} sampling calls in {st['runs'] - st0['runs']} decode runs, "
          f"largest {st['max_run_chunks']} chunks")
    assert st["max_run_chunks"] > 1
