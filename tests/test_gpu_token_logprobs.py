"""generate(..., return_token_logprobs=True) end to end on the GPU (fixture recipe of tests/test_gpu_model.py::setup: three
chunks, one of them short; `micro` and `tiny.en`):

  1. the exact identity: adding a hypothesis' token log-probs in order in float32, then its end value, gives the cumulative
     log-prob its score normalises — bit for bit at length_penalty 0 (the score IS the sum then);
  2. early finishes: hypotheses closed by <eot> before the budget (an end value, possibly no token at all) next to
     hypotheses cut at the budget (end value exactly 0.0);
  3. nothing else moves: ids, scores and no-speech probabilities are those of the call without the keyword, and a call that
     asks for log-probs shares a decode run with one that does not, each getting its solo result;
  4. every token's value against the CPU oracle teacher-forced along the engine's own ids.

Measured on an MI355X (test 4: the largest max_i |engine_i - oracle_fp16_i| over the three chunks, with that case's band
= max_i |oracle_fp16_i - oracle_fp32_i| on the same ids and its bound max(1e-3, 3 * band); no step was tied):
  micro   greedy 1.258e-03 (band 1.194e-03, bound 3.582e-03)   beam 5  2.472e-03 (band 1.102e-03, bound 3.307e-03)
  tiny.en greedy 7.779e-03 (band 6.869e-03, bound 2.061e-02)   beam 5  4.424e-03 (band 3.807e-03, bound 1.142e-02)
The closest case to its bound is micro, beam 5, chunk 1: 0.75 of it."""
import threading
import time

import numpy as np
import pytest

from conftest import bench_audio, forced_result, make_model

pytestmark = pytest.mark.gpu

BUDGET = 16


@pytest.fixture(scope="module", params=["micro", "tiny.en"])
def setup(request):
    from faster_whisper_amd.backend import StorageView
    from oracle.whisper import OracleWhisper
    cfg, w, model = make_model(request.param, seed=11, max_batch=4, max_beam=5)
    chunks = [bench_audio(480000, seed=1), bench_audio(200000, seed=2), bench_audio(480000, seed=3)[::-1].copy()]
    enc = model.encode(StorageView.from_array(model.log_mel(chunks)))
    return cfg, w, model, enc


def _prompt(cfg, timestamps=False):
    p = list(cfg.sot_sequence)
    if not timestamps:
        p.append(cfg.no_timestamps)
    return p


def _suppress(cfg):
    return sorted({cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, cfg.translate, cfg.transcribe, 1, 2, 7})


def _sum32(lps, end):
    c = np.float32(0)
    for x in lps:
        c = np.float32(c + np.float32(x))
    return np.float32(c + np.float32(end))


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _check_identity(res, length_penalty):
    n = 0
    for r in res:
        assert len(r.token_logprobs) == len(r.sequences_ids) == len(r.end_logprobs) == len(r.scores)
        for ids, lps, end, score in zip(r.sequences_ids, r.token_logprobs, r.end_logprobs, r.scores):
            assert len(lps) == len(ids)
            assert all(np.isfinite(x) and x <= 0 for x in lps) and np.isfinite(end) and end <= 0
            s = _sum32(lps, end)
            if length_penalty == 0:
                assert _bits(s) == _bits(score), (ids, lps, end, float(s), score)
            else:
                cum = float(np.float32(score)) * float(max(len(ids), 1)) ** length_penalty
                assert abs(cum - float(s)) <= 2 * float(np.spacing(np.abs(s))), (ids, cum, float(s))
            n += 1
    return n


MODES = {
    "greedy": dict(beam_size=1),
    "beam5": dict(beam_size=5, num_hypotheses=5, patience=1.0),
    "beam2": dict(beam_size=2, patience=1.0),
    "sampling": dict(beam_size=1, num_hypotheses=5, sampling_topk=0, sampling_temperature=0.8, seed=1234),
}


@pytest.mark.parametrize("timestamps", [False, True])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_token_logprobs_add_up_to_the_score(setup, mode, timestamps):
    cfg, _, model, enc = setup
    prompt = _prompt(cfg, timestamps)
    for lp in (0.0, 1.0):
        kw = dict(MODES[mode], max_length=len(prompt) + BUDGET, suppress_tokens=_suppress(cfg), length_penalty=lp,
                  return_scores=True)
        res = model.generate(enc, [prompt] * 3, return_token_logprobs=True, **kw)
        n = _check_identity(res, lp)
        assert n == 3 * kw.get("num_hypotheses", 1)
        if timestamps:      # the timestamp rules are part of the distribution: the first token is a timestamp
            assert all(ids[0] >= cfg.timestamp_begin for r in res for ids in r.sequences_ids)


def test_early_finishes(setup):
    """every id but {eot, 20, 21, 22} suppressed: hypotheses end with <eot> before the budget of 6, others are cut at it"""
    cfg, _, model, enc = setup
    prompt = _prompt(cfg)
    keep = {cfg.eot, 20, 21, 22}
    kw = dict(beam_size=4, num_hypotheses=4, max_length=len(prompt) + 6, length_penalty=0.0, suppress_blank=False,
              suppress_tokens=[t for t in range(cfg.n_vocab) if t not in keep], return_scores=True)
    res = model.generate(enc, [prompt] * 3, return_token_logprobs=True, **kw)
    assert _check_identity(res, 0.0) == 12
    hyps = [(len(ids), end) for r in res for ids, end in zip(r.sequences_ids, r.end_logprobs)]
    print(f"[{cfg.name}] early finishes (length, end log-prob): {hyps}")
    assert any(n < 6 and end != 0.0 for n, end in hyps)          # closed by <eot> before the budget
    assert any(n == 6 and end == 0.0 for n, end in hyps)         # cut at the budget
    assert all((end == 0.0) == (n == 6) for n, end in hyps)
    for r in res:                                                 # an empty hypothesis is an end value alone
        for ids, lps, end, score in zip(r.sequences_ids, r.token_logprobs, r.end_logprobs, r.scores):
            if not ids:
                assert lps == [] and _bits(end) == _bits(score)


def _same(a, b, with_lp=False):
    for x, y in zip(a, b):
        assert x.sequences_ids == y.sequences_ids and x.scores == y.scores and x.no_speech_prob == y.no_speech_prob
        if with_lp:
            assert x.token_logprobs == y.token_logprobs and x.end_logprobs == y.end_logprobs


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_keyword_changes_nothing_else(setup, mode):
    cfg, _, model, enc = setup
    prompt = _prompt(cfg, True)
    kw = dict(MODES[mode], max_length=len(prompt) + BUDGET, suppress_tokens=_suppress(cfg), return_scores=True,
              return_no_speech_prob=True)
    plain = model.generate(enc, [prompt] * 3, **kw)
    with_lp = model.generate(enc, [prompt] * 3, return_token_logprobs=True, **kw)
    _same(with_lp, plain)
    assert all(r.token_logprobs == [] and r.end_logprobs == [] for r in plain)
    assert all(len(r.token_logprobs) == len(r.sequences_ids) for r in with_lp)


def test_a_call_with_logprobs_shares_a_run_with_one_without():
    """inter_threads=2 (one lane): while a long beam-2 run holds the lane, a beam-5 call that asks for log-probs and one
    that does not are queued from two threads; the next run takes both (mergeable() does not look at the keyword).
    Each gets exactly its solo result, log-probs included."""
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    model = Whisper("synthetic:micro", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=21)},
                    max_batch_size=3, max_beam_size=5, inter_threads=2)
    prompt = _prompt(cfg)
    kw = dict(beam_size=5, num_hypotheses=5, max_length=len(prompt) + 10, length_penalty=0.0, return_scores=True,
              return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2])
    batches = [[bench_audio(480000 if (i + j) % 3 else 250000, seed=50 + 10 * i + j) for j in range(3)] for i in range(2)]
    extra = [dict(return_token_logprobs=True), {}]
    solo = [model.generate(model.encode_pcm(b), [prompt] * 3, **kw, **e) for b, e in zip(batches, extra)]
    _check_identity(solo[0], 0.0)
    # the blocker: not mergeable with the two (beam 2), <eot> suppressed so that it runs its whole budget
    blocker_enc = model.encode_pcm(batches[0])
    blocker_kw = dict(beam_size=2, max_length=cfg.n_text_ctx, suppress_tokens=[cfg.eot])
    out, errs = [None, None], []
    encoded, go = threading.Barrier(3), threading.Event()

    def work(i):
        try:
            e = model.encode_pcm(batches[i])
            encoded.wait(timeout=120)
            assert go.wait(timeout=120)
            out[i] = model.generate(e, [prompt] * 3, **kw, **extra[i])
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    encoded.wait(timeout=120)
    st0 = model.decode_stats()
    tb = threading.Thread(target=lambda: model.generate(blocker_enc, [prompt] * 3, **blocker_kw))
    tb.start()
    t_end = time.time() + 30
    while model.decode_stats()["runs"] == st0["runs"] and time.time() < t_end:
        pass                                   # until the blocker's run has started
    go.set()
    for t in ts + [tb]:
        t.join()
    assert not errs, errs
    st = model.decode_stats()
    print(f"3 calls -> {st['runs'] - st0['runs']} decode runs, {st['requests'] - st0['requests']} requests")
    assert st["requests"] - st0["requests"] == 3 and st["runs"] - st0["runs"] == 2     # the two calls shared ONE run
    _same(out[0], solo[0], with_lp=True)
    _same(out[1], solo[1])
    assert all(r.token_logprobs == [] for r in out[1])


# ------------------------------------------------------------------------------------------------ against the oracle
RULE_TIE = 2e-2


def _oracle_token_logprobs(oracle, enc_b, prompt, ids, kw):
    """log-prob of token i = forced score of ids[:i + 1] minus forced score of ids[:i], each prefix scored with a budget
    of exactly its length (no <eot> is appended) at length_penalty 0; the empty prefix scores 0"""
    s = [0.0]
    for k in range(1, len(ids) + 1):
        s.append(forced_result(oracle, enc_b, prompt, ids[:k], dict(kw, max_length=len(prompt) + k)).scores[0])
    return np.diff(np.asarray(s, np.float64))


@pytest.fixture(scope="module")
def engine_hyps(setup):
    """greedy and the best beam-5 hypothesis of every chunk, decoded once: (ids, token log-probs) per mode and chunk"""
    cfg, w, model, enc = setup
    prompt = _prompt(cfg)
    out = {}
    for mode in ("greedy", "beam5"):
        kw = dict(MODES[mode], max_length=len(prompt) + 12, suppress_tokens=_suppress(cfg), length_penalty=0.0,
                  return_scores=True)
        res = model.generate(enc, [prompt] * 3, return_token_logprobs=True, **kw)
        out[mode] = [(r.sequences_ids[0], r.token_logprobs[0]) for r in res]
    from oracle.whisper import OracleWhisper
    return out, enc.to_numpy(), OracleWhisper(cfg, w, emulate_fp16=True), OracleWhisper(cfg, w, emulate_fp16=False)


@pytest.mark.parametrize("chunk", [0, 1, 2])
@pytest.mark.parametrize("mode", ["greedy", "beam5"])
def test_token_logprobs_against_the_oracle(setup, engine_hyps, mode, chunk):
    """max_i |engine_i - oracle_fp16_i| <= max(1e-3, 3 * band), band = max_i |oracle_fp16_i - oracle_fp32_i| on the same
    ids: two valid fp16 evaluation orders lie about 1.7 times further apart than fp16 lies from fp32 (profiles/NOTES.md,
    round 2 numerics), and the engine's order is a third one.  Steps where timestamp rule (e) is numerically tied
    (|rule margin| < 2e-2) may renormalise differently on the two sides: reported and left out, at most one per hypothesis."""
    cfg = setup[0]
    hyps, enc_np, o16, o32 = engine_hyps
    prompt = _prompt(cfg)
    ids, lps = hyps[mode][chunk]
    assert 4 <= len(ids) == len(lps) <= 12
    kw = dict(beam_size=1, suppress_tokens=_suppress(cfg), length_penalty=0.0, max_length=len(prompt) + 12)
    ref16 = _oracle_token_logprobs(o16, enc_np[chunk], prompt, ids, kw)
    ref32 = _oracle_token_logprobs(o32, enc_np[chunk], prompt, ids, kw)
    margins = forced_result(o16, enc_np[chunk], prompt, ids, kw).rule_margins or []
    tied = [i for i, m in enumerate(margins[:len(ids)]) if m == m and abs(m) < RULE_TIE]
    if tied:
        print(f"[{cfg.name}] {mode} chunk {chunk}: rule (e) tied at step(s) {tied}: left out")
    assert len(tied) <= 1
    use = [i for i in range(len(ids)) if i not in tied]
    band = float(np.abs(ref16 - ref32)[use].max())
    err = float(np.abs(np.asarray(lps, np.float64) - ref16)[use].max())
    bound = max(1e-3, 3 * band)
    print(f"[{cfg.name}] {mode} chunk {chunk}: max |engine - oracle fp16| {err:.3e}, band {band:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
