"""Whisper.score / fw_score end to end: teacher-forced log-probs of GIVEN transcripts.

  * raw mode against the fp32 oracle (tests/score_refs.py::model_ref: one decoder_full pass, float64 log-softmax) at every
    position of arbitrary sequences, timestamp tokens included;
  * rules mode against generate itself: scoring the ids a greedy generate() returned, under the same rule keywords, gives
    back generate's own token_logprobs / end_logprobs;
  * candidates per chunk, batch composition and position blocks move no bit;
  * every argument error is a ValueError that leaves the model usable."""
import numpy as np
import pytest

import score_refs as sr
from conftest import bench_audio, make_model

pytestmark = pytest.mark.gpu

# Raw mode vs the fp32 oracle, per value: the largest |engine - reference| over both geometries, the three chunks and five
# target seeds is printed by test_raw_mode_measured_over_seeds
#   (python -m pytest tests/test_gpu_score.py -m gpu -s -k measured);
# it was 2.11e-3 on micro and 7.31e-3 on tiny.en, at log-probs of -10 .. -20 (the targets are arbitrary ids: improbable
# ones): the engine computes in fp16 what the reference computes in fp32.  The bound is twice the measured figure.
PER_VALUE_TOL = {"micro": 4.3e-3, "tiny.en": 1.5e-2}
SEQ_TOL = 2e-3                 # the project's bound on a sequence's cumulative log-prob: 2e-3 * max(1, |ref|)


@pytest.fixture(scope="module", params=["micro", "tiny.en"])
def setup(request):
    from oracle.whisper import OracleWhisper
    from faster_whisper_amd.backend import StorageView
    cfg, w, model = make_model(request.param, seed=11, max_batch=4, max_beam=5)
    chunks = [bench_audio(480000, seed=1), bench_audio(200000, seed=2), bench_audio(480000, seed=3)[::-1].copy()]
    enc = model.encode(StorageView.from_array(model.log_mel(chunks)))
    o32 = OracleWhisper(cfg, {k: np.asarray(v) for k, v in w.items()}, emulate_fp16=False)
    return cfg, model, o32, enc, enc.to_numpy()


def _prompt(cfg, timestamps=False):
    return list(cfg.sot_sequence) + ([] if timestamps else [cfg.no_timestamps])


def _suppress(cfg):
    return sorted({cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, cfg.translate, cfg.transcribe, 1, 2, 7})


def _targets(cfg, rng, n):
    """text ids, a timestamp pair in the middle and one at the end"""
    tb = cfg.timestamp_begin
    t = rng.integers(10, 300, size=n).tolist()
    if n >= 6:
        t[0], t[n // 2], t[n // 2 + 1], t[-1] = tb, tb + 7, tb + 7, tb + 30
    return t


def _bits(res):
    """everything a score() call returned, as bytes"""
    return [(r.sequences_ids, [np.asarray(x, np.float32).tobytes() for x in r.token_logprobs],
             np.asarray(r.end_logprobs, np.float32).tobytes(), r.best_ids,
             [np.asarray(x, np.float32).tobytes() for x in r.best_logprobs]) for r in res]


def _raw_errors(setup, seed):
    cfg, model, o32, enc, enc_np = setup
    rng = np.random.default_rng(seed)
    prompt = _prompt(cfg, True)
    tg = [_targets(cfg, rng, n) for n in (17, 6, 33)]
    got = model.score(enc, [prompt] * 3, tg)
    worst = 0.0
    for b in range(3):
        ref = sr.model_ref(o32, enc_np[b], prompt, tg[b])
        g = np.array(got[b].token_logprobs[0] + [got[b].end_logprobs[0]], np.float64)
        r = np.append(ref["token_lp"], ref["end_lp"])
        gb = np.array(got[b].best_logprobs[0], np.float64)
        assert len(g) == len(tg[b]) + 1 == len(gb) == len(got[b].best_ids[0]) and got[b].sequences_ids[0] == tg[b]
        err = max(float(np.abs(g - r).max()), float(np.abs(gb - ref["best_lp"]).max()))
        cg, cr = got[b].cum_logprob(0), sr.cum32(r)
        print(f"[{cfg.name} seed {seed}] chunk {b}: {len(tg[b])} targets, worst per-value error {err:.2e}, "
              f"sequence {cg:.4f} vs {cr:.4f}")
        assert abs(cg - cr) < SEQ_TOL * max(1.0, abs(cr)), (b, cg, cr)
        # the arg-max is the oracle's wherever the oracle's best two are further apart than twice the per-value bound
        lg = sr.model_logits(o32, enc_np[b], prompt, tg[b])
        for k, (gi, ri) in enumerate(zip(got[b].best_ids[0], ref["best_ids"])):
            top = np.sort(sr.raw_lp64(lg[k]))[-2:]
            assert gi == ri or top[1] - top[0] < 2 * PER_VALUE_TOL[cfg.name], (b, k, gi, ri)
        worst = max(worst, err)
    return worst


def test_raw_mode_against_the_fp32_oracle(setup):
    assert _raw_errors(setup, 201) < PER_VALUE_TOL[setup[0].name]


def test_raw_mode_measured_over_seeds(setup):
    """the figure PER_VALUE_TOL is derived from"""
    worst = max(_raw_errors(setup, s) for s in (201, 202, 203, 204, 205))
    print(f"[{setup[0].name}] MEASURED raw mode vs fp32 oracle over 5 seeds: {worst:.3e}; PER_VALUE_TOL {PER_VALUE_TOL[setup[0].name]:.1e}")
    assert worst < PER_VALUE_TOL[setup[0].name]


@pytest.mark.parametrize("timestamps", [False, True, "eot"])
def test_round_trip_with_generate(setup, timestamps):
    """score(rules=True) of the ids a greedy generate() chose, under the same rule keywords, returns generate's own
    token_logprobs and end_logprobs BIT FOR BIT: the scoring kernel restates the rules kernel's arithmetic, and a position
    block gives a row the logits its decode step gave it (test_position_blocks_same_bits).
    "eot": everything but <eot> and three ids suppressed (test_gpu_model.py::test_generate_eot_and_early_finish), so that
    sequences CLOSE before the budget and the <eot> entry is compared too."""
    cfg, model, o32, enc, enc_np = setup
    prompt = _prompt(cfg, timestamps is True)
    rules = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, suppress_blank=True, suppress_tokens=_suppress(cfg),
                 max_initial_timestamp_index=50)
    if timestamps == "eot":
        keep = {cfg.eot, 20, 21, 22}
        rules = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, suppress_blank=False,
                     suppress_tokens=[t for t in range(cfg.n_vocab) if t not in keep])
    L = 24
    n_closed = 0
    gen = model.generate(enc, [prompt] * 3, beam_size=1, max_length=len(prompt) + L, return_scores=True,
                         return_token_logprobs=True, length_penalty=1, **rules)
    ids = [g.sequences_ids[0] for g in gen]
    res = model.score(enc, [prompt] * 3, ids, rules=True, **rules)
    for b, (g, r) in enumerate(zip(gen, res)):
        n = len(ids[b])
        assert n >= (1 if timestamps == "eot" else 4)
        a = np.asarray(g.token_logprobs[0], np.float32)
        s = np.asarray(r.token_logprobs[0], np.float32)
        closed = n < L                                           # (cut at the budget: generate reports end_logprob 0)
        print(f"[{cfg.name} ts={timestamps}] chunk {b}: {n} ids, closed={closed}, max |score - generate| = "
              f"{np.abs(a - s).max():.2e}, end {r.end_logprobs[0]:.6f} vs {g.end_logprobs[0]:.6f}")
        assert a.tobytes() == s.tobytes(), (b, a, s)
        assert r.best_ids[0][:n] == ids[b]                       # a greedy sequence is its own arg-max path
        assert np.asarray(r.best_logprobs[0][:n], np.float32).tobytes() == s.tobytes()
        n_closed += int(closed)
        if closed:
            assert np.float32(r.end_logprobs[0]).tobytes() == np.float32(g.end_logprobs[0]).tobytes()
            assert r.best_ids[0][n] == cfg.eot
            assert np.float32(r.score(0, length_penalty=1)).tobytes() == np.float32(g.scores[0]).tobytes()
        else:
            cum = np.float32(sr.cum32(r.token_logprobs[0]))
            assert np.float32(cum / np.float32(n)).tobytes() == np.float32(g.scores[0]).tobytes()
    assert n_closed >= 1 or timestamps != "eot"
    with pytest.raises(ValueError):
        model.score(enc, [prompt] * 3, ids, repetition_penalty=1.2)          # rule keywords without rules=True


def test_candidates_and_batch_composition_move_no_bit(setup):
    cfg, model, o32, enc, enc_np = setup
    from faster_whisper_amd.backend import StorageView
    rng = np.random.default_rng(7)
    prompt = _prompt(cfg, True)
    full = cfg.n_text_ctx - len(prompt) - 1                      # fills the text context exactly
    cands = [[_targets(cfg, rng, 9), [], _targets(cfg, rng, 21)],
             [_targets(cfg, rng, full), _targets(cfg, rng, 3)],           # (two candidates: the third row is filled up)
             [_targets(cfg, rng, 14), _targets(cfg, rng, 6), _targets(cfg, rng, 30)]]
    rules = dict(repetition_penalty=1.1, no_repeat_ngram_size=2, suppress_tokens=_suppress(cfg))
    for kw in (dict(), dict(rules=True, **rules)):
        together = model.score(enc, [prompt] * 3, cands, **kw)
        assert [len(r.sequences_ids) for r in together] == [3, 2, 3]
        assert together[0].token_logprobs[1] == [] and len(together[1].token_logprobs[0]) == full
        for h in range(3):                                        # candidate h of chunk b == the sequence scored alone
            alone = model.score(enc, [prompt] * 3, [c[h] if h < len(c) else [] for c in cands], **kw)
            for b in range(3):
                if h < len(cands[b]):
                    x, y = _bits([together[b]])[0], _bits([alone[b]])[0]
                    assert x[0][h] == y[0][0] and x[1][h] == y[1][0] and x[3][h] == y[3][0] and x[4][h] == y[4][0], (kw, b, h)
                    assert np.float32(together[b].end_logprobs[h]).tobytes() == np.float32(alone[b].end_logprobs[0]).tobytes()
        # B = 1 vs that chunk inside B = 3
        one = StorageView.from_array(enc_np[2:3])
        solo = model.score(one, [prompt], [cands[2]], **kw)
        assert _bits(solo) == _bits([together[2]]), kw


def test_position_blocks_and_a_long_prompt(setup):
    """FWAMD_POS_BLOCKS = 0 and = 1 (fw_test_knob 4) give the same bits; a 223-token prompt with 100 targets runs"""
    from faster_whisper_amd import _lib
    cfg, model, o32, enc, enc_np = setup
    lib = _lib.load()
    rng = np.random.default_rng(8)
    prev = [cfg.sot_prev] + rng.integers(10, 300, size=223 - 1 - len(_prompt(cfg, True))).tolist()
    long_prompt = prev + _prompt(cfg, True)
    assert len(long_prompt) == 223
    jobs = [(_prompt(cfg, True), [_targets(cfg, rng, n) for n in (33, 5, 40)], dict()),
            (long_prompt, [_targets(cfg, rng, 100), _targets(cfg, rng, 7), []],
             dict(rules=True, repetition_penalty=1.3, suppress_tokens=_suppress(cfg)))]
    res = {}
    try:
        for on in (0, 1):
            _lib.check(lib.fw_test_knob(4, on))
            res[on] = [_bits(model.score(enc, [p] * 3, t, **kw)) for p, t, kw in jobs]
    finally:
        _lib.check(lib.fw_test_knob(4, 1))
    assert res[0] == res[1]
    lp = np.frombuffer(res[1][1][0][1][0], np.float32)
    assert lp.shape == (100,) and not np.isnan(lp).any() and (lp <= 0).all()


def test_argument_errors_leave_the_model_usable(setup):
    from faster_whisper_amd import _lib
    import ctypes as C
    cfg, model, o32, enc, enc_np = setup
    prompt = _prompt(cfg)
    V, NT = cfg.n_vocab, cfg.n_text_ctx
    kw = dict(beam_size=1, max_length=len(prompt) + 8, return_scores=True, suppress_tokens=_suppress(cfg))
    before = [(g.sequences_ids, g.scores) for g in model.generate(enc, [prompt] * 3, **kw)]
    ok = [[11, 12], [13], []]
    bad = [
        ([prompt] * 3, [[11, V], [13], []]),                                  # a target id outside [0, V)
        ([prompt] * 3, [[11, -1], [13], []]),
        ([prompt[:-1] + [V]] * 3, ok),                                        # a prompt id outside [0, V)
        ([prompt] * 3, [[11] * (NT - len(prompt)), [13], []]),                # prompt + targets + <eot> above the context
        ([prompt, prompt + [11], prompt], ok),                                # prompts of different lengths
        ([prompt] * 3, [[[11]] * 6, [13], []]),                               # more candidates than max_beam_size
        ([prompt] * 2, ok[:2]),                                               # B != the encoder output's batch
    ]
    for p, t in bad:
        with pytest.raises(ValueError):
            model.score(enc, p, t)
    # what the Python front cannot express: null arguments, H out of range, offsets that decrease
    h = enc._owner.handle
    pf = np.asarray(prompt * 3, np.int32)
    po = np.arange(4, dtype=np.int32) * len(prompt)
    tf = np.asarray([11, 12, 13], np.int32)
    out = np.zeros(16, np.float32)
    i32, f32 = _lib.as_i32p, _lib.as_f32p
    for args in ((i32(pf), i32(po), i32(tf), i32(np.asarray([0, 2, 1, 3], np.int32)), 3, 1, None, f32(out), None, None),
                 (i32(pf), i32(po), i32(tf), i32(np.asarray([0, 2, 3, 3], np.int32)), 3, 0, None, f32(out), None, None),
                 (i32(pf), i32(po), i32(tf), i32(np.zeros(19, np.int32)), 3, 6, None, f32(out), None, None),
                 (i32(pf), i32(po), None, i32(np.asarray([0, 2, 3, 3], np.int32)), 3, 1, None, f32(out), None, None),
                 (i32(pf), i32(po), i32(tf), i32(np.asarray([0, 2, 3, 3], np.int32)), 3, 1, None, None, None, None),
                 (i32(pf), i32(po), i32(tf), i32(np.asarray([0, 2, 3, 3], np.int32)), 5, 1, None, f32(out), None, None)):
        assert model._lib.fw_score(h, enc._handle, *args) == _lib.FW_EINVAL
    assert (out == 0).all()
    good = model.score(enc, [prompt] * 3, ok)
    assert len(good[0].token_logprobs[0]) == 2 and good[2].token_logprobs[0] == []
    after = [(g.sequences_ids, g.scores) for g in model.generate(enc, [prompt] * 3, **kw)]
    assert after == before
