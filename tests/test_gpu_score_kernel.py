"""The scoring kernel (dec_vocab.hip: dec_score_kernel — the log-prob of a GIVEN token per logits row, raw or after the
decoding rules, with the row's arg-max) alone: ONE launch per case through the C ABI test hook fw_test_score_rows on
seeded logits rows, against the float64 restatement of tests/score_refs.py (tests/test_score_refs.py shows on the CPU
what those inputs hold, and that rule (e) is never a tie on them: no row is excluded here).

Exact: the arg-max id (ties: the lowest id), the -inf pattern, the sentinels of rows without a target, and the logits
buffer, which must come back bit for bit.  Values: within ABS_TOL of the float64 reference."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import logits_rules_refs as lr
import score_refs as sr

pytestmark = pytest.mark.gpu

# Measured: the largest |value - float64 reference| over every case of this file, the three vocabularies and the five
# seeds of score_refs.SEEDS is printed by test_measured_error_over_all_seeds
#   (python -m pytest tests/test_gpu_score_kernel.py -m gpu -s -k measured);
# it was 2.27e-6 (raw 1.49e-6, rules 2.27e-6, both on the 51 865-id vocabulary).  The bound is twice that, and below the
# 2e-5 that tests/test_gpu_logits_rules.py allows the rules kernel's log-probs.
ABS_TOL = 4.6e-6
assert ABS_TOL <= 2e-5


@pytest.fixture(scope="module", params=["micro", "tiny", "large-v3"])
def env(request):
    """a model is needed only for its config: the vocabularies of `tiny` (51 865) and `large-v3` (51 866: 51 of the
    kernel's 56 register slots) ride on a micro-sized network; the micro vocabulary (1 913) is no multiple of 1 024"""
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    full = get_config(request.param)
    micro = get_config("micro")
    keep = ("name", "n_mels", "d_model", "n_heads", "n_enc_layers", "n_dec_layers")
    cfg = dataclasses.replace(full, **{k: getattr(micro, k) for k in keep})
    model = Whisper("synthetic:score", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    return cfg, model


def _opts(**opt):
    from faster_whisper_amd import _lib
    o = _lib.FwGenOpts()
    o.repetition_penalty = float(opt.get("repetition_penalty", 1.0))
    o.no_repeat_ngram_size = int(opt.get("no_repeat_ngram_size", 0))
    o.max_initial_timestamp_index = int(opt.get("max_initial_timestamp_index", 50))
    o.suppress_blank = int(opt.get("suppress_blank", True))
    sup = np.asarray(opt.get("suppress_tokens") or [], dtype=np.int32)
    o.suppress_tokens = _lib.as_i32p(sup) if sup.size else None
    o.n_suppress_tokens = int(sup.size)
    # fields the scoring rules must ignore: values that would change a decode run
    o.beam_size, o.num_hypotheses, o.min_new_tokens, o.sampling_topk, o.max_length = 7, 3, 1000, 0, 1
    return o, sup


def _launch(model, logits, targets, hists=None, rules=None, with_ts=False, rc_only=False):
    """one launch from sentinel-filled outputs: dict(logits (as it comes back), lp, best_id, best_lp)"""
    from faster_whisper_amd import _lib
    R = logits.shape[0]
    lg = np.array(logits, dtype=np.float32, order="C")
    t = np.ascontiguousarray(targets, np.int32)
    hists = [[] for _ in range(R)] if hists is None else hists
    offs = np.zeros(R + 1, np.int32)
    offs[1:] = np.cumsum([len(h) for h in hists])
    flat = np.ascontiguousarray([x for h in hists for x in h] or [0], np.int32)
    o, keep = _opts(**rules) if rules is not None else (None, None)
    lp = np.full(R, sr.SENT_F, np.float32)
    bl = np.full(R, sr.SENT_F, np.float32)
    bi = np.full(R, sr.SENT_I, np.int32)
    rc = model._lib.fw_test_score_rows(model._replicas[0].handle, _lib.ptr(lg), R, _lib.ptr(t), _lib.ptr(flat), _lib.ptr(offs),
                                       C.byref(o) if o is not None else None, int(with_ts), _lib.ptr(lp), _lib.ptr(bi),
                                       _lib.ptr(bl))
    out = dict(logits=lg, lp=lp, best_id=bi, best_lp=bl)
    if rc_only:
        return rc, out
    _lib.check(rc)
    return out


def _check(what, logits, got, ref):
    """-> the largest absolute error of a finite value"""
    assert np.array_equal(lr.bits(got["logits"]), lr.bits(logits)), (what, "the launch wrote to the logits")
    assert np.array_equal(got["best_id"], ref["best_id"]), (what, got["best_id"], ref["best_id"])
    worst = 0.0
    for k in ("lp", "best_lp"):
        g, r = got[k].astype(np.float64), ref[k]
        assert not np.isnan(g).any(), (what, k)
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(g), fin) and np.array_equal(g[~fin], r[~fin]), (what, k, g, r)
        if fin.any():
            worst = max(worst, float(np.abs(g[fin] - r[fin]).max()))
    return worst


def _run_raw(env, seed):
    cfg, model = env
    worst = 0.0
    for what, lg, t in sr.raw_cases(cfg, seed):
        err = _check(what, lg, _launch(model, lg, t), sr.score_rows_ref(cfg, lg, t))
        print(f"[V={cfg.n_vocab} seed {seed}] raw, {what}: worst |value - ref64| = {err:.2e}")
        worst = max(worst, err)
    return worst


def _run_rules(env, seed):
    cfg, model = env
    worst = 0.0
    for what, lg, t, hists, opt, with_ts in sr.rule_cases(cfg, seed):
        ref = sr.score_rows_ref(cfg, lg, t, hists, opt, with_ts)
        m = np.array(ref["margins"])
        assert (np.abs(m[np.isfinite(m)]) >= sr.MARGIN).all(), (what, m)      # a condition on the inputs
        err = _check(what, lg, _launch(model, lg, t, hists, opt, with_ts), ref)
        print(f"[V={cfg.n_vocab} seed {seed}] rules, {what}: worst |value - ref64| = {err:.2e}")
        worst = max(worst, err)
    return worst


def test_raw_rows(env):
    """vocabulary and target edges, rows 1 and 37, rows without a target, -inf rows, tied maxima, magnitude 1e4"""
    assert _run_raw(env, sr.SEEDS[0]) < ABS_TOL


def test_rules_rows(env):
    """penalty + n-gram, the first position, open and closed pairs, rule (e) on both sides, n = 0 and n = n_text_ctx - 1"""
    assert _run_rules(env, sr.SEEDS[0]) < ABS_TOL


def test_measured_error_over_all_seeds(env):
    """the figure ABS_TOL is derived from: every case on every seed"""
    cfg = env[0]
    raw = max(_run_raw(env, s) for s in sr.SEEDS)
    rules = max(_run_rules(env, s) for s in sr.SEEDS)
    print(f"[V={cfg.n_vocab}] MEASURED over seeds {sr.SEEDS}: raw {raw:.3e}, rules {rules:.3e}; ABS_TOL {ABS_TOL:.1e}")
    assert max(raw, rules) < ABS_TOL


def _rules_kernel_first(model, logits, hists, rules, with_ts):
    """the rules kernel on the same rows through fw_test_logits_rules_lp — greedy, beam 1, min_new_tokens 0, cum 0, one
    launch per history length (that hook takes one n per launch) -> (cand_tok[0], cand_lp[0]) of every row"""
    from faster_whisper_amd import _lib
    o, keep = _opts(**rules)
    o.beam_size, o.num_hypotheses, o.sampling_topk, o.min_new_tokens = 1, 1, 1, 0
    o.patience, o.length_penalty = 1.0, 1.0
    R = logits.shape[0]
    tok = np.full(R, sr.SENT_I, np.int32)
    lp = np.full(R, sr.SENT_F, np.float32)
    for n in sorted({len(h) for h in hists}):
        rows = [r for r in range(R) if len(hists[r]) == n]
        lg = np.ascontiguousarray(logits[rows], np.float32)
        h = np.ascontiguousarray([hists[r] for r in rows], np.int32).reshape(len(rows), n) if n else np.zeros((len(rows), 1), np.int32)
        cum = np.zeros(len(rows), np.float32)
        cv, ct = np.zeros((len(rows), 2), np.float32), np.full((len(rows), 2), sr.SENT_I, np.int32)
        cl = np.full((len(rows), 2), sr.SENT_F, np.float32)
        _lib.check(model._lib.fw_test_logits_rules_lp(model._replicas[0].handle, _lib.ptr(lg), len(rows), _lib.ptr(h), n,
                                                      _lib.ptr(cum), C.byref(o), int(with_ts), _lib.ptr(cv), _lib.ptr(ct),
                                                      _lib.ptr(cl)))
        tok[rows], lp[rows] = ct[:, 0], cl[:, 0]
    return tok, lp


def test_same_bits_as_the_rules_kernel(env):
    """The contract Whisper.score documents, at kernel level: a row scored against the rules kernel's first candidate
    gets that candidate's id as its arg-max and the BITS of its log-prob, as the target's value and as the best value
    (the two kernels hold and reduce the row through the same device functions, dec_vocab.hip).  Every rule-mode row of
    score_refs.rule_cases, and two rows with nothing left (all -inf): id 0 at -inf on both sides.  No tolerance."""
    cfg, model = env
    cases = [(what, lg, hists, opt, with_ts) for what, lg, _, hists, opt, with_ts in sr.rule_cases(cfg, sr.SEEDS[0])]
    dead = np.full((2, cfg.n_vocab), -np.inf, np.float32)
    cases.append(("everything masked", dead, [[], [40, 41]], dict(suppress_tokens=lr.suppress_list(cfg)), True))
    for what, lg, hists, opt, with_ts in cases:
        hists = [list(h) for h in hists]
        tok, lp = _rules_kernel_first(model, lg, hists, opt, with_ts)
        got = _launch(model, lg, tok, hists, opt, with_ts)
        print(f"[V={cfg.n_vocab}] {what}: rules kernel {tok.tolist()} {lp.tolist()}; score kernel {got['best_id'].tolist()} "
              f"{got['best_lp'].tolist()} {got['lp'].tolist()}")
        assert (tok >= 0).all() and not np.isnan(lp).any(), (what, tok, lp)
        assert np.array_equal(got["best_id"], tok), (what, got["best_id"], tok)
        assert np.array_equal(lr.bits(got["best_lp"]), lr.bits(lp)), (what, got["best_lp"], lp)
        assert np.array_equal(lr.bits(got["lp"]), lr.bits(lp)), (what, got["lp"], lp)
        if what == "everything masked":
            assert (tok == 0).all() and (lp == -np.inf).all(), (tok, lp)
        else:
            assert np.isfinite(lp).all(), (what, lp)


def test_hook_refuses_ids_out_of_range(env):
    from faster_whisper_amd import _lib
    cfg, model = env
    V = cfg.n_vocab
    lg = lr.signed_rows(V, 2, np.random.default_rng(3))
    good = _launch(model, lg, [5, 6], [[1, 2], [3]], dict(repetition_penalty=1.2), False)
    for t, hists in (([5, V], [[1, 2], [3]]), ([5, 6], [[1, V], [3]]), ([5, 6], [[1, 2], [-1]]),
                     ([5, 6], [[1] * cfg.n_text_ctx, [3]])):
        rc, out = _launch(model, lg, t, hists, dict(repetition_penalty=1.2), False, rc_only=True)
        assert rc == _lib.FW_EINVAL, (t, [len(h) for h in hists])
        assert (out["lp"] == sr.SENT_F).all() and (out["best_id"] == sr.SENT_I).all()
    again = _launch(model, lg, [5, 6], [[1, 2], [3]], dict(repetition_penalty=1.2), False)
    assert again["lp"].tobytes() == good["lp"].tobytes()
