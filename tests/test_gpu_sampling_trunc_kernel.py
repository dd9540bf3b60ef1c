"""The TRUNC instantiations of the logits-rules kernel (dec_vocab.hip: lp_trunc_cut), alone through their test hook
fw_test_logits_rules_trunc (include/fwamd_test.h): ONE launch per case of tests/sampling_trunc_refs.py, one logits row
repeated over up to 64 rows with their own seeds, limits and temperatures through the two per-row tables.

  * the drawn id of EVERY live row equals the reference's draw inside its kept set S (no row is skipped: the CPU test at the
    end of the file holds the data to the margins that make that safe);
  * cand_lp / cand_val stay the plain processed log-prob of the draw and cum + it;
  * wherever the untruncated draw lies in S the truncated draw is that id;
  * rows with (0, 1.0) get the bits of the plain sampling launch, the rows of a done chunk are untouched;
  * with n_alt > 0 the alternatives are those of the untruncated launch, bit for bit;
  * a launch repeated gives the same bits; the hook refuses wrong arguments.

Vocabularies: micro (TXI = 0) and large-v3 on the micro geometry (TXI = 48)."""
import ctypes as C

import numpy as np
import pytest

import logits_rules_refs as lr
import sampling_trunc_refs as st

ABS_TOL = 2e-5              # device log-probs against the oracle's (tests/test_gpu_logits_rules.py)
SENT_I, SENT_F = lr.SENT_I, lr.SENT_F
VOCABS = ["micro", "large-v3"]
gpu = pytest.mark.gpu       # (not the whole file: its last test holds the data to its margins without a GPU)


@pytest.fixture(scope="module", params=VOCABS)
def env(request):
    from faster_whisper_amd import Whisper
    cfg, w, _ = st.env(request.param)
    model = Whisper("synthetic:rules", device="cuda", files={"config": cfg, "weights": w}, max_batch_size=2, max_beam_size=5)
    return request.param, cfg, model


def _opts(**opt):
    from faster_whisper_amd import _lib
    o = _lib.FwGenOpts()
    o.beam_size, o.patience, o.num_hypotheses, o.length_penalty = 1, 1.0, 1, 1.0
    o.repetition_penalty = float(opt.get("repetition_penalty", 1.0))
    o.no_repeat_ngram_size = int(opt.get("no_repeat_ngram_size", 0))
    o.max_length = 448
    o.max_initial_timestamp_index = int(opt.get("max_initial_timestamp_index", 50))
    o.suppress_blank = int(opt.get("suppress_blank", True))
    sup = np.asarray(opt.get("suppress_tokens") or [], dtype=np.int32)
    o.suppress_tokens = _lib.as_i32p(sup) if sup.size else None
    o.n_suppress_tokens = int(sup.size)
    o.sampling_topk, o.sampling_temperature, o.seed = int(opt.get("sampling_topk", 0)), 123.0, 999   # (the table holds the rows' own)
    o.min_new_tokens = 0
    return o, sup


def _launch(model, c, trunc=True, n_alt=0, k=None, p=None, rc_only=False, **more):
    """one launch of case `c` from sentinel-filled outputs: through fw_test_logits_rules_trunc, or (trunc=False) through the
    plain sampling hooks fw_test_logits_rules_ex / _alt; dict(val, tok, lp[, atok, alp])"""
    from faster_whisper_amd import _lib
    R, n = c.R, c.n
    o, keep = _opts(**dict(c.opt, **more))
    h = np.ascontiguousarray(np.asarray(c.hists, dtype=np.int32).reshape(R, n)) if n else np.zeros((R, 1), np.int32)
    lg = np.array(c.logits, dtype=np.float32, order="C")
    out = dict(val=np.full((R, lr.STRIDE), SENT_F, np.float32), tok=np.full((R, lr.STRIDE), SENT_I, np.int32),
               lp=np.full((R, lr.STRIDE), SENT_F, np.float32), logits=lg)
    dn = None if c.done is None else np.ascontiguousarray(c.done, dtype=np.int32)
    kk = np.ascontiguousarray(c.k if k is None else k, np.int32)
    pp = np.ascontiguousarray(c.p if p is None else p, np.float32)
    head = [model._replicas[0].handle, _lib.ptr(lg), R, _lib.ptr(h), n, _lib.ptr(c.cum), C.byref(o), int(c.with_ts),
            None if dn is None else _lib.ptr(dn), _lib.ptr(c.inv), _lib.ptr(c.seed), _lib.ptr(c.row0)]
    cand = [_lib.ptr(out["val"]), _lib.ptr(out["tok"]), _lib.ptr(out["lp"])]
    alt = []
    if n_alt:
        out["atok"] = np.full((R, n_alt), SENT_I, np.int32)
        out["alp"] = np.full((R, n_alt), SENT_F, np.float32)
        alt = [n_alt, _lib.ptr(out["atok"]), _lib.ptr(out["alp"])]
    if trunc:
        rc = model._lib.fw_test_logits_rules_trunc(*head, _lib.ptr(kk), _lib.ptr(pp), *cand, *(alt or [0, None, None]))
    elif n_alt:
        rc = model._lib.fw_test_logits_rules_alt(*head, *cand, *alt)
    else:
        rc = model._lib.fw_test_logits_rules_ex(*head, *cand)
    if rc_only:
        return rc, out
    _lib.check(rc)
    return out


def _same_bits(a, b):
    return np.array_equal(lr.bits(a), lr.bits(b))


def _case_ids(vocab):
    return [c.name for c in st.cases(vocab)]


@gpu
@pytest.mark.parametrize("ci", range(len(st.cases("micro"))), ids=_case_ids("micro"))
def test_truncated_draw_equals_the_reference(env, ci):
    vocab, cfg, model = env
    c, ref = st.cases(vocab)[ci], st.reference(vocab)[ci]
    got = _launch(model, c)
    plain = _launch(model, c, trunc=False)
    worst, moved, inside = 0.0, 0, 0
    for r in range(c.R):
        if ref[r] is None:                                   # a done chunk: nothing is written
            for key in ("val", "tok", "lp"):
                assert _same_bits(got[key][r], np.full(lr.STRIDE, SENT_I if key == "tok" else SENT_F, got[key].dtype)), (r, key)
            continue
        want = ref[r]
        tok, lp, val = int(got["tok"][r, 0]), got["lp"][r, 0], got["val"][r, 0]
        print(f"[{vocab}] {c.name} row {r}: k {c.k[r]} p {c.p[r]:.4f} T {c.T[r]}: |S| {len(want['S'])} of {want['n_live']}, drew {tok} "
              f"(reference {want['tok']}, untruncated {want['plain_tok']}), key gap {want['gap']:.2e}")
        assert tok == want["tok"], (r, tok, want["tok"])
        if want["n_live"] == 0:                              # nothing live: id 0 at -inf, as always
            assert np.isneginf(lp) and np.isneginf(val) and tok == 0
        else:
            # what is recorded is the plain log-prob of the draw: not tempered, not renormalised over S
            ref_lp = float(want["lp"][tok])
            worst = max(worst, abs(float(lp) - ref_lp))
            assert val == np.float32(c.cum[r] + lp)
        assert got["tok"][r, 1] == 0 and np.isneginf(got["val"][r, 1]) and np.isneginf(got["lp"][r, 1])
        assert _same_bits(got["val"][r, 2:], np.full(lr.STRIDE - 2, SENT_F, np.float32))
        # invariance: the noise of an id does not depend on S
        if want["plain_tok"] in set(want["S"].tolist()):
            inside += 1
            assert tok == want["plain_tok"] == int(plain["tok"][r, 0]), r
            assert _same_bits(got["lp"][r, :2], plain["lp"][r, :2]) and _same_bits(got["val"][r, :2], plain["val"][r, :2])
        else:
            moved += 1
        if c.k[r] == 0 and c.p[r] == 1.0:                    # no limit: the bits of the plain sampling kernel
            for key in ("val", "tok", "lp"):
                assert _same_bits(got[key][r], plain[key][r]), (r, key)
    assert worst < ABS_TOL, worst
    assert _same_bits(got["logits"], plain["logits"])        # the sparse rules edit the rows as always
    print(f"[{vocab}] {c.name}: {moved} of {c.R} draws moved by the limits, {inside} kept; worst |lp - oracle| {worst:.2e}")
    assert 4 * moved >= c.R
    again = _launch(model, c)                                # fixed-order reductions: the same bits
    for key in ("val", "tok", "lp"):
        assert _same_bits(again[key], got[key]), key


@gpu
@pytest.mark.parametrize("n_alt", [3, 8])
def test_alternatives_do_not_move(env, n_alt):
    """with n_alt > 0 the alternatives of a truncated launch are those of the untruncated one, bit for bit, and the draw is
    the one of the launch without alternatives"""
    vocab, cfg, model = env
    for c in st.cases(vocab):
        if c.name not in ("top-k, ties straddle the cut", "per-row state", "closed pair and a suppress list: 0, 1 and 2 live ids"):
            continue
        got = _launch(model, c, n_alt=n_alt)
        plain = _launch(model, c, trunc=False, n_alt=n_alt)
        bare = _launch(model, c)
        assert np.array_equal(got["atok"], plain["atok"]) and _same_bits(got["alp"], plain["alp"]), c.name
        for key in ("val", "tok", "lp"):
            assert _same_bits(got[key], bare[key]), (c.name, key)


@gpu
def test_rows_without_limits_equal_the_plain_kernel(env):
    """every row (0, 1.0) in a TRUNC launch: all 32 candidate slots of every row carry the plain sampling launch's bits"""
    vocab, cfg, model = env
    for c in st.cases(vocab):
        got = _launch(model, c, k=np.zeros(c.R, np.int32), p=np.ones(c.R, np.float32))
        plain = _launch(model, c, trunc=False)
        for key in ("val", "tok", "lp", "logits"):
            assert _same_bits(got[key], plain[key]), (c.name, key)


@gpu
def test_hook_refuses_wrong_arguments(env):
    from faster_whisper_amd import _lib
    vocab, cfg, model = env
    c = st.cases(vocab)[0]
    bad = [dict(k=np.full(c.R, -1, np.int32)), dict(p=np.zeros(c.R, np.float32)), dict(p=np.full(c.R, 1.5, np.float32)),
           dict(p=np.full(c.R, np.nan, np.float32)), dict(sampling_topk=1)]
    for kw in bad:
        rc, out = _launch(model, c, rc_only=True, **kw)
        assert rc == _lib.FW_EINVAL, kw
        assert (out["tok"] == SENT_I).all() and (out["val"] == SENT_F).all()
    # n_alt and its arrays go together
    o, keep = _opts(**c.opt)
    rc = model._lib.fw_test_logits_rules_trunc(model._replicas[0].handle, _lib.ptr(np.array(c.logits)), c.R, None, 0,
                                               _lib.ptr(c.cum), C.byref(o), 0, None, _lib.ptr(c.inv), _lib.ptr(c.seed),
                                               _lib.ptr(c.row0), _lib.ptr(c.k), _lib.ptr(c.p), _lib.ptr(np.zeros((c.R, 32), np.float32)),
                                               _lib.ptr(np.zeros((c.R, 32), np.int32)), _lib.ptr(np.zeros((c.R, 32), np.float32)),
                                               3, None, None)
    assert rc == _lib.FW_EINVAL


# ---------------------------------------------------------------------------------------------- the data, without a GPU
@pytest.mark.parametrize("vocab", VOCABS)
def test_trunc_reference_keeps_its_margins(vocab):
    """(no GPU: the counterpart of test_sampling_table_reference_has_no_near_tie)  The reference alone holds the data to what
    lets the GPU tests compare every row literally: the best two keys inside S more than 1e-4 apart; in every nucleus case
    |mass ahead - p Z| >= 1e-2 Z for every id of S_k; in every case at least a quarter of the draws moved by the limits; the
    same p cutting at different ids for different temperatures; 0, 1 and 2 live ids present."""
    cs, refs = st.cases(vocab), st.reference(vocab)
    assert len(cs) == len(st.cases("micro")) and [c.name for c in cs] == _case_ids("micro")
    n_live = set()
    for c, rows in zip(cs, refs):
        live = [r for r in rows if r is not None]
        assert all(r["gap"] > st.KEY_TIE for r in live), c.name
        if c.nucleus:
            assert all(r["margin"] >= st.MASS_MARGIN for r in live), (c.name, min(r["margin"] for r in live))
            assert any(r["margin"] < float("inf") for r in live)
        assert 4 * sum(r["tok"] != r["plain_tok"] for r in live) >= c.R, c.name
        n_live |= {r["n_live"] for r in live}
        if c.name == "nucleus, peaked row, three temperatures":
            sizes = {}
            for r in range(c.R):
                sizes.setdefault(float(c.p[r]), {})[float(c.T[r])] = len(rows[r]["S"])
            assert all(len(v) == 3 for v in sizes.values()) and any(len(set(v.values())) == 3 for v in sizes.values()), sizes
            assert sorted(v[1.0] for v in sizes.values()) == [1, 3, 5]
        if c.name == "top-k, distinct values":
            assert {len(r["S"]) for r in live} == {1, 2, 5, live[0]["n_live"] - 1, live[0]["n_live"]}
            assert sorted(set(c.k.tolist()))[3:6] == [live[0]["n_live"] - 1, live[0]["n_live"], live[0]["n_live"] + 1]
        if c.name == "top-k, ties straddle the cut":
            ties = [5, 69, 700, 1029, c.cfg.n_vocab - 1]
            for r in range(c.R):                                 # ties at the cut go to the lower ids
                kk = int(c.k[r])
                assert sorted(rows[r]["S"].tolist())[:min(kk, 5)] == ties[:min(kk, 5)] or kk > 5
                assert set(rows[r]["S"][:min(kk, 5)].tolist()) == set(ties[:min(kk, 5)])
    assert {0, 1, 2} <= n_live
