"""The three kernels behind generate(return_alternatives=N), each alone through its test hook (include/fwamd_test.h):

  1-3. the ALT instantiations of the logits-rules kernel (fw_test_logits_rules_alt) against the launch without
       alternatives (fw_test_logits_rules_ex, bit for bit: candidates and the edited logits) and against the oracle's rule
       restatement (oracle/whisper.py::_process_logits, then a sort by (-log-prob, id)): ids exact, values within the 2e-5
       tests/test_gpu_logits_rules.py holds the same registers to;
  4.   the ALT instantiations of the beam update (fw_test_dec_beam_update_alt): the path of a finished hypothesis against
       tests/alternatives_refs.py, everything else against tests/token_logprob_refs.py, uniform and ragged;
  5.   the gather kernel (fw_test_alt_gather) against numpy indexing;
  6.   each hook refuses a wrong test with FW_EINVAL and leaves the outputs alone.

Logits are test_gpu_logits_rules.py's family: every row holds DISTINCT multiples of 1/4096, so the order is decided
exactly.  Vocabularies: micro (the per-lane class test, TXI = 0) and large-v3 on the micro geometry (TXI = 48)."""
import ctypes as C

import numpy as np
import pytest

import logits_rules_refs as lr
from alternatives_refs import beam_update_alt_ref, gather_ref, top_n
from decode_state_refs import FIN_CAP
from token_logprob_refs import lp_state

pytestmark = pytest.mark.gpu

ABS_TOL = 2e-5
SENT_I, SENT_F = lr.SENT_I, lr.SENT_F


@pytest.fixture(scope="module", params=["micro", "large-v3"])
def env(request):
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    from oracle.whisper import OracleWhisper
    import dataclasses
    full = get_config(request.param)
    micro = get_config("micro")
    keep = ("name", "n_mels", "d_model", "n_heads", "n_enc_layers", "n_dec_layers")
    cfg = dataclasses.replace(full, **{k: getattr(micro, k) for k in keep if hasattr(micro, k)})
    w = synthetic_weights(cfg, seed=5)
    model = Whisper("synthetic:rules", device="cuda", files={"config": cfg, "weights": w}, max_batch_size=2,
                    max_beam_size=16)
    return cfg, model, OracleWhisper(cfg, w)


def _logits(cfg, R, rng, scale=1.0):
    """every row: V DISTINCT multiples of 1/4096 in [0, 16) (times `scale`, a power of two), shuffled"""
    V = cfg.n_vocab
    assert V <= 65536
    base = rng.permutation(65536)[:V].astype(np.float32) / np.float32(4096.0)
    out = np.stack([rng.permutation(base) for _ in range(R)]) * np.float32(scale)
    return np.ascontiguousarray(out, dtype=np.float32)


def _opts(K, **opt):
    from faster_whisper_amd import _lib
    o = _lib.FwGenOpts()
    o.beam_size, o.patience, o.num_hypotheses, o.length_penalty = K, 1.0, 1, 1.0
    o.repetition_penalty = float(opt.get("repetition_penalty", 1.0))
    o.no_repeat_ngram_size = int(opt.get("no_repeat_ngram_size", 0))
    o.max_length = 448
    o.max_initial_timestamp_index = int(opt.get("max_initial_timestamp_index", 50))
    o.suppress_blank = int(opt.get("suppress_blank", True))
    sup = np.asarray(opt.get("suppress_tokens") or [], dtype=np.int32)
    o.suppress_tokens = _lib.as_i32p(sup) if sup.size else None
    o.n_suppress_tokens = int(sup.size)
    o.sampling_topk = int(opt.get("sampling_topk", 1))
    o.sampling_temperature = float(opt.get("sampling_temperature", 1.0))
    o.seed = int(opt.get("seed", 0))
    o.min_new_tokens = int(opt.get("min_new_tokens", 0))
    return o, sup          # (sup: keeps the array the options point to alive)


def _launch(model, logits, hists, cum, K, with_ts, n_alt=0, done=None, table=None, rc_only=False, **opt):
    """one launch from sentinel-filled outputs: n_alt == 0 through fw_test_logits_rules_ex, otherwise through
    fw_test_logits_rules_alt; dict(logits, val, tok, lp[, atok, alp]) as the launch leaves them"""
    from faster_whisper_amd import _lib
    R, V = logits.shape
    n = len(hists[0]) if hists is not None else 0
    o, keep = _opts(K, **opt)
    h = np.ascontiguousarray(np.asarray(hists, dtype=np.int32).reshape(R, n)) if n else np.zeros((R, 1), np.int32)
    lg = np.array(logits, dtype=np.float32, order="C")
    cv = np.full((R, lr.STRIDE), SENT_F, np.float32)
    cl = np.full((R, lr.STRIDE), SENT_F, np.float32)
    ct = np.full((R, lr.STRIDE), SENT_I, np.int32)
    cum = np.ascontiguousarray(cum, dtype=np.float32)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    tab = [None, None, None]
    if table is not None:
        tab = [np.ascontiguousarray(table[0], np.float32), np.ascontiguousarray(table[1], np.uint64),
               np.ascontiguousarray(table[2], np.int32)]
    args = [model._replicas[0].handle, _lib.ptr(lg), R, _lib.ptr(h), n, _lib.ptr(cum), C.byref(o), int(with_ts),
            None if dn is None else _lib.ptr(dn), *[None if t is None else _lib.ptr(t) for t in tab], _lib.ptr(cv),
            _lib.ptr(ct), _lib.ptr(cl)]
    out = dict(logits=lg, val=cv, tok=ct, lp=cl)
    if n_alt == 0:
        rc = model._lib.fw_test_logits_rules_ex(*args)
    else:
        na = max(n_alt, 1)
        out["atok"] = np.full((R, na), SENT_I, np.int32)
        out["alp"] = np.full((R, na), SENT_F, np.float32)
        rc = model._lib.fw_test_logits_rules_alt(*args, n_alt, _lib.ptr(out["atok"]), _lib.ptr(out["alp"]))
    if rc_only:
        return rc, out
    _lib.check(rc)
    return out


def _same_bits(a, b):
    return np.array_equal(lr.bits(a), lr.bits(b))


def _oracle_rows(oracle, logits, hists, with_ts, **opt):
    V = logits.shape[1]
    mask = None
    if opt.get("suppress_tokens"):
        mask = np.zeros(V, dtype=bool)
        mask[[t for t in opt["suppress_tokens"] if 0 <= t < V]] = True
    return [oracle._process_logits(logits[r], list(hists[r]) if hists is not None else [], with_ts, mask,
                                   bool(opt.get("suppress_blank", True)), int(opt.get("max_initial_timestamp_index", 50)),
                                   float(opt.get("repetition_penalty", 1.0)), int(opt.get("no_repeat_ngram_size", 0)),
                                   int(opt.get("min_new_tokens", 0))) for r in range(logits.shape[0])]


def _check_alt_launch(env, logits, hists, cum, K, with_ts, n_alt, **opt):
    """the three properties of group 1 for one launch; returns the launch with alternatives"""
    cfg, model, oracle = env
    plain = _launch(model, logits, hists, cum, K, with_ts, **opt)
    got = _launch(model, logits, hists, cum, K, with_ts, n_alt=n_alt, **opt)
    for k in ("val", "tok", "lp", "logits"):       # candidates (all 32 slots, sentinels included) and the edited rows
        assert _same_bits(got[k], plain[k]), (k, K, n_alt)
    m = min(n_alt, 2 * K)
    assert np.array_equal(got["atok"][:, :m], got["tok"][:, :m]) and _same_bits(got["alp"][:, :m], got["lp"][:, :m])
    worst = 0.0
    for r, lp in enumerate(_oracle_rows(oracle, logits, hists, with_ts, **opt)):
        ids, vals = top_n(lp, n_alt)
        assert np.array_equal(got["atok"][r], ids), (r, got["atok"][r], ids)
        fin = np.isfinite(vals)
        assert np.array_equal(np.isfinite(got["alp"][r]), fin) and np.isneginf(got["alp"][r][~fin]).all()
        if fin.any():
            worst = max(worst, float(np.abs(got["alp"][r][fin] - vals[fin]).max()))
    assert worst < ABS_TOL, worst
    return got, worst


RULE_SETS = {
    "plain": (False, dict()),
    "rules": (True, dict(repetition_penalty=1.3, no_repeat_ngram_size=2)),
}


@pytest.mark.parametrize("rules", sorted(RULE_SETS))
@pytest.mark.parametrize("K,n_alts", [(1, (1, 2, 3, 8)), (5, (1, 3, 8)), (16, (1, 3, 8))])
def test_rules_kernel_alternatives(env, K, n_alts, rules):
    """R = 2K rows; n_alt below, at and above 2K; with and without the timestamp rules, repetition penalty 1.3 and n-gram 2
    on per-row histories"""
    cfg = env[0]
    with_ts, opt = RULE_SETS[rules]
    R = 2 * K
    rng = np.random.default_rng(100 + K)
    logits = _logits(cfg, R, rng)
    cum = -rng.random(R).astype(np.float32) * 3
    hists = lr.row_histories(cfg, R, 4) if with_ts else None
    if with_ts:
        logits[:, cfg.timestamp_begin:] -= 8.0      # rule (e) far from its threshold: the text ids stay
        opt = dict(opt, suppress_tokens=lr.suppress_list(cfg))
    worst = 0.0
    for n_alt in n_alts:
        _, w = _check_alt_launch(env, logits, hists, cum, K, with_ts, n_alt, **opt)
        worst = max(worst, w)
    print(f"[V={cfg.n_vocab}] K={K} {rules}: worst |alt_lp - oracle| = {worst:.2e}")


@pytest.mark.parametrize("n_alt", [3, 8])
def test_ties_give_ascending_ids(env, n_alt):
    """two, three and n_alt + 1 equal logits at the top of a row: the alternatives list them by ascending id"""
    cfg, model, _ = env
    rng = np.random.default_rng(7)
    logits = _logits(cfg, 4, rng)
    top = np.float32(17.0)
    groups = [[900, 5], [1200, 64, 63], sorted(rng.permutation(min(cfg.eot, 1500))[:n_alt + 1].tolist(), reverse=True),
              [3, 1024 if cfg.n_vocab > 2048 else 77]]
    for r, g in enumerate(groups):
        logits[r, g] = top
    got = _launch(model, logits, None, np.zeros(4, np.float32), 1, False, n_alt=n_alt, suppress_blank=False)
    for r, g in enumerate(groups):
        m = min(len(g), n_alt)
        assert got["atok"][r, :m].tolist() == sorted(g)[:m], (r, got["atok"][r], sorted(g))
        assert (got["alp"][r, :m] == got["alp"][r, 0]).all()
        if m < n_alt:
            assert got["alp"][r, m] < got["alp"][r, 0]


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("n_alt", [3, 8])
def test_few_live_ids_and_done_chunks(env, K, n_alt):
    """a suppress list that leaves 0, 1 and n_alt - 1 live ids: the tail is (0, -inf); the rows of a chunk marked done keep
    the caller's sentinel"""
    cfg, model, oracle = env
    R = 2 * K
    rng = np.random.default_rng(11)
    logits = _logits(cfg, R, rng)
    cum = np.zeros(R, np.float32)
    tb = cfg.timestamp_begin
    hist = [[tb + 1, tb + 1]] * R                     # a closed pair: no timestamp is allowed, text and <eot> only
    ids = [9, 70, 300, 276, 5, 64, 33][:n_alt - 1]
    for left in (0, 1, n_alt - 1):
        keep = ids[:left]
        sup = [t for t in range(tb) if t not in keep]
        got = _launch(model, logits, hist, cum, K, True, n_alt=n_alt, suppress_tokens=sup, done=[0, 1])
        plain = _launch(model, logits, hist, cum, K, True, suppress_tokens=sup, done=[0, 1])
        for k in ("val", "tok", "lp", "logits"):
            assert _same_bits(got[k], plain[k]), k
        assert (got["atok"][K:] == SENT_I).all() and (got["alp"][K:] == np.float32(SENT_F)).all()     # chunk 1: done
        for r in range(K):
            want = sorted(keep, key=lambda t: (-logits[r, t], t))
            assert got["atok"][r, :left].tolist() == want, (left, r, got["atok"][r], want)
            assert np.isfinite(got["alp"][r, :left]).all()
            assert (got["atok"][r, left:] == 0).all() and np.isneginf(got["alp"][r, left:]).all()


@pytest.mark.parametrize("form", ["table", "opts"])
@pytest.mark.parametrize("n_alt", [1, 8])
def test_sampling_instantiation(env, n_alt, form):
    """8 sampling rows with per-row temperature, seed and row0 (table), or the options' own (opts): the drawn token, its
    cand_val and cand_lp are those of the launch without alternatives, bit for bit; the alternatives are those of the
    greedy launch on the same rows (the same distribution), bit for bit"""
    cfg, model, _ = env
    R = 8
    rng = np.random.default_rng(31)
    logits = _logits(cfg, R, rng, scale=0.5)
    cum = -rng.random(R).astype(np.float32)
    hists = [[11, 12, 13 + r] for r in range(R)]
    opt = dict(suppress_tokens=lr.suppress_list(cfg), repetition_penalty=1.3)
    table = None
    if form == "table":
        table = (1.0 / np.linspace(0.5, 1.2, R), (np.arange(R, dtype=np.uint64) * np.uint64(7919) + np.uint64(5 << 32)),
                 np.array([0, 0, 0, 3, 3, 5, 5, 5]))
    smp = dict(opt, sampling_topk=0, sampling_temperature=0.7, seed=(3 << 32) | 77)
    plain = _launch(model, logits, hists, cum, 1, False, table=table, **smp)
    got = _launch(model, logits, hists, cum, 1, False, n_alt=n_alt, table=table, **smp)
    for k in ("val", "tok", "lp", "logits"):
        assert _same_bits(got[k], plain[k]), k
    assert (got["tok"][:, 0] >= 0).all() and np.isfinite(got["val"][:, 0]).all()
    greedy = _launch(model, logits, hists, cum, 1, False, n_alt=n_alt, **opt)
    assert np.array_equal(got["atok"], greedy["atok"]) and _same_bits(got["alp"], greedy["alp"])
    assert np.isfinite(got["alp"]).all()
    # the drawn token's log-prob is the one its entry among the alternatives carries, when it is there
    for r in range(R):
        hit = np.nonzero(got["atok"][r] == got["tok"][r, 0])[0]
        if hit.size:
            assert _same_bits(got["alp"][r, hit[0]], got["lp"][r, 0])
    if n_alt == 8:
        assert any(got["tok"][r, 0] != got["atok"][r, 0] for r in range(R)), "every draw was the arg-max: no test of the draw"


# ------------------------------------------------------------------------------------------------------ beam update
B, NT, P = 2, 16, 3
STATE_KEYS = ("hist2", "kvidx2", "cur_tok", "done", "n_done", "n_fin", "fin_tok", "fin_len")
PATH_SENT = 0xEE


def _beam_call(model, st, cv, ct, cl, path, *, K, V, step, budget, max_fin, eot, ptab=None, hook="alt", rc_only=False):
    from faster_whisper_amd import _lib as L
    R, cur = B * K, step & 1
    pos = (P if ptab is None else max(ptab)) - 1 + step
    hist = np.ascontiguousarray(st["hist2"][cur, :, :step], np.int32)
    lphist = np.ascontiguousarray(st["lphist2"][cur, :, :step], np.float32)
    kvidx = np.ascontiguousarray(st["kvidx2"][cur, :, :pos], np.uint8)
    cum = np.ascontiguousarray(st["cum2"][cur], np.float32)
    cv, ct, cl = (np.ascontiguousarray(cv, np.float32), np.ascontiguousarray(ct, np.int32),
                  np.ascontiguousarray(cl, np.float32))
    out = {k: np.ascontiguousarray(st[k]).copy() for k in ("done", "n_done", "n_fin", "fin_tok", "fin_len", "fin_score",
                                                            "fin_cum", "fin_lp")}
    out["hist2"] = np.zeros((2, R, NT), np.int32)
    out["lphist2"] = np.zeros((2, R, NT), np.float32)
    out["kvidx2"] = np.zeros((2, R, NT), np.uint8)
    out["cum2"] = np.zeros((2, R), np.float32)
    out["cur_tok"] = np.zeros(R, np.int32)
    out["fin_path"] = None if path is None else np.ascontiguousarray(path, np.uint8).copy()
    args = [model._replicas[0].handle, B, K, NT, V, P, step, budget, max_fin, 0.0, eot, L.ptr(cv), L.ptr(ct), L.ptr(cl),
            L.ptr(hist), L.ptr(lphist), L.ptr(kvidx), L.ptr(cum), SENT_I, SENT_F, L.ptr(out["done"]), L.ptr(out["n_done"]),
            L.ptr(out["n_fin"]), L.ptr(out["fin_tok"]), L.ptr(out["fin_len"]), L.ptr(out["fin_score"]), L.ptr(out["fin_cum"]),
            L.ptr(out["fin_lp"]), L.ptr(out["hist2"]), L.ptr(out["lphist2"]), L.ptr(out["kvidx2"]), L.ptr(out["cum2"]),
            L.ptr(out["cur_tok"])]
    if hook == "lp":
        rc = model._lib.fw_test_dec_beam_update_lp(*args)
    else:
        pt = None if ptab is None else np.ascontiguousarray(ptab, np.int32)
        rc = model._lib.fw_test_dec_beam_update_alt(*args, None if pt is None else L.ptr(pt),
                                                    None if path is None else L.ptr(out["fin_path"]))
    if rc_only:
        return rc, out
    L.check(rc)
    return out


def _cands(rng, K, eot):
    """[B K][2K] candidates: distinct values (rows sorted descending), tokens = 100 + flat index inside the chunk,
    log-probs = recognisable negatives (they are only carried)"""
    R, Cn = B * K, 2 * K
    v = rng.permutation(40 * 64)[:R * Cn].astype(np.float32).reshape(R, Cn) / np.float32(-64.0) - np.float32(1 / 64)
    v = -np.sort(-v, axis=1)
    t = np.tile(100 + np.arange(K * Cn, dtype=np.int32).reshape(K, Cn), (B, 1))
    lp = -(1.0 + np.arange(R * Cn, dtype=np.float32).reshape(R, Cn) / np.float32(8.0))
    assert eot < 100
    return v, t, lp


def _merged(v):
    f = v.reshape(-1)
    return [int(i) for i in np.argsort(-f, kind="stable") if f[i] != -np.inf]


def _state(rng, K, step, ptab=None, **kw):
    R = B * K
    Pm = P if ptab is None else max(ptab)
    hist = rng.integers(0, 90, (R, step)).astype(np.int32)
    lphist = -rng.random((R, step)).astype(np.float32) * 9
    kvidx = rng.integers(0, K, (R, Pm - 1 + step)).astype(np.uint8)
    cum = -rng.random(R).astype(np.float32) * 5
    st = lp_state(B, K, NT, step, Pm, hist, lphist, kvidx, cum, SENT_I, SENT_F, **kw)
    for c in range(B if ptab is not None else 0):      # a ragged launch: chunk c's rows hold ptab[c] - 1 + step bytes
        st["kvidx2"][step & 1, c * K:(c + 1) * K, ptab[c] - 1 + step:] = SENT_I & 0xFF
    return st


def _check_beam(model, st, cv, ct, cl, path, ptab=None, **kw):
    got = _beam_call(model, st, cv, ct, cl, path, ptab=ptab, **kw)
    ref, rpath = beam_update_alt_ref(st, cv, ct, cl, path, P=P, lp_pow=0.0, ptab=ptab,
                                     **{k: v for k, v in kw.items() if k != "V"})
    for k in STATE_KEYS:
        assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:8])
    for k in ("cum2", "fin_cum", "lphist2", "fin_lp"):
        assert _same_bits(got[k], ref[k]), k
    assert np.array_equal(got["fin_score"].astype(np.float64), ref["fin_score"])
    assert np.array_equal(got["fin_path"], rpath), np.argwhere(got["fin_path"] != rpath)[:8]
    return got, rpath


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("step", [0, 1, 5])
def test_beam_update_records_the_path_on_eot(env, K, step):
    """the best candidate of chunk 0 is <eot>: one finished hypothesis, whose path is its source row's slot-table bytes from
    P - 1 on and then the row's own beam index; chunk 1 records nothing"""
    model = env[1]
    rng = np.random.default_rng(200 + 10 * K + step)
    eot = 90
    cv, ct, cl = _cands(rng, K, eot)
    m = _merged(cv[:1] if step == 0 else cv[:K])
    ct[:K].reshape(-1)[m[0]] = eot
    st = _state(rng, K, step)
    path = np.full((B, FIN_CAP, NT + 1), PATH_SENT, np.uint8)
    kw = dict(K=K, V=400, step=step, budget=12, max_fin=FIN_CAP - K, eot=eot)
    got, rpath = _check_beam(model, st, cv, ct, cl, path, **kw)
    src = m[0] // (2 * K)
    assert got["n_fin"].tolist() == [1, 0]
    assert got["fin_path"][0, 0, :step].tolist() == st["kvidx2"][step & 1, src, P - 1:P - 1 + step].tolist()
    assert got["fin_path"][0, 0, step] == src and (got["fin_path"][0, 0, step + 1:] == PATH_SENT).all()
    assert (got["fin_path"][0, 1:] == PATH_SENT).all() and (got["fin_path"][1] == PATH_SENT).all()
    # a null path pointer: the launch of fw_test_dec_beam_update_lp, bit for bit
    a = _beam_call(model, st, cv, ct, cl, None, **kw)
    b = _beam_call(model, st, cv, ct, cl, None, hook="lp", **kw)
    for k in a:
        if k != "fin_path":
            assert _same_bits(a[k], b[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k]), k
    for k in a:                                      # ... and what the path launch leaves of everything else
        if k != "fin_path":
            assert _same_bits(a[k], got[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], got[k]), k


@pytest.mark.parametrize("K", [1, 3])
def test_beam_update_last_step_fin_cap_and_done(env, K):
    """the last step finishes every slot (a real token, or <eot>); nothing is written past FIN_CAP or for a chunk that was
    done on entry"""
    model = env[1]
    rng = np.random.default_rng(300 + K)
    step, eot = 5, 90
    cv, ct, cl = _cands(rng, K, eot)
    m = _merged(cv[:K])
    if K > 1:
        ct[:K].reshape(-1)[m[1]] = eot
    path = rng.integers(200, 250, (B, FIN_CAP, NT + 1)).astype(np.uint8)
    kw = dict(K=K, V=400, step=step, budget=step + 1, max_fin=FIN_CAP - K, eot=eot)
    st = _state(rng, K, step, done=[0, 1], n_done=1, n_fin=[2, 3])
    got, _ = _check_beam(model, st, cv, ct, cl, path, **kw)
    assert got["n_fin"].tolist() == [2 + K, 3] and got["done"].tolist() == [1, 1]
    assert np.array_equal(got["fin_path"][1], path[1])                                  # done on entry
    assert np.array_equal(got["fin_path"][0, :2], path[0, :2]) and np.array_equal(got["fin_path"][0, 2 + K:], path[0, 2 + K:])
    for slot in range(K):
        assert got["fin_path"][0, 2 + slot, step] == m[slot] // (2 * K)
    st2 = _state(rng, K, step, n_fin=[FIN_CAP, FIN_CAP - 1])
    got2, _ = _check_beam(model, st2, cv, ct, cl, path, **kw)
    assert got2["n_fin"].tolist() == [FIN_CAP, FIN_CAP]
    assert np.array_equal(got2["fin_path"][0], path[0])                                 # at FIN_CAP: nothing recorded
    assert np.array_equal(got2["fin_path"][1, :FIN_CAP - 1], path[1, :FIN_CAP - 1])


@pytest.mark.parametrize("K", [1, 3])
def test_beam_update_ragged_path(env, K):
    """ptab = [3, 5]: chunk 1's path starts at its own prompt's last position, and the step that uses up ITS budget (two
    steps before chunk 0's) finishes it"""
    model = env[1]
    rng = np.random.default_rng(400 + K)
    ptab, eot, budget = [3, 5], 90, 8            # the run reaches 11 positions: budgets 8 and 6
    cv, ct, cl = _cands(rng, K, eot)
    step = 5                                     # chunk 1's last step, not chunk 0's
    m0 = _merged(cv[:K])
    ct[:K].reshape(-1)[m0[0]] = eot
    st = _state(rng, K, step, ptab=ptab)
    path = np.full((B, FIN_CAP, NT + 1), PATH_SENT, np.uint8)
    got, _ = _check_beam(model, st, cv, ct, cl, path, ptab=ptab, K=K, V=400, step=step, budget=budget,
                         max_fin=FIN_CAP - K, eot=eot)
    assert got["n_fin"].tolist() == [1, K] and got["done"].tolist() == [0, 1]     # (chunk 0: slot 0 refilled, it goes on)
    m1 = _merged(cv[K:])
    for slot in range(K):
        src = K + m1[slot] // (2 * K)
        assert got["fin_path"][1, slot, :step].tolist() == st["kvidx2"][step & 1, src, 4:4 + step].tolist()
        assert got["fin_path"][1, slot, step] == src - K
    src0 = m0[0] // (2 * K)
    assert got["fin_path"][0, 0, :step].tolist() == st["kvidx2"][step & 1, src0, 2:2 + step].tolist()


# ----------------------------------------------------------------------------------------------------------- gather
def _gather(model, atok, alp, path, hyps, K, T, rc_only=False):
    from faster_whisper_amd import _lib as L
    steps, R, n = atok.shape
    h = np.ascontiguousarray(np.asarray(hyps, np.int32).reshape(-1, 4))
    cols = [np.ascontiguousarray(h[:, i]) for i in range(4)]
    out_t = np.full((len(hyps), T + 1, n), SENT_I, np.int32)
    out_l = np.full((len(hyps), T + 1, n), SENT_F, np.float32)
    atok, alp, path = np.ascontiguousarray(atok, np.int32), np.ascontiguousarray(alp, np.float32), np.ascontiguousarray(path, np.uint8)
    rc = model._lib.fw_test_alt_gather(model._replicas[0].handle, L.ptr(atok), L.ptr(alp), steps, R, K, NT, n, L.ptr(path),
                                       len(hyps), *[L.ptr(c) for c in cols], T, L.ptr(out_t), L.ptr(out_l))
    if rc_only:
        return rc, out_t, out_l
    L.check(rc)
    return out_t, out_l


@pytest.mark.parametrize("K,n", [(1, 1), (3, 3), (5, 8)])
def test_gather_walks_the_path(env, K, n):
    """a distinct value per (step, row, rank); paths that change rows at every step; hypotheses closed by <eot> (the end slot
    is the closing step's), cut at the budget ((-1, 0) in the end slot), empty, and entries past the length ((-1, 0))"""
    model = env[1]
    rng = np.random.default_rng(500 + K)
    Bc, steps, T = 3, 9, 9
    R = Bc * K
    flat = np.arange(steps * R * n, dtype=np.int32).reshape(steps, R, n)
    atok = flat * 3 + 1
    alp = -(flat.astype(np.float32) / np.float32(4.0)) - np.float32(0.25)
    path = np.full((Bc, FIN_CAP, NT + 1), PATH_SENT, np.uint8)
    hyps = [(0, 0, 4, 4), (0, 47, 9, -1), (1, 3, 0, 0), (2, 1, 8, 8), (2, 2, 1, -1), (1, 4, 6, 6)]
    for c, f, ln, end in hyps:
        for q in range(max(ln, end + 1)):
            path[c, f, q] = (q * 2 + c + f) % K       # another row at every step (K > 1)
    got_t, got_l = _gather(model, atok, alp, path, hyps, K, T)
    ref_t, ref_l = gather_ref(atok, alp, path, hyps, K, T)
    assert np.array_equal(got_t, ref_t) and _same_bits(got_l, ref_l)
    assert (got_t[1, T] == -1).all() and (got_l[1, T] == 0).all() and (got_t[1, :T] >= 0).all()     # cut at the budget
    assert (got_t[0, 4:T] == -1).all() and (got_l[0, 4:T] == 0).all()                                 # past the length
    assert np.array_equal(got_t[0, T], atok[4, 0 * K + path[0, 0, 4]])                                # the closing step
    assert (got_t[2, :T] == -1).all() and np.array_equal(got_t[2, T], atok[0, 1 * K + path[1, 3, 0]])  # <eot> at step 0


# ----------------------------------------------------------------------------------- each hook refuses a wrong test
def test_hooks_refuse_wrong_tests(env):
    from faster_whisper_amd import _lib as L
    cfg, model, _ = env
    rng = np.random.default_rng(9)
    logits = _logits(cfg, 2, rng)
    cum = np.zeros(2, np.float32)
    for kw in (dict(n_alt=9), dict(n_alt=-1)):
        rc, out = _launch(model, logits, [[11, 12]] * 2, cum, 1, False, rc_only=True, **kw)
        assert rc == L.FW_EINVAL
        assert (out["atok"] == SENT_I).all() and (out["alp"] == np.float32(SENT_F)).all() and (out["tok"] == SENT_I).all()
    for bad in (cfg.n_vocab, -1):                                  # a history id the sparse rules would index the row with
        rc, out = _launch(model, logits, [[11, bad]] * 2, cum, 1, False, n_alt=3, rc_only=True, repetition_penalty=1.3)
        assert rc == L.FW_EINVAL and (out["atok"] == SENT_I).all() and _same_bits(out["logits"], logits)
    # gather: n_alt 9, a path byte that is no beam of K, a closing step outside alt_*
    K, T, steps = 2, 4, 4
    path = np.zeros((1, FIN_CAP, NT + 1), np.uint8)
    ok = [(0, 0, 3, 3)]
    for n, p, hyps in ((9, path, ok), (2, np.where(np.arange(NT + 1) == 2, K, 0).astype(np.uint8) + path, ok),
                       (2, path, [(0, 0, 3, 4)]), (2, path, [(0, 0, 5, -1)]), (2, path, [(1, 0, 1, -1)]),
                       (2, path, [(0, FIN_CAP, 1, -1)])):
        atok = np.ones((steps, K, n), np.int32)
        rc, ot, ol = _gather(model, atok, atok.astype(np.float32), p, hyps, K, T, rc_only=True)
        assert rc == L.FW_EINVAL and (ot == SENT_I).all() and (ol == np.float32(SENT_F)).all(), (n, hyps)
    # beam update: a slot-table byte that is no beam, a ragged prompt beyond what the run reaches
    Kb, step, eot = 3, 2, 90
    cv, ct, cl = _cands(rng, Kb, eot)
    st = _state(rng, Kb, step)
    pathb = np.full((B, FIN_CAP, NT + 1), PATH_SENT, np.uint8)
    kw = dict(K=Kb, V=400, step=step, budget=9, max_fin=FIN_CAP - Kb, eot=eot, rc_only=True)
    st["kvidx2"][step & 1, 1, 1] = Kb
    rc, out = _beam_call(model, st, cv, ct, cl, pathb, **kw)
    assert rc == L.FW_EINVAL and (out["fin_path"] == PATH_SENT).all()
    st = _state(rng, Kb, step, ptab=[3, 12])
    rc, out = _beam_call(model, st, cv, ct, cl, pathb, ptab=[3, 12], **kw)       # 12 - 1 + 2 >= min(NT, 3 + 9)
    assert rc == L.FW_EINVAL and (out["fin_path"] == PATH_SENT).all()
