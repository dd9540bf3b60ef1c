"""The two decode-state kernels that record per-token log-probs, each in ONE launch through the hooks
fw_test_logits_rules_lp / fw_test_dec_beam_update_lp (include/fwamd_test.h):

  * dec_logits_process_kernel stores, beside cand_val = cum + raw and cand_tok, the `raw` it added: cand_val must be
    float32(cum + cand_lp) BIT FOR BIT for every valid candidate, and cand_lp the oracle's processed log-prob of cand_tok
    to the tolerance tests/test_gpu_logits_rules.py uses for the candidate values (2e-5: float32 round-off of the
    log-sum-exp).  Three chunks per launch (R = 3 K rows: the hook wants whole chunks; 3 rows for K = 1 and sampling), the
    vocabularies 1 913 (synthetic ids, the kernel's TXI = 0 instantiation) and 51 864 (TXI = 48), K = 1, 2, 5 and sampling;
  * dec_beam_update_kernel carries cand_lp through merge and walk into lphist2 (the log-prob history beside hist2) and
    fin_lp (finished hypotheses, end slot at [NT]).  These are copies: compared element for element, bit for bit, with
    tests/token_logprob_refs.py — both parity halves whole, so a store outside the contract shows as a changed sentinel.
    Everything the existing contract covers is compared with decode_state_refs.beam_update_ref as before."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_model
from decode_state_refs import FIN_CAP
from token_logprob_refs import beam_update_lp_ref, lp_state

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, -1234.5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ logits kernel
@pytest.fixture(scope="module", params=["micro", "tiny.en"])
def env(request):
    """only the vocabulary matters to this kernel: tiny.en's ids ride on a micro-sized network"""
    import dataclasses
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    from oracle.whisper import OracleWhisper
    full, micro = get_config(request.param), get_config("micro")
    keep = ("name", "n_mels", "d_model", "n_heads", "n_enc_layers", "n_dec_layers")
    cfg = dataclasses.replace(full, **{k: getattr(micro, k) for k in keep if hasattr(micro, k)})
    assert cfg.n_vocab == {"micro": 1913, "tiny.en": 51864}[request.param]
    w = synthetic_weights(cfg, seed=5)
    model = Whisper("synthetic:lp-rules", device="cuda", files={"config": cfg, "weights": w}, max_batch_size=3,
                    max_beam_size=5)
    return cfg, model, OracleWhisper(cfg, w)


def _logits(V, R, rng):
    """every row: V distinct multiples of 1/4096 in [0, 16), shuffled (tests/test_gpu_logits_rules.py)"""
    base = rng.permutation(65536)[:V].astype(np.float32) / np.float32(4096.0)
    return np.ascontiguousarray(np.stack([rng.permutation(base) for _ in range(R)]), dtype=np.float32)


def _launch(model, logits, hist, cum, K, with_ts, sampling=False, seed=0, suppress=()):
    from faster_whisper_amd import _lib
    R = logits.shape[0]
    n = len(hist[0]) if hist else 0
    o = _lib.FwGenOpts()
    o.beam_size, o.patience, o.num_hypotheses, o.length_penalty = K, 1.0, 1, 1.0
    o.repetition_penalty, o.no_repeat_ngram_size, o.max_length = 1.0, 0, 448
    o.max_initial_timestamp_index, o.suppress_blank = 50, 1
    sup = np.asarray(list(suppress), dtype=np.int32)
    o.suppress_tokens = _lib.as_i32p(sup) if sup.size else None
    o.n_suppress_tokens = int(sup.size)
    o.sampling_topk, o.sampling_temperature, o.seed, o.min_new_tokens = (0 if sampling else 1), 0.8, seed, 0
    Cn = 1 if sampling else 2 * K
    h = np.ascontiguousarray(np.asarray(hist, np.int32).reshape(R, n)) if n else np.zeros((R, 1), np.int32)
    cv, ct = np.zeros((R, Cn), np.float32), np.zeros((R, Cn), np.int32)
    cl = np.full((R, Cn), 7.0, np.float32)
    cum = np.ascontiguousarray(cum, np.float32)
    args = (model._replicas[0].handle, _lib.ptr(logits), R, _lib.ptr(h), n, _lib.ptr(cum), C.byref(o), int(with_ts),
            _lib.ptr(cv), _lib.ptr(ct))
    _lib.check(model._lib.fw_test_logits_rules_lp(*args, _lib.ptr(cl)))
    # the hook without the log-prob array (the kernel's null-pointer path) returns the same candidates
    cv0, ct0 = np.zeros_like(cv), np.zeros_like(ct)
    _lib.check(model._lib.fw_test_logits_rules(*args[:-2], _lib.ptr(cv0), _lib.ptr(ct0)))
    assert np.array_equal(_bits(cv0), _bits(cv)) and np.array_equal(ct0, ct)
    return cv, ct, cl


def _oracle_lp(oracle, logits, hist, with_ts, suppress):
    V = logits.shape[1]
    mask = None
    if len(suppress):
        mask = np.zeros(V, dtype=bool)
        mask[list(suppress)] = True
    return np.stack([oracle._process_logits(logits[r], list(hist[r]) if hist else [], with_ts, mask, True, 50, 1.0, 0, 0)
                     for r in range(logits.shape[0])])


def _check_logits(env, K, hist, with_ts, seed, sampling=False, suppress=(), cum_scale=3.0):
    cfg, model, oracle = env
    rng = np.random.default_rng(seed)
    R = 3 * K
    logits = _logits(cfg.n_vocab, R, rng)
    if with_ts:
        logits[:, cfg.timestamp_begin:] -= 8.0      # the timestamp mass well below the best text token (rule (e) off)
    cum = -rng.random(R).astype(np.float32) * np.float32(cum_scale)
    hist = [list(hist)] * R if hist is not None else None
    cv, ct, cl = _launch(model, logits, hist, cum, K, with_ts, sampling, seed=seed + 1000, suppress=suppress)
    valid = np.isfinite(cv)
    assert valid.any() and np.array_equal(np.isfinite(cl), valid)
    assert np.isneginf(cl[~valid]).all()                       # nothing left on the row: -inf, like cand_val
    # the stored value IS what was added to cum
    want = (cum[:, None] + cl).astype(np.float32)
    assert np.array_equal(_bits(cv)[valid], _bits(want)[valid]), np.argwhere(_bits(cv) != _bits(want))[:8]
    ref = _oracle_lp(oracle, logits, hist, with_ts, suppress)
    rlp = np.take_along_axis(ref, ct.astype(np.int64), axis=1)
    err = float(np.abs(cl[valid] - rlp[valid]).max())
    print(f"[V={cfg.n_vocab}] K={K} sampling={sampling} ts={with_ts}: {int(valid.sum())} candidates, "
          f"max |cand_lp - oracle| {err:.2e}")
    assert err < 2e-5
    return cv, ct, cl


@pytest.mark.parametrize("K", [1, 2, 5])
def test_logits_kernel_stores_the_logprob_it_added(env, K):
    cfg = env[0]
    tb = cfg.timestamp_begin
    sup = sorted({cfg.sot, cfg.sot_prev, cfg.no_speech, 1, 2, 63, 64, 1023, 1024, cfg.n_vocab - 1})
    _check_logits(env, K, None, False, 1 + K)
    _check_logits(env, K, [11, 12, 13], False, 11 + K, suppress=sup)
    _check_logits(env, K, [tb + 3, 40], True, 21 + K, suppress=sup)
    # |raw| > |cum|: where a difference of the two running sums would not give raw back
    _check_logits(env, K, [11, 12], False, 31 + K, cum_scale=2.0 ** -10)


def test_logits_kernel_sampling(env):
    cfg = env[0]
    cv, ct, cl = _check_logits(env, 1, [11, 12, 13], False, 40, sampling=True)
    assert cv.shape == (3, 1)
    cv, ct, cl = _check_logits(env, 1, None, True, 41, sampling=True)
    assert (ct >= cfg.timestamp_begin).all()


def test_logits_kernel_nothing_left(env):
    """a closed timestamp pair and every text id suppressed: no candidate, cand_lp = -inf everywhere (sampling: the drawn
    slot)"""
    cfg, model, _ = env
    tb = cfg.timestamp_begin
    logits = _logits(cfg.n_vocab, 3, np.random.default_rng(3))
    for sampling in (False, True):
        cv, ct, cl = _launch(model, logits, [[tb + 1, tb + 1]] * 3, np.zeros(3, np.float32), 1, True, sampling,
                             suppress=range(tb))
        assert np.isneginf(cv).all() and np.isneginf(cl).all() and (ct == 0).all()


# ------------------------------------------------------------------------------------------------ beam update
@pytest.fixture(scope="module")
def model():
    _, _, m = make_model("micro", max_batch=2, max_beam=2)
    return m


B, NT, P = 2, 16, 3
STATE_KEYS = ("hist2", "kvidx2", "cur_tok", "done", "n_done", "n_fin", "fin_tok", "fin_len")


def _beam_call(model, st, cv, ct, cl, *, K, V, step, budget, max_fin, eot):
    from faster_whisper_amd import _lib as L
    R, cur, pos = B * K, step & 1, P - 1 + step
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
    L.check(model._lib.fw_test_dec_beam_update_lp(
        model._replicas[0].handle, B, K, NT, V, P, step, budget, max_fin, 0.0, eot, L.ptr(cv), L.ptr(ct), L.ptr(cl),
        L.ptr(hist), L.ptr(lphist), L.ptr(kvidx), L.ptr(cum), SENT_I, SENT_F, L.ptr(out["done"]), L.ptr(out["n_done"]),
        L.ptr(out["n_fin"]), L.ptr(out["fin_tok"]), L.ptr(out["fin_len"]), L.ptr(out["fin_score"]), L.ptr(out["fin_cum"]),
        L.ptr(out["fin_lp"]), L.ptr(out["hist2"]), L.ptr(out["lphist2"]), L.ptr(out["kvidx2"]), L.ptr(out["cum2"]),
        L.ptr(out["cur_tok"])))
    return out


def _check_beam(model, st, cv, ct, cl, **kw):
    got = _beam_call(model, st, cv, ct, cl, **kw)
    ref = beam_update_lp_ref(st, cv, ct, cl, P=P, lp_pow=0.0, **{k: v for k, v in kw.items() if k != "V"})
    for k in STATE_KEYS:
        assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:8])
    for k in ("cum2", "fin_cum", "lphist2", "fin_lp"):       # copies of inputs: bit for bit, sentinels included
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (k, np.argwhere(_bits(got[k]) != _bits(ref[k]))[:8])
    assert np.array_equal(got["fin_score"].astype(np.float64), ref["fin_score"])     # (lp_pow = 0: the cum itself)
    return got, ref


def _cands(rng, K, eot):
    """[B K][2K] candidates: distinct values (multiples of 1/64, rows sorted descending), tokens = 100 + flat index inside
    the chunk, log-probs = distinct recognisable negatives unrelated to the values (they are only carried)"""
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


def _state(rng, K, step, **kw):
    R = B * K
    hist = rng.integers(0, 90, (R, step)).astype(np.int32)
    lphist = -rng.random((R, step)).astype(np.float32) * 9
    kvidx = rng.integers(0, K, (R, P - 1 + step)).astype(np.uint8)
    cum = -rng.random(R).astype(np.float32) * 5
    return lp_state(B, K, NT, step, P, hist, lphist, kvidx, cum, SENT_I, SENT_F, **kw)


@pytest.mark.parametrize("K", [2, 5])
def test_beam_step0_only_row0_is_a_source(model, K):
    rng = np.random.default_rng(50 + K)
    eot = 90
    cv, ct, cl = _cands(rng, K, eot)
    for r in range(B * K):
        if r % K:
            cv[r] += np.float32(100.0)      # poison rows: would win every slot if they were sources
    ct[K, 0] = eot                          # chunk 1: <eot> is the best candidate at step 0 -> an empty hypothesis
    st = _state(rng, K, 0)
    got, ref = _check_beam(model, st, cv, ct, cl, K=K, V=400, step=0, budget=9, max_fin=FIN_CAP - K, eot=eot)
    # every live row's first log-prob is one of row 0's candidates, in merge order
    assert np.array_equal(got["lphist2"][1, :K, 0], cl[0, :K])
    assert got["n_fin"].tolist() == [0, 1] and got["fin_len"][1, 0] == 0
    assert got["fin_lp"][1, 0, NT] == cl[K, 0] and (got["fin_lp"][1, 0, :NT] == np.float32(SENT_F)).all()
    assert np.array_equal(got["lphist2"][1, K:, 0], np.concatenate([cl[K, K:K + 1], cl[K, 1:K]]))   # slot 0 refilled


@pytest.mark.parametrize("K", [2, 5])
def test_beam_middle_step_eot_slot_refilled(model, K):
    """slot 0 is <eot> (a finished hypothesis with an end value), the first secondary is <eot> too (skipped, not
    recorded), the next secondary refills slot 0"""
    rng = np.random.default_rng(60 + K)
    step, eot = 5, 90
    cv, ct, cl = _cands(rng, K, eot)
    m = _merged(cv[:K])
    ct[:K].reshape(-1)[[m[0], m[K]]] = eot
    st = _state(rng, K, step)
    got, ref = _check_beam(model, st, cv, ct, cl, K=K, V=400, step=step, budget=12, max_fin=FIN_CAP - K, eot=eot)
    Cn = 2 * K
    nxt = (step & 1) ^ 1
    assert got["n_fin"].tolist() == [1, 0] and got["done"].tolist() == [0, 0]
    par = m[0] // Cn
    assert np.array_equal(got["fin_lp"][0, 0, :step], st["lphist2"][step & 1, par, :step])
    assert got["fin_lp"][0, 0, NT] == cl[:K].reshape(-1)[m[0]]
    assert (got["fin_lp"][0, 0, step:NT] == np.float32(SENT_F)).all()        # <eot> is no token of the hypothesis
    assert got["lphist2"][nxt, 0, step] == cl[:K].reshape(-1)[m[K + 1]]       # the refill is the SECOND secondary
    assert np.array_equal(got["lphist2"][nxt, 0, :step], st["lphist2"][step & 1, m[K + 1] // Cn, :step])
    for k in range(1, K):
        assert got["lphist2"][nxt, k, step] == cl[:K].reshape(-1)[m[k]]
    assert np.array_equal(got["lphist2"][step & 1], st["lphist2"][step & 1])  # the current half is left as it was


@pytest.mark.parametrize("K", [2, 5])
def test_beam_last_step_done_on_entry_and_fin_cap(model, K):
    """the last step: every slot finishes, a real token's log-prob is the hypothesis' last value and the end value is 0,
    an <eot>'s goes to the end slot; chunk 1 in the first launch is done on entry (nothing is written); in the second
    launch it holds FIN_CAP hypotheses already (nothing is recorded)"""
    rng = np.random.default_rng(70 + K)
    step, eot = 6, 90
    cv, ct, cl = _cands(rng, K, eot)
    m = _merged(cv[:K])
    ct[:K].reshape(-1)[m[1]] = eot
    fin_lp = -rng.random((B, FIN_CAP, NT + 1)).astype(np.float32) - 50
    st = _state(rng, K, step, done=[0, 1], n_done=1, n_fin=[2, 3], fin_lp=fin_lp)
    kw = dict(K=K, V=400, step=step, budget=step + 1, max_fin=FIN_CAP - K, eot=eot)
    got, ref = _check_beam(model, st, cv, ct, cl, **kw)
    assert got["done"].tolist() == [1, 1] and got["n_fin"].tolist() == [2 + K, 3]
    for slot in range(K):
        f = cl[:K].reshape(-1)[m[slot]]
        row = got["fin_lp"][0, 2 + slot]
        assert np.array_equal(row[:step], st["lphist2"][step & 1, m[slot] // (2 * K), :step])
        if slot == 1:
            assert row[NT] == f and row[step] == fin_lp[0, 2 + slot, step]
        else:
            assert row[step] == f and row[NT] == 0.0
    assert np.array_equal(_bits(got["fin_lp"][1]), _bits(fin_lp[1]))                    # done on entry
    assert (got["lphist2"][(step & 1) ^ 1] == np.float32(SENT_F)).all()                 # no row state is rewritten
    st2 = _state(rng, K, step, n_fin=[FIN_CAP, FIN_CAP - 1], fin_lp=fin_lp)
    got2, _ = _check_beam(model, st2, cv, ct, cl, **kw)
    assert got2["n_fin"].tolist() == [FIN_CAP, FIN_CAP]
    assert np.array_equal(_bits(got2["fin_lp"][0]), _bits(fin_lp[0]))                   # at FIN_CAP: nothing recorded
    assert np.array_equal(_bits(got2["fin_lp"][1, :FIN_CAP - 1]), _bits(fin_lp[1, :FIN_CAP - 1]))


@pytest.mark.parametrize("K", [2, 5])
def test_beam_dead_beams_copy_live_beam_0(model, K):
    """K - 1 finite candidates: the last beam is dead (cum = -inf) and carries live beam 0's history and log-probs"""
    rng = np.random.default_rng(80 + K)
    step, eot = 3, 90
    cv, ct, cl = _cands(rng, K, eot)
    keep = _merged(cv[:K])[:K - 1]
    cut = np.full(K * 2 * K, -np.inf, np.float32)
    cut[keep] = cv[:K].reshape(-1)[keep]
    cv[:K] = cut.reshape(K, 2 * K)
    st = _state(rng, K, step)
    got, ref = _check_beam(model, st, cv, ct, cl, K=K, V=400, step=step, budget=12, max_fin=FIN_CAP - K, eot=eot)
    nxt = (step & 1) ^ 1
    assert got["cum2"][nxt, K - 1] == -np.inf and np.isfinite(got["cum2"][nxt, :K - 1]).all()
    assert np.array_equal(got["lphist2"][nxt, K - 1, :step + 1], got["lphist2"][nxt, 0, :step + 1])
    assert np.array_equal(got["hist2"][nxt, K - 1, :step + 1], got["hist2"][nxt, 0, :step + 1])
