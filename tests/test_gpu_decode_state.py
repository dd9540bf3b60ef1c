"""The kernels that carry a decode run's state from one step to the next, each in isolation against the plain references
of tests/decode_state_refs.py, through the hooks fw_test_dec_beam_update / fw_test_dec_embed / fw_test_align_post
(include/fwamd_test.h):

  * dec_beam_update_kernel (dec_kernels.hip K19/K20): merge, EOS walk, finished hypotheses, the rewrite of history,
    slot table, cum and next token into the other parity half, done / n_done.  Compared EXACTLY (integers and fp32
    bits, both parity halves whole, so a write outside the contract shows as a changed sentinel) except fin_score under
    a length penalty, which goes through the device powf and one division;
  * dec_embed_kernel (K12): bit-exact, row-major and fragment-major, in its three position modes;
  * align_stats_kernel + align_filter_kernel (decoder.hip): against fp64, with a tolerance taken from an fp32
    restatement in the kernels' operation order evaluated on the same input.

The hooks check every index and extent before they launch: the tests that pass bad arguments assert FW_EINVAL only."""
import numpy as np
import pytest

from conftest import make_model
from decode_state_refs import (FIN_CAP, align_post_fp32, align_post_ref, beam_state, beam_update_ref, embed_positions,
                               embed_ref, finished_list, run_chain, toy_table)

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, -1234.5
FW_EINVAL = -1        # include/fwamd.h

# fin_score under a length penalty: the largest relative deviation of the kernel from the fp64 reference over the lengths
# 1 .. 447 of test_fin_score_length_penalty, measured on an MI355X (ROCm 7.x): 1.489e-7 for lp_pow = 1.0, 2.517e-7 for
# lp_pow = 0.6.  (lp_pow = 1.0 is more than the half ulp, 6e-8, of one correctly rounded division: the device
# powf(len, 1) is itself an ulp off for some lengths.)  The bound is 4 x the measured value: the device powf and the
# division differ between library versions by a few ulp.
FIN_SCORE_MEASURED = {1.0: 1.489e-7, 0.6: 2.517e-7}
FIN_SCORE_RTOL = {p: 4 * v for p, v in FIN_SCORE_MEASURED.items()}


@pytest.fixture(scope="module")
def model():
    _, _, m = make_model("micro", max_batch=2, max_beam=2)
    return m


def _L():
    from faster_whisper_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ beam update
def _beam_call(model, st, cv, ct, *, K, V, P, step, budget, max_fin, lp_pow, eot):
    """one hook call on a state in beam_state's layout: returns (rc, the state the launch left)"""
    L = _L()
    _, R, NT = st["hist2"].shape
    B, cur, pos = R // K if K > 0 else 1, step & 1, P - 1 + step
    hist = np.ascontiguousarray(st["hist2"][cur, :, :max(step, 0)], np.int32)
    kvidx = np.ascontiguousarray(st["kvidx2"][cur, :, :max(pos, 0)], np.uint8)
    cum = np.ascontiguousarray(st["cum2"][cur], np.float32)
    cv = np.ascontiguousarray(cv, np.float32)
    ct = np.ascontiguousarray(ct, np.int32)
    out = {k: np.ascontiguousarray(st[k]).copy() for k in ("done", "n_done", "n_fin", "fin_tok", "fin_len", "fin_score",
                                                            "fin_cum")}
    out["hist2"] = np.zeros((2, R, NT), np.int32)
    out["kvidx2"] = np.zeros((2, R, NT), np.uint8)
    out["cum2"] = np.zeros((2, R), np.float32)
    out["cur_tok"] = np.zeros(R, np.int32)
    rc = model._lib.fw_test_dec_beam_update(
        model._replicas[0].handle, B, K, NT, V, P, step, budget, max_fin, float(lp_pow), eot, L.ptr(cv), L.ptr(ct),
        L.ptr(hist), L.ptr(kvidx), L.ptr(cum), SENT_I, SENT_F, L.ptr(out["done"]), L.ptr(out["n_done"]),
        L.ptr(out["n_fin"]), L.ptr(out["fin_tok"]), L.ptr(out["fin_len"]), L.ptr(out["fin_score"]), L.ptr(out["fin_cum"]),
        L.ptr(out["hist2"]), L.ptr(out["kvidx2"]), L.ptr(out["cum2"]), L.ptr(out["cur_tok"]))
    return rc, out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _beam_check(model, st, cv, ct, **kw):
    """launch and compare the WHOLE returned state with the reference; returns (kernel state, reference state, largest
    relative deviation of a newly recorded fin_score)"""
    rc, got = _beam_call(model, st, cv, ct, **kw)
    _L().check(rc)
    ref = beam_update_ref(st, cv, ct, **{k: v for k, v in kw.items() if k != "V"})
    for k in ("hist2", "kvidx2", "cur_tok", "done", "n_done", "n_fin", "fin_tok", "fin_len"):
        assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:8])
    for k in ("cum2", "fin_cum"):          # copies of inputs: bit for bit (-inf and the sentinel included)
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (k, np.argwhere(_bits(got[k]) != _bits(ref[k]))[:8])
    new = ref["fin_score"] != st["fin_score"].astype(np.float64)
    assert np.array_equal(_bits(got["fin_score"])[~new], _bits(st["fin_score"])[~new])
    dev = 0.0
    if new.any():
        g, r = got["fin_score"][new].astype(np.float64), ref["fin_score"][new]
        if kw["lp_pow"] == 0:
            assert np.array_equal(g, r)
        else:
            dev = float((np.abs(g - r) / np.abs(r)).max())
            assert dev <= FIN_SCORE_RTOL[kw["lp_pow"]], dev
    return got, ref, dev


def _rows(rng, K, lo=-40.0):
    """[K][2K] distinct multiples of 1/64 in [lo, 0), every row sorted descending"""
    C = 2 * K
    v = rng.permutation(int(-lo * 64))[:K * C].astype(np.float32).reshape(K, C) / np.float32(-64.0) - np.float32(1 / 64)
    return -np.sort(-v, axis=1)


def _merged(v):
    """flat indices of a chunk's finite candidates in merge order (value descending, flat index ascending)"""
    f = v.reshape(-1)
    return [int(i) for i in np.argsort(-f, kind="stable") if f[i] != -np.inf]


def _keep_finite(v, n):
    """only the first n candidates of the merge order stay finite (rows stay sorted: what is cut is a tail of each)"""
    out = np.full_like(v, -np.inf)
    idx = _merged(v)[:n]
    out.reshape(-1)[idx] = v.reshape(-1)[idx]
    return out


SCENARIOS = ("plain", "ties", "eos_slot0", "eos_many", "sec_exhausted", "all_inf", "few_finite")


def _scenario(name, rng, K, eot):
    """one chunk's candidates [K][2K]: tokens are the flat candidate index (every candidate is identifiable), <eot>
    where the scenario wants a hypothesis to finish"""
    C = 2 * K
    v = _rows(rng, K)
    t = np.arange(K * C, dtype=np.int32).reshape(K, C)
    if name == "ties":      # four distinct values only: ties across rows and inside rows
        v = -np.sort(-(rng.integers(1, 5, (K, C)).astype(np.float32) * np.float32(-0.5)), axis=1)
    elif name == "eos_slot0":
        t.reshape(-1)[_merged(v)[0]] = eot
    elif name == "eos_many":                      # primaries 0, 2 and the last one; the first two secondaries
        m = _merged(v)
        for s in {0, min(2, K - 1), K - 1, K, min(K + 1, len(m) - 1)}:
            t.reshape(-1)[m[s]] = eot
    elif name == "sec_exhausted":                 # K + 1 finite, two <eot> primaries, one secondary: K - 1 live beams
        v = _keep_finite(v, K + 1)
        m = _merged(v)
        for s in (0, min(1, K - 1)):
            t.reshape(-1)[m[s]] = eot
    elif name == "all_inf":
        v[:] = -np.inf
    elif name == "few_finite":
        v = _keep_finite(v, max(K - 1, 1))
    t[v == -np.inf] = 0
    return v, t


def _random_fin(rng, B, NT):
    """finished-hypothesis arrays `as they stand`: arbitrary recognisable content"""
    return (rng.integers(1000, 2000, (B, FIN_CAP, NT)).astype(np.int32), rng.integers(1, 9, (B, FIN_CAP)).astype(np.int32),
            -rng.random((B, FIN_CAP)).astype(np.float32), -rng.random((B, FIN_CAP)).astype(np.float32) * 9)


def _state(rng, B, K, NT, P, step, **kw):
    R = B * K
    hist = rng.integers(0, 500, (R, step)).astype(np.int32)
    kvidx = rng.integers(0, K, (R, P - 1 + step)).astype(np.uint8)
    cum = -rng.random(R).astype(np.float32) * 5
    kw.setdefault("fin", _random_fin(rng, B, NT))
    return beam_state(B, K, NT, step, P, hist, kvidx, cum, SENT_I, SENT_F, **kw)


@pytest.mark.parametrize("K", [5, 1, 2, 16])
def test_beam_hand_built_scenarios(model, K):
    """the seven candidate scenarios as the chunks of ONE launch (chunk isolation), then the same launch with chunks
    done on entry, whose every byte must stay"""
    rng = np.random.default_rng(100 + K)
    B, NT, P, step, eot = 7, 24, 3, 4, 2 * K * K + 3
    V = eot + 1
    cands = [_scenario(s, rng, K, eot) for s in SCENARIOS]
    cv, ct = np.concatenate([c[0] for c in cands]), np.concatenate([c[1] for c in cands])
    kw = dict(K=K, V=V, P=P, step=step, budget=20, max_fin=FIN_CAP - K, lp_pow=0.0, eot=eot)
    st = _state(rng, B, K, NT, P, step, n_fin=[0, 1, 2, 3, 0, 5, 1], n_done=0)
    got, ref, _ = _beam_check(model, st, cv, ct, **kw)
    # the scenarios reach the branches they are named after (asserted on the reference: the kernel equals it)
    sc = {s: i for i, s in enumerate(SCENARIOS)}
    nxt = (step & 1) ^ 1
    assert ref["done"][sc["all_inf"]] == 1 and ref["n_fin"][sc["all_inf"]] == 5
    assert ref["n_fin"][sc["eos_slot0"]] == 2 + 1
    assert ref["n_fin"][sc["eos_many"]] == 3 + len({0, min(2, K - 1), K - 1})
    assert ref["done"][sc["plain"]] == 0 and ref["n_fin"][sc["plain"]] == 0
    if K >= 2:
        for s in ("sec_exhausted", "few_finite"):
            c = sc[s]
            assert ref["done"][c] == 0 and ref["cum2"][nxt, c * K + K - 1] == -np.inf
            assert np.isfinite(ref["cum2"][nxt, c * K:c * K + K - 1]).all()
    assert ref["n_done"][0] == int(ref["done"].sum())
    # chunks 0, 3 and 6 done on entry
    st2 = _state(rng, B, K, NT, P, step, n_fin=[4, 1, 2, 3, 0, 5, 1], done=[1, 0, 0, 1, 0, 0, 1], n_done=3)
    got2, ref2, _ = _beam_check(model, st2, cv, ct, **kw)
    for c in (0, 3, 6):
        rows = slice(c * K, (c + 1) * K)
        for k in ("hist2", "kvidx2", "cum2"):
            assert np.array_equal(got2[k][:, rows], st2[k][:, rows])
        for k in ("fin_tok", "fin_len", "n_fin", "done"):
            assert np.array_equal(got2[k][c], st2[k][c])
        assert (got2["cur_tok"][rows] == SENT_I).all()


def test_beam_step0_only_row0_is_a_source(model):
    """step 0: rows 1 .. K - 1 hold LARGER poison candidates that must be ignored; an <eot> at step 0 is a hypothesis of
    length 0, scored with denominator 1"""
    rng = np.random.default_rng(7)
    B, K, NT, P, eot = 3, 5, 16, 3, 90
    cv = np.concatenate([_rows(rng, K) for _ in range(B)])
    ct = np.tile(np.arange(2 * K, dtype=np.int32), (B * K, 1)) + 10 * (np.arange(B * K, dtype=np.int32) % K)[:, None]
    for r in range(B * K):
        if r % K:
            cv[r] += np.float32(100.0)       # poison: would win every slot if it were a source
    ct[1 * K, 0] = eot                       # chunk 1: <eot> is the best candidate of row 0
    ct[2 * K, [1, 3]] = eot                  # chunk 2: two <eot> primaries
    st = _state(rng, B, K, NT, P, 0)
    got, ref, _ = _beam_check(model, st, cv, ct, K=K, V=eot + 1, P=P, step=0, budget=9, max_fin=FIN_CAP - K, lp_pow=1.0,
                              eot=eot)
    assert (got["kvidx2"][1, :, P - 1] == 0).all() and (got["cur_tok"] < 10).all()      # every parent is row 0
    assert got["fin_len"][1, 0] == 0 and got["fin_score"][1, 0] == got["fin_cum"][1, 0] == cv[K, 0]
    assert got["n_fin"].tolist() == [0, 1, 2]


def test_beam_last_step(model):
    """step + 1 == budget: all K primaries finish, a non-<eot> token is appended (len == step + 1), done is set, n_done
    rises from a non-zero start by the number of chunks that finished, the other half stays all sentinel"""
    rng = np.random.default_rng(8)
    B, K, NT, P, step, eot = 3, 5, 16, 2, 6, 60
    cv = np.concatenate([_rows(rng, K) for _ in range(B)])
    ct = rng.integers(0, eot, (B * K, 2 * K)).astype(np.int32)
    m0 = _merged(cv[:K])
    ct[:K].reshape(-1)[[m0[1], m0[3]]] = eot
    st = _state(rng, B, K, NT, P, step, done=[0, 1, 0], n_done=4, n_fin=[0, 2, 3], fin=None)
    got, ref, _ = _beam_check(model, st, cv, ct, K=K, V=eot + 1, P=P, step=step, budget=step + 1, max_fin=FIN_CAP - K,
                              lp_pow=0.0, eot=eot)
    assert got["done"].tolist() == [1, 1, 1] and got["n_done"][0] == 4 + 2
    assert got["n_fin"].tolist() == [K, 2, 3 + K]
    assert sorted(got["fin_len"][0, :K].tolist()) == [step] * 2 + [step + 1] * 3
    assert (got["fin_len"][2, 3:3 + K] == step + 1).all()
    nxt = (step & 1) ^ 1
    assert (got["hist2"][nxt] == SENT_I).all() and (got["kvidx2"][nxt] == SENT_I & 0xFF).all()
    assert (got["cum2"][nxt] == np.float32(SENT_F)).all() and (got["cur_tok"] == SENT_I).all()


def test_beam_max_fin_per_chunk(model):
    """max_fin reached on some chunks of a launch and not on others"""
    rng = np.random.default_rng(9)
    B, K, NT, P, step, eot = 4, 5, 16, 2, 3, 60
    cv = np.concatenate([_rows(rng, K) for _ in range(B)])
    ct = rng.integers(0, eot, (B * K, 2 * K)).astype(np.int32)
    for c in range(B):                                       # one <eot> primary per chunk, two on chunk 3
        m = _merged(cv[c * K:(c + 1) * K])
        ct[c * K:(c + 1) * K].reshape(-1)[m[:2] if c == 3 else m[2:3]] = eot
    st = _state(rng, B, K, NT, P, step, n_fin=[0, 2, 1, 1])
    got, ref, _ = _beam_check(model, st, cv, ct, K=K, V=eot + 1, P=P, step=step, budget=20, max_fin=3, lp_pow=0.0, eot=eot)
    assert got["n_fin"].tolist() == [1, 3, 2, 3] and got["done"].tolist() == [0, 1, 0, 1] and got["n_done"][0] == 2


def test_beam_fin_cap_guard(model):
    """n_fin_in = FIN_CAP - 1 and two <eot> primaries: one hypothesis is recorded, n_fin == FIN_CAP, and the
    neighbouring chunk's fin_* entries (the next addresses) are untouched"""
    rng = np.random.default_rng(10)
    B, K, NT, P, step, eot = 2, 5, 16, 2, 3, 60
    cv = np.concatenate([_rows(rng, K) for _ in range(B)])
    ct = rng.integers(0, eot, (B * K, 2 * K)).astype(np.int32)
    m = _merged(cv[:K])
    ct[:K].reshape(-1)[[m[0], m[2]]] = eot
    st = _state(rng, B, K, NT, P, step, n_fin=[FIN_CAP - 1, 0])
    got, ref, _ = _beam_check(model, st, cv, ct, K=K, V=eot + 1, P=P, step=step, budget=20, max_fin=FIN_CAP + 5, lp_pow=0.0,
                              eot=eot)
    assert got["n_fin"].tolist() == [FIN_CAP, 0] and got["done"].tolist() == [0, 0]
    assert got["fin_cum"][0, FIN_CAP - 1] == cv[:K].reshape(-1)[m[0]]
    for k in ("fin_tok", "fin_len", "fin_score", "fin_cum"):
        assert np.array_equal(got[k][1], st[k][1])
        assert np.array_equal(got[k][0, :FIN_CAP - 1], st[k][0, :FIN_CAP - 1])


@pytest.mark.parametrize("P,step", [(4, 70), (4, 444)])
def test_beam_long_copies(model, P, step):
    """history and slot table longer than the 64-thread copy stride and no multiple of it; (4, 444): the parent byte lands
    on the last position NT - 1.  Chunk 0: the parents are a permutation of the rows; chunk 1: every row has ONE parent.
    Rows hold distinct random histories and slot bytes, so a copy from the wrong row or the wrong half shows."""
    rng = np.random.default_rng(step)
    B, K, NT, eot = 2, 5, 448, 600
    assert P - 1 + step < NT and (step % 64) and ((P - 1 + step) % 64)
    cv = np.full((B * K, 2 * K), -np.inf, np.float32)
    ct = rng.integers(0, eot, (B * K, 2 * K)).astype(np.int32)
    perm = [3, 0, 4, 1, 2]
    for slot, row in enumerate(perm):                    # row perm[s] owns merged slot s; its other candidates lose
        cv[row] = np.float32(-1.0 - slot) - np.arange(2 * K, dtype=np.float32) * 50
    cv[K + 2] = -np.arange(2 * K, dtype=np.float32) - 1  # chunk 1: row 2 holds the K best
    cv[[K, K + 1, K + 3, K + 4]] = (np.float32(-100.0) - np.arange(2 * K, dtype=np.float32))[None]
    st = _state(rng, B, K, NT, P, step)
    got, ref, _ = _beam_check(model, st, cv, ct, K=K, V=eot + 1, P=P, step=step, budget=NT, max_fin=FIN_CAP - K, lp_pow=0.0,
                              eot=eot)
    nxt, pos = (step & 1) ^ 1, P - 1 + step
    assert got["kvidx2"][nxt, :K, pos].tolist() == perm and got["kvidx2"][nxt, K:, pos].tolist() == [2] * K
    assert np.array_equal(got["hist2"][nxt, :K, :step], st["hist2"][step & 1, perm, :step])
    assert np.array_equal(got["kvidx2"][nxt, K:, :pos], np.repeat(st["kvidx2"][step & 1, K + 2:K + 3, :pos], K, 0))


@pytest.mark.parametrize("max_fin", [5, FIN_CAP - 5])
def test_beam_driven_chain(model, max_fin):
    """beam search over a toy language model (V = 12, K = 5, 3 chunks with different tables, budget 14): every step's
    output state is the next launch's input, compared with the reference after every step through both parity
    halves; the final finished lists equal those of the reference chained on its own"""
    V, K, B, budget, eot, P, NT, lp_pow = 12, 5, 3, 14, 11, 3, 32, 0.6
    logp = toy_table(22, V, n=B)
    logp[:, :, eot] += np.float32(1.0)          # (a likelier <eot>: the chunks finish at different steps at max_fin = 5,
    #                                              and one of them reaches max_fin = 43 before the budget)
    kw = dict(K=K, V=V, P=P, budget=budget, max_fin=max_fin, lp_pow=lp_pow, eot=eot)
    steps = []

    def gpu_step(st, cv, ct, step):
        got, ref, _ = _beam_check(model, st, cv, ct, step=step, **kw)
        steps.append(step)
        return got

    final = run_chain(logp, B, K, NT, P, budget, max_fin, lp_pow, eot, SENT_I, SENT_F, step_fn=gpu_step)
    ref = run_chain(logp, B, K, NT, P, budget, max_fin, lp_pow, eot, SENT_I, SENT_F)
    assert len(steps) >= 4 and final["done"].all() and final["n_done"][0] == B
    for c in range(B):
        g, r = finished_list(final, c), finished_list(ref, c)
        assert [h[:2] for h in g] == [h[:2] for h in r] and len(g) >= 1
        np.testing.assert_allclose([h[2] for h in g], [h[2] for h in r], rtol=FIN_SCORE_RTOL[lp_pow])
    print(f"chain max_fin={max_fin}: {len(steps)} steps, finished per chunk {final['n_fin'].tolist()}")


@pytest.mark.parametrize("lp_pow", [1.0, 0.6])
def test_fin_score_length_penalty(model, lp_pow):
    """score = cum / len ** lp_pow for every length 1 .. 447 against fp64 (an <eot> at step L finishes a hypothesis of
    length L).  Prints the largest relative deviation; the bound is FIN_SCORE_RTOL[lp_pow] (see its comment)."""
    rng = np.random.default_rng(int(lp_pow * 10))
    B, K, NT, P, eot = 2, 1, 448, 1, 5
    worst = 0.0
    for Ln in range(1, NT):
        cv = np.stack([-rng.random(2), np.full(2, -np.inf)], axis=1).astype(np.float32) * np.float32(Ln)
        ct = np.array([[eot, 0], [eot, 0]], np.int32)
        st = beam_state(B, K, NT, Ln, P, rng.integers(0, 5, (B, Ln)), np.zeros((B, Ln), np.uint8), np.zeros(B, np.float32),
                        SENT_I, SENT_F)
        got, ref, dev = _beam_check(model, st, cv, ct, K=K, V=eot + 1, P=P, step=Ln, budget=NT, max_fin=FIN_CAP - K,
                                    lp_pow=lp_pow, eot=eot)
        assert got["fin_len"][:, 0].tolist() == [Ln, Ln]
        worst = max(worst, dev)
    print(f"fin_score lp_pow={lp_pow}: largest relative deviation from fp64 over lengths 1..447 = {worst:.3e} "
          f"(bound {FIN_SCORE_RTOL[lp_pow]:.3e})")
    assert 0 < worst <= FIN_SCORE_RTOL[lp_pow]


def test_beam_bad_arguments_are_refused(model):
    """every index or extent the kernel would use is checked before anything is launched: FW_EINVAL, nothing else"""
    rng = np.random.default_rng(1)
    B, K, NT, P, step, eot = 2, 3, 16, 3, 4, 40
    good = dict(K=K, V=eot + 1, P=P, step=step, budget=9, max_fin=4, lp_pow=0.0, eot=eot)
    cv = np.concatenate([_rows(rng, K) for _ in range(B)])
    ct = rng.integers(0, eot, (B * K, 2 * K)).astype(np.int32)
    st = _state(rng, B, K, NT, P, step)
    assert _beam_call(model, st, cv, ct, **good)[0] == 0
    for bad in (dict(K=0), dict(K=17), dict(P=0), dict(step=-1), dict(step=NT), dict(P=NT - step + 1), dict(eot=eot + 1),
                dict(V=eot)):
        assert _beam_call(model, st, cv, ct, **{**good, **bad})[0] == FW_EINVAL, bad

    def edited(key, idx, val):
        s2 = {k: v.copy() for k, v in st.items()}
        a, b = cv.copy(), ct.copy()
        if key == "ct":
            b[idx] = val
        else:
            s2[key][idx] = val
        return _beam_call(model, s2, a, b, **good)[0]

    assert edited("ct", (3, 1), eot + 1) == FW_EINVAL and edited("ct", (0, 0), -1) == FW_EINVAL
    assert edited("kvidx2", (step & 1, 4, 2), K) == FW_EINVAL
    assert edited("n_fin", 1, FIN_CAP + 1) == FW_EINVAL and edited("n_fin", 0, -1) == FW_EINVAL


# ------------------------------------------------------------------------------------------------ embedding
def _embed_call(model, tok, emb, pos_emb, d, pos_fixed, P, step, blk_n, sentinel=-7.0):
    L = _L()
    rows, R16 = len(tok), (len(tok) + 15) // 16 * 16
    tok = np.ascontiguousarray(tok, np.int32)
    x = np.zeros((rows, d), np.float32)
    xf = np.zeros((R16, d), np.float32)
    rc = model._lib.fw_test_dec_embed(model._replicas[0].handle, L.ptr(tok), rows, L.ptr(emb), emb.shape[0], L.ptr(pos_emb),
                                      pos_emb.shape[0], d, pos_fixed, P, step, blk_n, sentinel, L.ptr(x), L.ptr(xf))
    return rc, x, xf


EMBED_V, EMBED_NT = 37, 24
# (rows, pos_fixed, P, step, blk_n): fixed; the step counter with P - 1 + step the LAST position; position blocks
EMBED_MODES = [(r, 5, 0, 0, 0) for r in (1, 17, 33)] + [(r, -1, 4, EMBED_NT - 4, 0) for r in (1, 17, 33)] + \
    [(48, 3, 0, 0, 16), (35, EMBED_NT - 5, 0, 0, 5)]


@pytest.fixture(scope="module")
def embed_tables():
    rng = np.random.default_rng(3)
    return {d: (np.ascontiguousarray(rng.standard_normal((EMBED_V, d)), np.float32),
                np.ascontiguousarray(rng.standard_normal((EMBED_NT, d)) * 3, np.float32)) for d in (64, 384, 1280)}


@pytest.mark.parametrize("d", [64, 384, 1280])
@pytest.mark.parametrize("rows,pos_fixed,P,step,blk_n", EMBED_MODES)
def test_embed(model, embed_tables, d, rows, pos_fixed, P, step, blk_n):
    """bit-exact against fp16(fp32(E[tok]) + fp32(pos[p])), row-major and fragment-major; the padding rows of the last
    16-row fragment tile still hold the sentinel"""
    emb, pos_emb = embed_tables[d]
    rng = np.random.default_rng(rows * 31 + blk_n)
    tok = rng.integers(0, EMBED_V, rows)
    tok[0] = EMBED_V - 1                       # boundary and repeated tokens
    tok[-1] = tok[rows // 2] = 0 if rows > 1 else EMBED_V - 1
    rc, x, xf = _embed_call(model, tok, emb, pos_emb, d, pos_fixed, P, step, blk_n)
    _L().check(rc)
    pos = embed_positions(rows, pos_fixed, P, step, blk_n)
    assert pos.max() < EMBED_NT and (blk_n or pos_fixed >= 0 or pos[0] == EMBED_NT - 1)
    want = embed_ref(tok, emb, pos_emb, pos)
    assert np.array_equal(_bits(x), _bits(want))
    assert np.array_equal(_bits(xf[:rows]), _bits(want))
    assert (xf[rows:] == -7.0).all() and xf.shape[0] % 16 == 0 and (rows % 16 == 0 or xf.shape[0] > rows)


def test_embed_bad_arguments_are_refused(model, embed_tables):
    emb, pos_emb = embed_tables[64]
    ok = dict(tok=[1, 2, 3, 4], emb=emb, pos_emb=pos_emb, d=64, pos_fixed=2, P=1, step=0, blk_n=0)
    assert _embed_call(model, **ok)[0] == 0
    for bad in (dict(tok=[1, EMBED_V, 3, 4]), dict(tok=[-1, 2, 3, 4]), dict(blk_n=17), dict(blk_n=3), dict(blk_n=-1),
                dict(blk_n=4, pos_fixed=EMBED_NT - 3), dict(blk_n=2, pos_fixed=-1), dict(pos_fixed=EMBED_NT),
                dict(pos_fixed=-1, P=0), dict(pos_fixed=-1, P=2, step=EMBED_NT - 1), dict(pos_fixed=-1, P=1, step=-1),
                dict(d=48), dict(d=0)):
        assert _embed_call(model, **{**ok, **bad})[0] == FW_EINVAL, bad


# ------------------------------------------------------------------------------------------------ align post-processing
def _align_call(model, probs, n_tok, nfr, width, mat):
    L = _L()
    B, n_sel, cap, T = probs.shape
    n_tok, nfr = np.ascontiguousarray(n_tok, np.int32), np.ascontiguousarray(nfr, np.int32)
    out = np.ascontiguousarray(mat, np.float32).copy()
    rc = model._lib.fw_test_align_post(model._replicas[0].handle, L.ptr(probs), B, n_sel, cap, T, L.ptr(n_tok), L.ptr(nfr),
                                       width, L.ptr(out))
    return rc, out


def _softmax_like(rng, shape):
    """positive rows that sum to one over the frames (last axis), float32"""
    x = rng.standard_normal(shape) * 2
    p = np.exp(x - x.max(axis=-1, keepdims=True))
    return np.ascontiguousarray(p / p.sum(axis=-1, keepdims=True), np.float32)


def _align_check(model, probs, n_tok, nfr, width, what):
    B, n_sel, cap, T = probs.shape
    for b in range(B):    # the input has strictly positive variance over the tokens in every frame that is used
        assert (probs[b, :, :n_tok[b], :nfr[b]].astype(np.float64).std(axis=-2) > 0).all()
        assert (probs[b] > 0).all()
    mat = np.full((B, cap, T), SENT_F, np.float32)
    rc, got = _align_call(model, probs, n_tok, nfr, width, mat)
    _L().check(rc)
    ref = align_post_ref(probs, n_tok, nfr, width, mat)
    f32 = align_post_fp32(probs, n_tok, nfr, width, mat)
    used = np.zeros((B, cap, T), bool)
    for b in range(B):
        used[b, :n_tok[b], :nfr[b]] = True
    assert np.array_equal(_bits(got[~used]), _bits(mat[~used]))         # nothing outside n_tok x nfr is written
    bound = 4 * float(np.abs(f32.astype(np.float64) - ref)[used].max())
    dev = float(np.abs(got.astype(np.float64) - ref)[used].max())
    print(f"align {what}: kernel vs fp64 {dev:.3e}, bound 4 x (fp32 restatement vs fp64) {bound:.3e}")
    assert bound > 0 and dev <= bound, (what, dev, bound)
    return dev, bound


@pytest.mark.parametrize("n_sel", [1, 6])
@pytest.mark.parametrize("T", [200, 64])
@pytest.mark.parametrize("width", [1, 3, 7, 15])
def test_align_post(model, width, T, n_sel):
    """B = 3 chunks of n_tok = (3, 9, 20 = n_tok_cap) in one launch; the frame counts {T, 77, pad, pad + 1, 1} rotate
    over the chunks in five launches (pad = width // 2: a window wider than the frames, and both reflections folding;
    77 is replaced by T - 1 where T < 77, pad by 1 where it is 0)"""
    rng = np.random.default_rng(width * 1000 + T + n_sel)
    pad = width // 2
    n_tok = [3, 9, 20]
    probs = _softmax_like(rng, (3, n_sel, 20, T))
    frames = [T, min(77, T - 1), max(pad, 1), pad + 1, 1]
    for rot in range(5):
        nfr = [frames[(b + rot) % 5] for b in range(3)]
        _align_check(model, probs, n_tok, nfr, width, f"w={width} T={T} n_sel={n_sel} nfr={nfr}")


def test_align_post_long_token_sums(model):
    """n_tok = 448: the long sequential fp32 sums of the statistics kernel"""
    rng = np.random.default_rng(448)
    probs = _softmax_like(rng, (2, 2, 448, 64))
    _align_check(model, probs, [448, 100], [64, 37], 7, "n_tok=448")


def test_align_bad_arguments_are_refused(model):
    rng = np.random.default_rng(2)
    probs = _softmax_like(rng, (2, 2, 5, 32))
    mat = np.zeros((2, 5, 32), np.float32)
    assert _align_call(model, probs, [5, 2], [32, 1], 7, mat)[0] == 0
    for n_tok, nfr, width in (([0, 2], [32, 1], 7), ([6, 2], [32, 1], 7), ([5, 2], [0, 1], 7), ([5, 2], [32, 33], 7),
                              ([5, 2], [32, 1], 4), ([5, 2], [32, 1], 17), ([5, 2], [32, 1], 0), ([5, 2], [32, 1], -1)):
        assert _align_call(model, probs, n_tok, nfr, width, mat)[0] == FW_EINVAL, (n_tok, nfr, width)
    L = _L()
    z = np.zeros(2, np.int32) + 1
    assert model._lib.fw_test_align_post(model._replicas[0].handle, L.ptr(probs), 2, 0, 5, 32, L.ptr(z), L.ptr(z), 7,
                                         L.ptr(mat)) == FW_EINVAL
