"""The decoder's attention kernels one by one (dec_kernels.hip: dec_self_attn_kernel / dec_self_attn2_kernel,
dec_cross_attn_kernel, dec_cross_probs_kernel, dec_nospeech_kernel, dec_token_prob_kernel) through the C-ABI hooks of
include/fwamd_test.h, against float64 references built from the fp16-rounded inputs, at the edges where these kernels
can go wrong: slot-table indirection and its step parity, the position batches of every self-attention form up to the
last position 447, the padded keys and idle waves of the cross-attention, skipped chunks, the encoder-chunk map,
position blocks, and the fragment-major against the row-major output.

Each tolerance is derived from the kernel's rounding points (written beside the assert), not fitted to a run.  Every
bit-identity assert sits next to an fp64 check, so that "identical" cannot mean "identically wrong"."""
import numpy as np
import pytest

from conftest import make_model

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24   # float32 unit roundoff
U16 = 2.0 ** -11   # float16 unit roundoff (round to nearest)
N_CTX = 448        # the text context of every Whisper model: the slot-table stride and the last position 447 + 1


@pytest.fixture(scope="module")
def model():
    _, _, m = make_model("micro", max_batch=2, max_beam=2)
    return m


def _h(x):  # fp16 rounding (what the device holds)
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _lib():
    from faster_whisper_amd import _lib as L
    return L, L.load()


def _knob(knob, value, fn):
    """fn() with measurement knob `knob` set to `value`; the product's default (0) is restored whatever happens"""
    L, lib = _lib()
    L.check(lib.fw_test_knob(knob, value))
    try:
        return fn()
    finally:
        L.check(lib.fw_test_knob(knob, 0))


def _softmax64(s, axis=-1):
    s = s - s.max(axis, keepdims=True)
    p = np.exp(s)
    return p / p.sum(axis, keepdims=True)


# ------------------------------------------------------------------------------------------------ self-attention
def _self_attn(model, qkv, kc, vc, kvidx, n_chunks, kmul, Kbeam, H, cache_ctx, pos_fixed, P, step, blk_n, frag, form):
    L, lib = _lib()
    kc, vc = kc.copy(), vc.copy()
    out = np.full((qkv.shape[0], H * 64), np.nan, np.float32)

    def go():
        L.check(lib.fw_test_dec_self_attn(model._replicas[0].handle, L.ptr(qkv), L.ptr(kc), L.ptr(vc), L.ptr(kvidx),
                                          n_chunks, kmul, Kbeam, H, N_CTX, cache_ctx, pos_fixed, P, step, blk_n, frag,
                                          L.ptr(out)))
    _knob(2, form, go)
    return out, kc, vc


def _self_bound(ref, A, vmax):
    """fp32 scores, softmax and P V, one fp16 rounding of the output (dec_kernels.hip K13):
      - the output store: U16 * |ref|;
      - a score is a sum of 64 fp32 products (q * 0.125 is exact): in any order <= 64 U32 * sum |q_e k_e| / 8 <= 64 U32 A,
        and a score error e moves the output by at most 2 e max|v| (softmax weights sum to one);
      - __expf (argument rounding and v_exp_f32, ~2 ulp on weights that matter), the sum of <= 448 weights (7 per lane +
        a 6-level wave tree), the P V accumulation (<= 56 fmas per lane + 3 shuffles), 1 / sum: < 128 U32 in all,
        taken as 256 U32 of max|v|"""
    return U16 * np.abs(ref) + (2 * 64 * U32 * A + 256 * U32) * vmax


def _self_case(rng, n_chunks, kmul, Kbeam, H, cache_ctx):
    d, R, Rt = H * 64, n_chunks * kmul, n_chunks * Kbeam
    qkv = _h(rng.standard_normal((R, 3 * d)))
    kc = _h(rng.standard_normal((Rt, H, cache_ctx, 64)))
    vc = _h(rng.standard_normal((Rt, H, cache_ctx, 64)))
    # every byte of both parity halves, at every position up to n_ctx, a valid beam (the kernels make addresses of them);
    # the two halves drawn independently, so that reading the wrong one changes the answer
    kvidx = rng.integers(0, Kbeam, size=(2, Rt, N_CTX), dtype=np.uint8)
    return qkv, kc, vc, kvidx


def _self_ref(qkv, kc, vc, kvidx, n_chunks, kmul, Kbeam, H, pos, cur):
    """fp64 reference of one decode step: row r = c * kmul + w (slot c * Kbeam + w) at position pos reads key p < pos from
    slot c * Kbeam + kvidx[cur][slot][p] and its own new key at pos.  Returns out, the mask of cache rows
    [slot][position] the step may read, A = max sum |q_e k_e| / 8 (for the bound) and each row's own slot."""
    d, R = H * 64, n_chunks * kmul
    r = np.arange(R)
    c, w = r // kmul, r % kmul
    slot = c * Kbeam + w
    q = qkv[:, :d].reshape(R, H, 64).astype(np.float64)
    kn = qkv[:, d:2 * d].reshape(R, H, 64)
    vn = qkv[:, 2 * d:].reshape(R, H, 64)
    src = c[:, None] * Kbeam + kvidx[cur, slot, :pos].astype(np.int64)       # (R, pos)
    pidx = np.arange(pos)[None, :]
    Kall = np.concatenate([kc[src, :, pidx, :], kn[:, None]], axis=1).astype(np.float64)   # (R, pos + 1, H, 64)
    Vall = np.concatenate([vc[src, :, pidx, :], vn[:, None]], axis=1).astype(np.float64)
    p = _softmax64(np.einsum("rhe,rphe->rhp", q, Kall) / 8.0)
    out = np.einsum("rhp,rphe->rhe", p, Vall).reshape(R, d)
    A = np.einsum("rhe,rphe->rhp", np.abs(q), np.abs(Kall)).max() / 8.0
    read = np.zeros(kc.shape[0:1] + kc.shape[2:3], bool)
    read[src, np.broadcast_to(pidx, src.shape)] = True
    return out, read, A, slot


def _poison(kc, vc, read):
    """NaN in every cache row the step must not read: a stray read fails the fp64 check instead of hiding behind a
    zero softmax weight"""
    m = ~read[:, None, :, None]
    return np.where(m, np.float32(np.nan), kc), np.where(m, np.float32(np.nan), vc)


def _run_self_case(model, rng, n_chunks, kmul, Kbeam, H, pos, cache_ctx, route, what):
    qkv, kc, vc, kvidx = _self_case(rng, n_chunks, kmul, Kbeam, H, cache_ctx)
    if route == "step":   # pos = P - 1 + step, slot-table half step & 1: an ODD step reads half 1
        step = 1 if pos < 3 else 3
        pos_fixed, P, cur = -1, pos + 1 - step, 1
    else:
        step, pos_fixed, P, cur = 5, pos, 0, 0   # (an explicit position reads half 0, whatever the step counter holds)
    ref, read, A, slot = _self_ref(qkv, kc, vc, kvidx, n_chunks, kmul, Kbeam, H, pos, cur)
    kc, vc = _poison(kc, vc, read)
    d = H * 64
    ekc, evc = kc.copy(), vc.copy()
    ekc[slot, :, pos, :] = qkv[:, d:2 * d].reshape(-1, H, 64)
    evc[slot, :, pos, :] = qkv[:, 2 * d:].reshape(-1, H, 64)
    outs = {}
    for form, frag in ((0, 1), (1, 1), (2, 1), (3, 1), (0, 0)):
        out, okc, ovc = _self_attn(model, qkv, kc, vc, kvidx, n_chunks, kmul, Kbeam, H, cache_ctx, pos_fixed, P, step, 0,
                                   frag, form)
        # the new K / V land bit for bit at (own slot, pos); every other cache element is left as it was
        assert np.array_equal(okc, ekc, equal_nan=True), f"{what} form {form} frag {frag}: K cache"
        assert np.array_equal(ovc, evc, equal_nan=True), f"{what} form {form} frag {frag}: V cache"
        outs[(form, frag)] = out
    out = outs[(0, 1)]
    vmax = np.abs(qkv[:, 2 * H * 64:]).max() if pos == 0 else max(np.abs(qkv[:, 2 * H * 64:]).max(),
                                                                   np.nanmax(np.abs(vc)))
    bound = _self_bound(ref, A, vmax)
    err = np.abs(out - ref)
    print(f"self-attn {what}: max err {err.max():.2e}, worst err / bound {(err / bound).max():.3f}")
    assert np.all(np.isfinite(out)), f"{what}: non-finite output (a poisoned cache row was read)"
    assert np.all(err <= bound), f"{what}: max err {err.max():.3e}"
    # forms 1 (first), 2 (latency), 3 (throughput) and the product's choice: the same bits; fp16 fragment-major output
    # and the int8 path's row-major output: the same values
    for key, o in outs.items():
        assert np.array_equal(o, out), f"{what}: form {key[0]} frag {key[1]} differs from the product's choice"


SELF_POS = [0, 1, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 447]


@pytest.mark.parametrize("pos", SELF_POS)
@pytest.mark.parametrize("route,cache", [("fixed", "reach"), ("step", "full"), ("fixed", "full"), ("step", "reach")])
def test_self_attn_positions(model, pos, route, cache):
    """every position-batch boundary of the forms (32 / 64 / 128 / 256) up to the last position 447, with the cache
    sized to the run's reach (rounded up to 8) and to the whole context; explicit positions and the step-counter route
    with an odd step (the other slot-table half).  Five beams of two chunks, slot tables that point anywhere in the
    chunk."""
    cache_ctx = N_CTX if cache == "full" else (pos + 1 + 7) // 8 * 8
    rng = np.random.default_rng(1000 + pos * 4 + ["fixed", "step"].index(route) * 2 + int(cache == "full"))
    _run_self_case(model, rng, 2, 5, 5, 6, pos, cache_ctx, route, f"pos {pos} {route} cache {cache_ctx}")


# (kmul, Kbeam, H, n_chunks, pos, route): kmul 1 .. 16 with spare slots (Kbeam > kmul) in some; the product's form rule
# on both sides (kmul <= 8 and H * n_chunks <= 768: latency form; otherwise throughput form): 20 x 38 = 760, 20 x 40 = 800
SELF_GEOMS = [
    (1, 1, 2, 3, 200, "step"), (2, 3, 6, 3, 129, "fixed"), (5, 5, 20, 2, 100, "step"), (8, 8, 6, 2, 300, "fixed"),
    (8, 9, 2, 3, 65, "step"), (9, 10, 2, 2, 447, "step"), (16, 16, 20, 2, 64, "fixed"), (16, 17, 6, 1, 257, "step"),
    (1, 2, 20, 38, 100, "step"), (1, 2, 20, 40, 100, "step"), (5, 5, 20, 40, 33, "fixed"),
]


@pytest.mark.parametrize("kmul,Kbeam,H,n_chunks,pos,route", SELF_GEOMS)
def test_self_attn_geometries(model, kmul, Kbeam, H, n_chunks, pos, route):
    rng = np.random.default_rng(kmul * 1000 + H * 10 + n_chunks)
    _run_self_case(model, rng, n_chunks, kmul, Kbeam, H, pos, (pos + 1 + 7) // 8 * 8, route,
                   f"kmul {kmul} Kbeam {Kbeam} H {H} chunks {n_chunks} pos {pos} {route}")


@pytest.mark.parametrize("blk_n", [1, 5, 16])
@pytest.mark.parametrize("pos_fixed", [0, 1, 100, 432])
def test_self_attn_position_blocks(model, blk_n, pos_fixed):
    """position blocks (prompt forward, align): row c * blk + j is position pos_fixed + j of chunk c's beam slot 0;
    earlier positions come from the cache, the block's own from its sibling rows (causally).  blk_n = 16 > Kbeam = 5 as
    in align.  Also the same bits as blk_n one-position launches run one after another, each on the cache the previous
    one left (dec_kernels.hip: 'the same values in the same order as position-by-position launches')."""
    n_chunks, Kbeam, H = 3, 5, 6
    d, R = H * 64, n_chunks * blk_n
    cache_ctx = N_CTX if pos_fixed == 432 else (pos_fixed + blk_n + 7) // 8 * 8
    rng = np.random.default_rng(77 + blk_n * 1000 + pos_fixed)
    qkv, kc, vc, kvidx = _self_case(rng, n_chunks, blk_n, Kbeam, H, cache_ctx)
    q = qkv[:, :d].reshape(n_chunks, blk_n, H, 64).astype(np.float64)
    kn = qkv[:, d:2 * d].reshape(n_chunks, blk_n, H, 64)
    vn = qkv[:, 2 * d:].reshape(n_chunks, blk_n, H, 64)
    s0 = np.arange(n_chunks) * Kbeam
    Kall = np.concatenate([kc[s0, :, :pos_fixed].transpose(0, 2, 1, 3), kn], axis=1).astype(np.float64)  # (c, pf+blk, H, 64)
    Vall = np.concatenate([vc[s0, :, :pos_fixed].transpose(0, 2, 1, 3), vn], axis=1).astype(np.float64)
    s = np.einsum("cjhe,cphe->cjhp", q, Kall) / 8.0
    causal = np.arange(pos_fixed + blk_n)[None, :] > (pos_fixed + np.arange(blk_n))[:, None]      # (j, p)
    s[np.broadcast_to(causal[None, :, None, :], s.shape)] = -np.inf
    ref = np.einsum("cjhp,cphe->cjhe", _softmax64(s), Vall).reshape(R, d)
    A = np.einsum("cjhe,cphe->cjhp", np.abs(q), np.abs(Kall)).max() / 8.0
    read = np.zeros((n_chunks * Kbeam, cache_ctx), bool)
    read[s0, :pos_fixed] = True
    wrote = np.zeros_like(read)
    wrote[s0, pos_fixed:pos_fixed + blk_n] = True
    kc, vc = _poison(kc, vc, read)
    ekc, evc = _poison(kc, vc, read | wrote)
    for j in range(blk_n):
        ekc[s0, :, pos_fixed + j] = kn[:, j]
        evc[s0, :, pos_fixed + j] = vn[:, j]
    outs = []
    for frag in (1, 0):
        out, okc, ovc = _self_attn(model, qkv, kc, vc, kvidx, n_chunks, blk_n, Kbeam, H, cache_ctx, pos_fixed, 0, 0,
                                   blk_n, frag, 0)
        assert np.array_equal(okc, ekc, equal_nan=True) and np.array_equal(ovc, evc, equal_nan=True), f"frag {frag}: cache"
        outs.append(out)
    out = outs[0]
    bound = _self_bound(ref, A, max(np.abs(vn).max(), np.nanmax(np.abs(vc)) if pos_fixed else 0.0))
    err = np.abs(out - ref)
    print(f"self-attn block {blk_n} at {pos_fixed}: max err {err.max():.2e}, worst err / bound {(err / bound).max():.3f}")
    assert np.all(np.isfinite(out)) and np.all(err <= bound), f"max err {err.max():.3e}"
    assert np.array_equal(outs[1], out), "row-major and fragment-major outputs differ"
    # the same positions one launch at a time (kvidx all zero: every row reads its chunk's slot 0, as the prompt does)
    zero_idx = np.zeros_like(kvidx)
    ckc, cvc = kc, vc
    seq = np.empty_like(out)
    for j in range(blk_n):
        rows = np.arange(n_chunks) * blk_n + j
        o, ckc, cvc = _self_attn(model, np.ascontiguousarray(qkv[rows]), ckc, cvc, zero_idx, n_chunks, 1, Kbeam, H,
                                 cache_ctx, pos_fixed + j, 0, 0, 0, 1, 0)
        seq[rows] = o
    assert np.array_equal(seq, out), "a position block differs from position-by-position launches"
    assert np.array_equal(ckc, ekc, equal_nan=True) and np.array_equal(cvc, evc, equal_nan=True)


# ------------------------------------------------------------------------------------------------ cross-attention
def _cross_attn(model, q, k, v, T, H, B, kmul, kv_div, slot_map, done, frag, k_pad, out0, cap):
    L, lib = _lib()
    out = out0.copy()
    dp = L.ptr(done) if done is not None else None

    def go():
        L.check(lib.fw_test_dec_cross_attn(model._replicas[0].handle, L.ptr(q), L.ptr(k), L.ptr(v), k.shape[0], T, H, B,
                                           kmul, kv_div, L.ptr(slot_map), dp, frag, k_pad, L.ptr(out)))
    _knob(7, cap, go)
    return out


# (T, H, kmul, B, kv_div, scale, with_done): T = 1500 (the product's: 4 padded keys in the last 32-key group) first;
# 33 (two groups, six of the eight waves idle), 100, 1473 (31 padded keys); kv_div 3: several decode chunks per
# encoder chunk (sampling)
CROSS_CASES = [
    (1500, 20, 5, 6, 3, 1.0, True), (1500, 6, 16, 4, 1, 3.0, True), (1500, 2, 1, 5, 1, 3.0, False),
    (1500, 20, 2, 3, 1, 3.0, True), (1500, 6, 5, 7, 3, 1.0, False),
    (33, 6, 5, 3, 1, 1.0, True), (33, 2, 16, 3, 3, 3.0, False), (100, 2, 16, 6, 3, 3.0, True),
    (100, 20, 1, 4, 1, 1.0, True), (1473, 6, 2, 4, 1, 1.0, True), (1473, 20, 5, 5, 3, 3.0, True),
]


@pytest.mark.parametrize("T,H,kmul,B,kv_div,scale,with_done", CROSS_CASES)
def test_cross_attn(model, T, H, kmul, B, kv_div, scale, with_done):
    """decode chunk c attends to encoder chunk slot_map[c // kv_div] (a map that permutes and repeats the three encoder
    chunks); done chunks keep the caller's rows; K's padded keys hold a large finite value (the pool only promises V^T
    zeros there).  Scale 3: keys sorted along the key axis (rising for even heads, falling for odd), so that the 8 waves,
    which stride over 32-key groups, see widely different maxima and move them group after group."""
    d, R, n_enc = H * 64, B * kmul, 3
    rng = np.random.default_rng(T * 31 + H * 7 + kmul + B)
    q = _h(scale * rng.standard_normal((R, d)))
    k = _h(scale * rng.standard_normal((n_enc, T, d)))
    v = _h(rng.standard_normal((n_enc, T, d)))
    if scale > 1:
        for e in range(n_enc):
            for h in range(H):
                o = np.argsort(k[e, :, h * 64] * (1 if h % 2 == 0 else -1))
                k[e, :, h * 64:(h + 1) * 64] = k[e, o, h * 64:(h + 1) * 64]
    n_map = (B + kv_div - 1) // kv_div
    slot_map = np.array([2, 0, 2, 1, 0, 1, 2][:n_map], np.int32)
    done = None
    if with_done:
        done = np.zeros(B, np.int32)
        done[1] = 1
        done[B - 1] = 1
    sentinel = _h(rng.uniform(-4, 4, (R, d)))
    k_pad = 30000.0   # finite in fp16; as a score it would swamp every real key
    qh = q.reshape(B, kmul, H, 64).astype(np.float64)
    ke = k[slot_map[np.arange(B) // kv_div]].reshape(B, T, H, 64).astype(np.float64)
    ve = v[slot_map[np.arange(B) // kv_div]].reshape(B, T, H, 64).astype(np.float64)
    p = _softmax64(np.einsum("cjhe,cthe->cjht", qh, ke) / 8.0)
    ref = np.einsum("cjht,cthe->cjhe", p, ve).reshape(R, d)
    A = np.einsum("cjhe,cthe->cjht", np.abs(qh), np.abs(ke)).max() / 8.0
    live = np.ones(R, bool) if done is None else np.repeat(done == 0, kmul)
    outs = {}
    for cap, frag in ((0, 1), (1, 1), (2, 1), (0, 0)):
        outs[(cap, frag)] = _cross_attn(model, q, k, v, T, H, B, kmul, kv_div, slot_map, done, frag, k_pad, sentinel, cap)
    out = outs[(0, 1)]
    # rounding points beyond the self-attention's (dec_kernels.hip K14): the scores come out of MFMAs (any order of the
    # 64 products) and are scaled by log2(e) in fp32 (66 U32 A in all); P is rounded to fp16 before the P V MFMA, relative
    # to the wave's running maximum (<= 1): U16 of each weight, or 2^-25 absolute for a weight in the fp16 subnormal
    # range, i.e. (U16 + T 2^-25) max|v| with a softmax sum >= 1; the 8-wave merge and the online rescales (<= 6 per
    # lane) stay inside the 256 U32 slack
    vmax = np.abs(v).max()
    bound = U16 * np.abs(ref) + (2 * 66 * U32 * A + U16 + T * 2.0 ** -25 + 256 * U32) * vmax
    err = np.abs(out - ref)[live]
    print(f"cross-attn T {T} H {H} kmul {kmul} B {B} kv_div {kv_div} scale {scale}: max err {err.max():.2e}, "
          f"worst err / bound {(err / bound[live]).max():.3f}")
    assert np.all(np.isfinite(out)), "non-finite output"
    assert np.all(err <= bound[live]), f"max err {err.max():.3e}"
    assert np.array_equal(out[~live], sentinel[~live]), "a done chunk's rows were written"
    # the three register caps (knob 7): the same bits; fp16 fragment-major and int8-path row-major output: the same values
    for key, o in outs.items():
        assert np.array_equal(o, out), f"register cap {key[0]} frag {key[1]} differs"


# ------------------------------------------------------------------------------------------------ align probabilities
@pytest.mark.parametrize("blk_n", [1, 16])
def test_cross_probs(model, blk_n):
    """probs[b][hs][tok_idx + j][t] = softmax_t(q[b * blk + j][heads[hs]] . K_b[t] / 8) at T = 1500 for non-contiguous
    heads (as the alignment heads of large-v3 pick them); token slots outside the block keep the caller's values"""
    L, lib = _lib()
    B, T, H, n_tok, tok_idx = 3, 1500, 20, 21, 4
    blk = max(blk_n, 1)
    heads = np.array([7, 2, 15, 19, 11], np.int32)
    n_sel, d = len(heads), H * 64
    rng = np.random.default_rng(40 + blk_n)
    q = _h(rng.standard_normal((B * blk, d)))
    k = _h(rng.standard_normal((B, T, d)))
    probs = rng.uniform(-1, 0, (B, n_sel, n_tok, T)).astype(np.float32)   # negative: no probability
    before = probs.copy()
    L.check(lib.fw_test_dec_cross_probs(model._replicas[0].handle, L.ptr(q), L.ptr(k), B, T, H, L.ptr(heads), n_sel,
                                        n_tok, tok_idx, blk_n, L.ptr(probs)))
    qh = q.reshape(B, blk, H, 64)[:, :, heads].astype(np.float64)           # (b, j, hs, 64)
    kh = k.reshape(B, T, H, 64)[:, :, heads].astype(np.float64)             # (b, t, hs, 64)
    s = np.einsum("bjse,btse->bsjt", qh, kh) / 8.0
    ref = _softmax64(s)
    A = np.einsum("bjse,btse->bsjt", np.abs(qh), np.abs(kh)).max() / 8.0
    x = s - s.max(-1, keepdims=True)
    got = probs[:, :, tok_idx:tok_idx + blk]
    # fp32 throughout (dec_cross_probs_kernel): a score <= 64 U32 A off (2 x that on a probability, relative); __expf of
    # x = s - max: the subtraction and the argument's scaling by log2(e) ~ 2 |x| U32, v_exp_f32 ~ 2 U32; the sum of 1500
    # weights (6 per lane, a 6-level wave tree, 4 partials) and 1 / sum, one product: < 20 U32; fp32 underflow: 2^-126
    bound = ref * (2 * 64 * U32 * A + (2 * np.abs(x) + 24) * U32) + 2.0 ** -126
    err = np.abs(got - ref)
    print(f"cross probs blk {blk_n}: max err {err.max():.2e} (max prob {ref.max():.3f}), "
          f"worst err / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound), f"max err {err.max():.3e}"
    untouched = np.ones(n_tok, bool)
    untouched[tok_idx:tok_idx + blk] = False
    assert np.array_equal(probs[:, :, untouched], before[:, :, untouched]), "a token slot outside the block was written"


# ------------------------------------------------------------------------------------------------ no-speech / token prob
@pytest.mark.parametrize("V", [700, 1913, 51865, 51866])
@pytest.mark.parametrize("row_mul", [1, 5])
def test_softmax_picks(model, V, row_mul):
    """softmax(logits[b * row_mul])[target] in fp64: ordinary logits; logits spread over +-1e3 (nearly every exponential
    underflows); a row whose maximum sits in another wave than thread 0's (v = 500: thread 500 of the 1024) with the
    target just below it.  Token probabilities also for targets outside [0, V) (0 by contract)."""
    L, lib = _lib()
    rows = 4
    rng = np.random.default_rng(V + row_mul)
    lg = (3.0 * rng.standard_normal((rows * row_mul, V))).astype(np.float32)
    lg[1 * row_mul] = rng.uniform(-1e3, 1e3, V).astype(np.float32)
    r2 = lg[2 * row_mul]
    r2[:] = rng.uniform(-8, 0, V)
    r2[500] = 12.0                       # the row maximum, in wave 7; thread 0's wave holds nothing above 0
    tgt_ns = min(V - 1, 613)             # the no-speech id: a token of wave 9 (of wave 613 - 512 = 101 for V = 700)
    for b in range(rows):
        row = lg[b * row_mul]
        row[tgt_ns] = row.max() - 1.5    # a probability that matters in every row
    lg[3 * row_mul, 7] = lg[3 * row_mul].max() + 0.25
    h = model._replicas[0].handle
    out_ns = np.full(rows, np.nan, np.float32)
    L.check(lib.fw_test_dec_softmax_pick(h, L.ptr(lg), rows, V, row_mul, L.ptr(np.full(rows, tgt_ns, np.int32)), 1,
                                         L.ptr(out_ns)))
    targets = np.array([tgt_ns, int(np.argmax(lg[row_mul])), 500, -1], np.int32)
    out_tp = np.full(rows, np.nan, np.float32)
    L.check(lib.fw_test_dec_softmax_pick(h, L.ptr(lg), rows, V, row_mul, L.ptr(targets), 0, L.ptr(out_tp)))
    out_hi = np.full(rows, np.nan, np.float32)
    hi = np.full(rows, V, np.int32)
    L.check(lib.fw_test_dec_softmax_pick(h, L.ptr(lg), rows, V, row_mul, L.ptr(hi), 0, L.ptr(out_hi)))
    x = lg[::row_mul].astype(np.float64)
    x -= x.max(-1, keepdims=True)
    p = np.exp(x) / np.exp(x).sum(-1, keepdims=True)
    per_thread = (V + 1023) // 1024
    for name, got, tg in (("no-speech", out_ns, np.full(rows, tgt_ns)), ("token prob", out_tp, targets)):
        ok = (tg >= 0) & (tg < V)
        ref = np.where(ok, p[np.arange(rows), np.clip(tg, 0, V - 1)], 0.0)
        xt = np.where(ok, x[np.arange(rows), np.clip(tg, 0, V - 1)], 0.0)
        # fp32: the target's exponential ~ (2 |x| + 2) U32 (subtraction, argument scaling, v_exp_f32); the sum: a lane's
        # ceil(V / 1024) terms in order, a 6-level wave tree, 16 wave partials in order; the division: 1 U32;
        # fp32 underflow: 2^-126
        bound = ref * ((2 * np.abs(xt) + 2 + per_thread + 6 + 16 + 1) * U32) + 2.0 ** -126
        err = np.abs(got - ref)
        print(f"{name} V {V} row_mul {row_mul}: max err {err.max():.2e}, worst err / bound {(err / bound).max():.3f}")
        assert np.all(err <= bound), f"{name}: {got} vs {ref}"
    assert np.all(out_hi == 0.0), "a target >= V must give probability 0"
