"""The encoder GEMM (gemm.hip) in the forms the product launches — batched, strided, gapped, blocked tile order,
layered, int8 — and the row kernels in front of it (rowops.hip), each against a plain high-precision reference.

Every output buffer starts as a sentinel that is exact in fp16 and carries at least 64 elements of tail; after the
launch every element outside the described output must still hold it.  The tile is 256 x 256 x 64 halves: M = 300 is
two m tiles, the last one 44 rows.  References and helpers: tests/gemm_refs.py (checked on the CPU by
tests/test_gemm_refs.py)."""
import numpy as np
import pytest

import gemm_refs as gr
from conftest import make_model
from gemm_refs import SENTINEL, h16

pytestmark = pytest.mark.gpu

M = 300
TAIL = 64


@pytest.fixture(scope="module")
def model():
    return make_model("micro", max_batch=2, max_beam=2)[2]


@pytest.fixture(scope="module")
def kmodel():
    return make_model("micro", max_batch=2, max_beam=2, compute_type="int8_float16")[2]


def _lib():
    from faster_whisper_amd import _lib as L
    return L, L.load()


def _p(a):
    L, _ = _lib()
    return L.ptr(a) if a is not None else None


def _f32(a):
    return np.ascontiguousarray(a, np.float32) if a is not None else None


def gemm_ex(model, A, lda, a_bs, W, bias, C, ldc, c_bs, N, K, batch, res=None, ldr=0, r_bs=0, c_off=0, c_ls=0, m=M,
            n_layers=1, act=0, trans=0, head_rows=0, int8=0, ln=None, a_elems=None, r_elems=None, c_elems=None):
    """one fw_test_gemm_ex launch on flat float32 buffers (C in place); returns the status code"""
    L, lib = _lib()
    A, W, bias, res = _f32(A).reshape(-1), _f32(W), _f32(bias), (_f32(res).reshape(-1) if res is not None else None)
    assert C.dtype == np.float32 and C.ndim == 1 and C.flags.c_contiguous
    g, b = (_f32(ln[0]), _f32(ln[1])) if ln is not None else (None, None)
    return lib.fw_test_gemm_ex(model._replicas[0].handle, _p(A), A.size if a_elems is None else a_elems, lda, a_bs,
                               _p(W), _p(bias), _p(res), (res.size if res is not None else 0) if r_elems is None else r_elems,
                               ldr, r_bs, _p(C), C.size if c_elems is None else c_elems, c_off, ldc, c_bs, c_ls, m, N, K,
                               batch, n_layers, act, trans, head_rows, int8, _p(g), _p(b))


def gemm_ok(*a, **k):
    L, _ = _lib()
    L.check(gemm_ex(*a, **k))


def gemm_one(model, A, W, bias=None, res=None, act=0, int8=0):
    """fw_test_gemm: the contiguous single-chunk form"""
    L, lib = _lib()
    m, K = A.shape
    N = W.shape[0]
    out = np.empty((N, m) if act >= 2 else (m, N), np.float32)
    A, W, bias, res = _f32(A), _f32(W), _f32(bias), _f32(res)
    L.check(lib.fw_test_gemm(model._replicas[0].handle, _p(A), _p(W), _p(bias), _p(res), m, N, K, act, int8, _p(out)))
    return out


def operands(rng, batch, m, N, K, n_layers=1, a_scale=1.0, w_scale=1.0):
    """fp16-rounded operands with asymmetric row and column scalings: a transposed or shifted tile cannot pass"""
    A = h16(a_scale * rng.standard_normal((batch, m, K)) * (1.0 + np.arange(m)[None, :, None] / m)
            * (1.0 + 0.25 * np.arange(batch)[:, None, None]))
    W = h16(w_scale * rng.standard_normal((n_layers, N, K)) * (0.5 + np.arange(N)[None, :, None] / N)
            * (1.0 + 0.5 * np.arange(n_layers)[:, None, None]))
    b = h16(rng.standard_normal((n_layers, N)))
    return A, (W if n_layers > 1 else W[0]), (b if n_layers > 1 else b[0])


def strided(x, ld, bstride, tail=0, fill=0.0):
    """x [batch][rows][cols] laid out with row stride ld and chunk stride bstride in a flat float32 buffer"""
    batch, rows, cols = x.shape
    buf = np.full((batch - 1) * bstride + (rows - 1) * ld + cols + tail, fill, np.float32)
    gr.view3(buf, 0, batch, bstride, rows, ld, cols)[...] = x
    return buf


def check_sentinel(C, *views):
    keep = gr.untouched(C, *views)
    assert keep[-TAIL:].all()
    bad = np.flatnonzero(keep & (C != SENTINEL))
    assert bad.size == 0, f"{bad.size} elements outside the output were written, first at {bad[:8]}"


def rel_err(out, ref):
    return float(np.abs(out - ref).max() / max(1.0, np.abs(ref).max()))


def check_fp64(out, ref, epilogue, what):
    """2e-3 relative to max(1, max |ref|) (test_gemm_plain); the GELU / residual forms at test_gemm_epilogues' bound"""
    if epilogue:
        err, lim = float(np.abs(out - ref).max()), 2e-2 * max(1.0, np.abs(ref).max() / 4)
    else:
        err, lim = rel_err(out, ref), 2e-3
    print(f"{what}: err {err:.2e} (bound {lim:.2e})")
    assert err < lim, what


# ------------------------------------------------------------------------------------------------------------------
# A. strided, batched, row-major and transposed output
# ------------------------------------------------------------------------------------------------------------------
# ldc = N + 4 = 264 and 272 are multiples of 8 (16-byte stores; the last 8-column segment, N % 8 = 4, still takes the
# scalar path); ldc = 268 is the stride at which vec_ok is false and every segment takes the scalar path
@pytest.mark.parametrize("ldc", [264, 268, 272])
def test_rowmajor_batched_strided(model, ldc):
    batch, N, K = 3, 260, 128
    lda = K + 8
    a_bs = M * lda + 16
    c_bs = M * ldc + 3 * ldc
    rng = np.random.default_rng(ldc)
    A, W, b = operands(rng, batch, M, N, K, a_scale=0.5, w_scale=0.2)
    Abuf = strided(A, lda, a_bs, fill=7.0)
    r_own = h16(rng.standard_normal((batch, M, N)))
    ldr, r_bs = ldc, M * ldc + 8
    Rown = strided(r_own, ldr, r_bs, fill=3.0)
    Rshared = strided(r_own[:1], ldr, 0, fill=3.0)
    cview = lambda buf: gr.view3(buf, 0, batch, c_bs, M, ldc, N)      # noqa: E731
    for what, act, res, rbuf, rbs in (("bias", 0, None, None, 0), ("bias+gelu", 1, None, None, 0),
                                      ("bias+res", 0, r_own, Rown, r_bs),
                                      ("bias+shared res", 0, np.broadcast_to(r_own[:1], r_own.shape), Rshared, 0)):
        C = gr.sentinel_buffer(batch * c_bs + TAIL)
        gemm_ok(model, Abuf, lda, a_bs, W, b, C, ldc, c_bs, N, K, batch, res=rbuf, ldr=ldr, r_bs=rbs, act=act)
        out = cview(C).copy()
        check_sentinel(C, cview)
        check_fp64(out, gr.gemm64(A, W, b, act, res), act or res is not None, f"ldc={ldc} {what}")
        for z in range(batch):
            one = gemm_one(model, A[z], W, b, res[z] if res is not None else None, act)
            assert np.array_equal(out[z], one), f"ldc={ldc} {what}: chunk {z} differs from the contiguous launch"


def test_conv2_form_overlapping_rows(model):
    """conv2: A is a channel-last image [2M + 2][d], output row m reads image rows 2m .. 2m + 2 (lda = 2 d, K = 3 d),
    GELU, one positional block shared by the chunks"""
    d, batch = 64, 2
    N, K, lda = d, 3 * d, 2 * d
    a_bs = (2 * M + 2) * d
    c_bs = M * N + 64
    rng = np.random.default_rng(11)
    img = h16(0.5 * rng.standard_normal((batch, 2 * M + 2, d)) * (1.0 + np.arange(2 * M + 2)[None, :, None] / (2 * M)))
    _, W, b = operands(rng, 1, 1, N, K, w_scale=0.2)
    pos = h16(rng.standard_normal((1, M, N)))
    Abuf = np.ascontiguousarray(img.reshape(-1))
    A = gr.view3(Abuf, 0, batch, a_bs, M, lda, K)              # the overlapping rows
    assert np.array_equal(A[1, 5, d:2 * d], img[1, 11])
    C = gr.sentinel_buffer(batch * c_bs + TAIL)
    gemm_ok(model, Abuf, lda, a_bs, W, b, C, N, c_bs, N, K, batch, res=pos, ldr=N, r_bs=0, act=1)
    cview = lambda buf: gr.view3(buf, 0, batch, c_bs, M, N, N)      # noqa: E731
    out = cview(C).copy()
    check_sentinel(C, cview)
    check_fp64(out, gr.gemm64(A, W, b, 1, pos), True, "conv2 form")
    for z in range(batch):
        assert np.array_equal(out[z], gemm_one(model, np.ascontiguousarray(A[z]), W, b, pos[0], 1)), z


def test_conv1_form_padded_image(model):
    """conv1: the output goes one row into a zero-padded image of M + 2 rows per chunk; rows 0 and M + 1 are the
    padding conv2 reads and must not be touched"""
    batch, N, K = 3, 64, 128
    ldc = N
    c_bs = (M + 2) * ldc
    rng = np.random.default_rng(12)
    A, W, b = operands(rng, batch, M, N, K, a_scale=0.5, w_scale=0.2)
    C = gr.sentinel_buffer(batch * c_bs + TAIL)
    gemm_ok(model, A, K, M * K, W, b, C, ldc, c_bs, N, K, batch, c_off=ldc, act=1)
    cview = lambda buf: gr.view3(buf, ldc, batch, c_bs, M, ldc, N)      # noqa: E731
    out = cview(C).copy()
    check_sentinel(C, cview)
    image = gr.view3(C, 0, batch, c_bs, M + 2, ldc, N)
    assert (image[:, 0] == SENTINEL).all() and (image[:, M + 1] == SENTINEL).all()
    check_fp64(out, gr.gemm64(A, W, b, 1), True, "conv1 form")
    for z in range(batch):
        assert np.array_equal(out[z], gemm_one(model, A[z], W, b, None, 1)), z


@pytest.mark.parametrize("ldc", [304, 310])     # 304: staged epilogue, partial last 16-byte chunk; 310: direct stores
def test_transposed_batched(model, ldc):
    L, lib = _lib()
    batch, N, K = 3, 200, 128
    c_bs = N * ldc + 2 * ldc
    rng = np.random.default_rng(ldc)
    A, W, b = operands(rng, batch, M, N, K)
    cview = lambda buf: gr.view3(buf, 0, batch, c_bs, N, ldc, M)      # noqa: E731
    out = {}
    try:
        for knob in (0, 1):
            L.check(lib.fw_test_knob(5, knob))
            C = gr.sentinel_buffer(batch * c_bs + TAIL)
            gemm_ok(model, A, K, M * K, W, b, C, ldc, c_bs, N, K, batch, trans=1)
            out[knob] = cview(C).copy()
            check_sentinel(C, cview)
            assert (gr.view3(C, M, batch, c_bs, N, ldc, ldc - M) == SENTINEL).all()     # columns [M, ldc)
    finally:
        L.check(lib.fw_test_knob(5, 1))
    assert np.array_equal(out[0], out[1])
    check_fp64(out[1], gr.gemm64(A, W, b).transpose(0, 2, 1), False, f"V^T ldc={ldc}")
    for z in range(batch):
        assert np.array_equal(out[1][z], gemm_one(model, A[z], W, b, None, 2)), z


# ------------------------------------------------------------------------------------------------------------------
# B. tile order: two bands with a short last band (tests/test_gemm_refs.py pins the rule's figures)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,batch", [(260, 9), (516, 7), (1028, 4), (1540, 3)])
def test_blocked_tile_order_two_bands(model, N, batch):
    L, lib = _lib()
    K = 64
    bn, bm, last, grid = gr.tile_order(M, N, batch)
    assert 0 < last < bm and 2 * batch > bm and grid == 2 * batch * -(-N // 256)
    ldc = N + 4                                                # a multiple of 8 at all four widths; one gap row per chunk
    c_bs = M * ldc + ldc
    rng = np.random.default_rng(N)
    A, W, b = operands(rng, batch, M, N, K)
    cview = lambda buf: gr.view3(buf, 0, batch, c_bs, M, ldc, N)      # noqa: E731
    out = {}
    try:
        for order in (0, 1):
            L.check(lib.fw_test_knob(1, order))
            C = gr.sentinel_buffer(batch * c_bs + TAIL)
            gemm_ok(model, A, K, M * K, W, b, C, ldc, c_bs, N, K, batch)
            out[order] = cview(C).copy()
            check_sentinel(C, cview)
    finally:
        L.check(lib.fw_test_knob(1, 1))
    check_fp64(out[1], gr.gemm64(A, W, b), False, f"blocked {bn}x{bm}, grid {grid}")
    assert np.array_equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------------------------
# C. layered cross-K / V^T
# ------------------------------------------------------------------------------------------------------------------
def frag_index(vt, kvp, N):
    L, lib = _lib()
    idx = np.empty((kvp, N), np.int64)
    L.check(lib.fw_test_cross_kv_frag_index(int(vt), kvp, N, L.ptr(idx)))
    return idx


def check_frag_output(C, idx, bases, vt, refs, what, tol):
    """C: the raw buffer; bases / refs: start and [M][N] reference of every fragment-major block.  Real keys against
    the reference; K's padded keys keep the sentinel, V^T's are the sentinel or 0; nothing else is written."""
    written = np.zeros(C.size, bool)
    worst = 0.0
    for base, ref in zip(bases, refs):
        blk = C[base + idx]                                    # [kvp][N]
        worst = max(worst, rel_err(blk[:M], ref))
        pad = blk[M:]
        if vt:
            assert ((pad == SENTINEL) | (pad == 0.0)).all(), what
        else:
            assert (pad == SENTINEL).all(), what
        written[base + idx.reshape(-1)] = True
    print(f"{what}: rel err {worst:.2e}")
    assert worst < tol, what
    assert written[-TAIL:].sum() == 0 and (C[~written] == SENTINEL).all(), what


@pytest.mark.parametrize("vt", [0, 1])
def test_layered_cross_kv(model, vt):
    n_layers, N, K, batch, kvp = 5, 320, 128, 4, 320
    assert gr.tile_order(M, N, batch, n_layers)[:3] == (5, 6, 2)     # blocks straddle the 2-tile layers; bands 6 + 2
    c_bs = N * kvp
    c_ls = 6 * c_bs                                            # two spare slots per layer
    rng = np.random.default_rng(40 + vt)
    A, W, b = operands(rng, batch, M, N, K, n_layers=n_layers)
    idx = frag_index(vt, kvp, N)
    ldc = kvp if vt else N
    C = gr.sentinel_buffer(n_layers * c_ls + TAIL)
    gemm_ok(model, A, K, M * K, W, b, C, ldc, c_bs, N, K, batch, c_ls=c_ls, n_layers=n_layers, trans=vt, head_rows=kvp)
    bases = [l * c_ls + z * c_bs for l in range(n_layers) for z in range(batch)]
    refs = [gr.gemm64(A[z], W[l], b[l]) for l in range(n_layers) for z in range(batch)]
    check_frag_output(C, idx, bases, vt, refs, f"layered cross-{'V^T' if vt else 'K'}", 2e-3)
    C1 = gr.sentinel_buffer(C.size)
    for l in range(n_layers):
        gemm_ok(model, A, K, M * K, W[l], b[l], C1, ldc, c_bs, N, K, batch, c_off=l * c_ls, trans=vt, head_rows=kvp)
    assert np.array_equal(C, C1), "the layered launch differs from five per-layer launches"


# ------------------------------------------------------------------------------------------------------------------
# D. int8 forms
# ------------------------------------------------------------------------------------------------------------------
def quant_rows_dev(model, x, ldx=None, ln=None, frag=0):
    L, lib = _lib()
    rows, d = x.shape
    ldx = ldx or d
    xb = strided(x[None], ldx, 0, fill=9.0)
    g, b = (_f32(ln[0]), _f32(ln[1])) if ln is not None else (None, None)
    q = np.full((rows, d), 99, np.int8)
    s = np.full(rows, -1.0, np.float32)
    L.check(lib.fw_test_quant_rows(model._replicas[0].handle, _p(xb), rows, d, ldx, _p(g), _p(b), frag, _p(q), _p(s)))
    return q.astype(np.int64), s


def i8_operands(K, N, batch=2):
    rng = np.random.default_rng(K + N)
    A = h16(rng.standard_normal((batch, M, K)) * (1.0 + np.arange(M)[None, :, None] / M))
    A[0, 5] = 0.0                                              # an all-zero row: scale 1, codes 0
    W = h16(rng.standard_normal((N, K)) * (0.2 + np.arange(N)[:, None] / N))
    b = h16(rng.standard_normal(N))
    r = h16(rng.standard_normal((batch, M, N)))
    return A, W, b, r


@pytest.mark.parametrize("K", [128, 256])
def test_int8_rowmajor_forms(kmodel, K):
    """bias + GELU, bias + residual and the LayerNorm-fused quantiser in front, batch = 2, against the exact integer
    product of the codes and scales (LayerNorm form: the codes of fw_test_quant_rows on the same rows, so that a
    one-ulp LayerNorm difference cannot enter)"""
    batch, N, ldc = 2, 260, 272
    c_bs = M * ldc + 3 * ldc
    A, W, b, r = i8_operands(K, N)
    wq, w_s = gr.quant_rows32(W)
    aq, a_s = gr.quant_rows32(A)
    rng = np.random.default_rng(K)
    ln = (h16(1 + 0.1 * rng.standard_normal(K)), h16(0.1 * rng.standard_normal(K)))
    lq, l_s = quant_rows_dev(kmodel, A.reshape(-1, K), ln=ln)
    lq, l_s = lq.reshape(batch, M, K), l_s.reshape(batch, M)
    Rbuf = strided(r, ldc, c_bs)
    cview = lambda buf: gr.view3(buf, 0, batch, c_bs, M, ldc, N)      # noqa: E731
    for what, act, res, lnp, (q, s) in (("bias+gelu", 1, None, None, (aq, a_s)), ("bias+res", 0, r, None, (aq, a_s)),
                                        ("layernorm+bias+gelu", 1, None, ln, (lq, l_s))):
        C = gr.sentinel_buffer(batch * c_bs + TAIL)
        gemm_ok(kmodel, A, K, M * K, W, b, C, ldc, c_bs, N, K, batch, res=Rbuf if res is not None else None, ldr=ldc,
                r_bs=c_bs, act=act, int8=1, ln=lnp)
        out = cview(C).copy()
        check_sentinel(C, cview)
        ref = h16(gr.int8_linear32(q, s, wq, w_s, b, act, res))
        err = rel_err(out, ref)
        print(f"int8 K={K} {what}: rel err vs integer reference {err:.2e}")
        assert err < 1e-3, what


@pytest.mark.parametrize("K", [128, 256])
def test_int8_transposed_and_fragment_major(kmodel, K):
    batch = 2
    # transposed, ldc = 304 (the int8 instantiation keeps the direct stores)
    N, ldc = 260, 304
    c_bs = N * ldc + 2 * ldc
    A, W, b, _ = i8_operands(K, N)
    aq, a_s = gr.quant_rows32(A)
    wq, w_s = gr.quant_rows32(W)
    C = gr.sentinel_buffer(batch * c_bs + TAIL)
    gemm_ok(kmodel, A, K, M * K, W, b, C, ldc, c_bs, N, K, batch, trans=1, int8=1)
    cview = lambda buf: gr.view3(buf, 0, batch, c_bs, N, ldc, M)      # noqa: E731
    out = cview(C).copy()
    check_sentinel(C, cview)
    ref = h16(gr.int8_linear32(aq, a_s, wq, w_s, b)).transpose(0, 2, 1)
    err = rel_err(out, ref)
    print(f"int8 K={K} transposed: rel err {err:.2e}")
    assert err < 1e-3
    # fragment-major K / V^T
    N = kvp = 320
    c_bs = N * kvp + 128
    A, W, b, _ = i8_operands(K, N)
    aq, a_s = gr.quant_rows32(A)
    wq, w_s = gr.quant_rows32(W)
    ref = h16(gr.int8_linear32(aq, a_s, wq, w_s, b))
    for vt in (0, 1):
        C = gr.sentinel_buffer(batch * c_bs + TAIL)
        gemm_ok(kmodel, A, K, M * K, W, b, C, kvp if vt else N, c_bs, N, K, batch, trans=vt, head_rows=kvp, int8=1)
        check_frag_output(C, frag_index(vt, kvp, N), [z * c_bs for z in range(batch)], vt, list(ref),
                          f"int8 K={K} cross-{'V^T' if vt else 'K'}", 1e-3)


# ------------------------------------------------------------------------------------------------------------------
# E. one rounding, exactly
# ------------------------------------------------------------------------------------------------------------------
def dec_linear(model, x, W, bias=None, res=None, act=0, variant=0):
    L, lib = _lib()
    R, K = x.shape
    N = W.shape[0]
    out = np.empty((R, N), np.float32)
    out_frag = np.empty((R, N), np.float32)
    keep = [_f32(a) for a in (x, W, bias, None, None, res)]
    L.check(lib.fw_test_dec_linear(model._replicas[0].handle, *[_p(a) for a in keep], R, N, K, act, variant, _p(out),
                                   _p(out_frag)))
    return out, out_frag


def assert_bits(out, want, what):
    bad = np.argwhere(out != want)
    assert bad.size == 0, (f"{what}: {len(bad)} of {out.size} elements differ from fp16(f32(f32(a w) + b) + r), first "
                           f"{[(tuple(i), float(out[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]}")


@pytest.mark.parametrize("K", [64, 128])
def test_one_rounding_encoder_gemm(model, K):
    """y = fp16(act(acc + bias) + res) with ONE rounding: with a single nonzero per A row the accumulator is one exact
    product, and the result must equal the IEEE float32 emulation bit for bit (tests/test_gemm_refs.py shows that a
    second rounding before the residual changes 20 % of these elements)"""
    N = 260
    rng = np.random.default_rng(M + N + K)
    A, a, W, b, r = gr.one_hot_operands(rng, M, N, K)
    assert_bits(gemm_one(model, A, W, b, r), gr.one_rounding(a, W, K, b, r), f"row-major K={K}")
    assert_bits(gemm_one(model, A, W, b, None, act=2), gr.one_rounding(a, W, K, b).T, f"transposed K={K}")
    # the batched, strided form: two chunks (the second negated, with the residual rows reversed)
    batch, lda, ldc = 2, K + 8, 272
    a_bs, c_bs = M * lda + 16, M * ldc + 3 * ldc
    A2 = np.stack([A, -A])
    r2 = np.stack([r, r[::-1]])
    C = gr.sentinel_buffer(batch * c_bs + TAIL)
    gemm_ok(model, strided(A2, lda, a_bs), lda, a_bs, W, b, C, ldc, c_bs, N, K, batch, res=strided(r2, ldc, c_bs),
            ldr=ldc, r_bs=c_bs)
    cview = lambda buf: gr.view3(buf, 0, batch, c_bs, M, ldc, N)      # noqa: E731
    out = cview(C).copy()
    check_sentinel(C, cview)
    assert_bits(out[0], gr.one_rounding(a, W, K, b, r2[0]), f"batched chunk 0 K={K}")
    assert_bits(out[1], gr.one_rounding(-a, W, K, b, r2[1]), f"batched chunk 1 K={K}")


# workgroup shapes of dec_gemm_big_kernel (variant 10 + cfg) whose k-steps per stage do not fit K = 128 = 4 k-steps
# (dec_kernels.hip: dec_linear_plan): the launcher refuses them; at K = 256 all three run
BIG_REFUSED = {128: (10, 11), 256: ()}


def dec_linear_variants(model, K, variants, *a, **k):
    """(variant, out, out_frag) of every variant that exists at this K; a refusal anywhere else is an error"""
    for variant in variants:
        if variant in BIG_REFUSED[K]:
            with pytest.raises(RuntimeError):
                dec_linear(model, *a, variant=variant, **k)
            continue
        yield (variant,) + dec_linear(model, *a, variant=variant, **k)


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("R", [80, 333])
def test_one_rounding_decoder_linear(model, R, K):
    N = 256
    rng = np.random.default_rng(R + N + K)
    A, a, W, b, r = gr.one_hot_operands(rng, R, N, K)
    want = gr.one_rounding(a, W, K, b, r)
    for variant, out, out_frag in dec_linear_variants(model, K, (0, 5, 6, 7, 10, 11, 12), A, W, b, r):
        assert_bits(out, want, f"decoder linear R={R} K={K} variant {variant}")
        assert_bits(out_frag, want, f"decoder linear R={R} K={K} variant {variant}, fragment-major copy")


# ------------------------------------------------------------------------------------------------------------------
# F. GELU over every fp16 input
# ------------------------------------------------------------------------------------------------------------------
def check_gelu(out, x, what):
    """out, x [128][512]: out = gelu(x) from the device.  Bound: gemm_refs.gelu_bound, c = 6.4 = 4 x the 1.6 measured
    for the float32 evaluation of the same formula (tests/test_gemm_refs.py)."""
    g = gr.gelu64(x)
    err = np.abs(out.astype(np.float64) - g)
    bad = err > gr.gelu_bound(x)
    print(f"{what}: worst error {float((err / gr.ulp16(g)).max()):.3f} fp16 ulps of the result, "
          f"{float((err / gr.gelu_bound(x)).max()):.3f} of the bound; {int(bad.sum())} inputs outside")
    if bad.any() and (np.abs(g[bad]) < 2.0 ** -14).all():
        pytest.fail(f"{what}: {int(bad.sum())} results differ, ALL of them fp16-subnormal: the device flushes "
                    f"subnormal results (inputs {x[bad][:8]})")
    assert not bad.any(), (what, x[bad][:8], out[bad][:8], g[bad][:8])


def test_gelu_every_fp16_input_encoder_gemm(model):
    x = gr.all_normal_fp16()
    W = x.reshape(512, 128)
    out = gemm_one(model, np.eye(128, dtype=np.float32), W, act=1)         # out[m][n] = gelu(W[n][m])
    check_gelu(out, W.T, "encoder GEMM epilogue")


@pytest.mark.parametrize("K", [128, 256])      # 256: x = [I | 0], W = [patterns | 0], the K at which every shape runs
def test_gelu_every_fp16_input_decoder_linear(model, K):
    W = np.zeros((512, K), np.float32)
    W[:, :128] = gr.all_normal_fp16().reshape(512, 128)
    x = np.eye(128, K, dtype=np.float32)
    for variant, out, out_frag in dec_linear_variants(model, K, (5, 10, 11, 12), x, W, act=1):
        check_gelu(out, W[:, :128].T, f"decoder linear K={K} variant {variant}")
        assert np.array_equal(out, out_frag)


# ------------------------------------------------------------------------------------------------------------------
# G. row kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 1536, 1600, 5120])        # 1600: the first d on the QR_MAXC path
def test_quant_rows_plain(kmodel, d):
    rows = 37
    rng = np.random.default_rng(d)
    x = h16(rng.standard_normal((rows, d)) * (0.1 + np.arange(rows)[:, None]))
    x[11] = 0.0
    q_ref, s_ref = gr.quant_rows32(x)
    for ldx in (d, d + 8):
        q0, s0 = quant_rows_dev(kmodel, x, ldx=ldx, frag=0)
        q1, s1 = quant_rows_dev(kmodel, x, ldx=ldx, frag=1)
        assert np.array_equal(s0.view(np.uint32), s_ref.view(np.uint32)), (d, ldx)
        assert np.array_equal(q0, q_ref), (d, ldx, int((q0 != q_ref).sum()))
        assert np.array_equal(q1, q0) and np.array_equal(s1, s0), (d, ldx, "fragment-major")
    assert s_ref[11] == 1.0 and not q_ref[11].any()


@pytest.mark.parametrize("d", [128, 384, 1280, 1536])
def test_quant_rows_layernorm(kmodel, d):
    """y = LayerNorm in fp64.  The device rounds its float32 LayerNorm to fp16 (<= ulp16(y) / 2 + the float32 error),
    takes s = max |y| / 127 and q = rint(y / s) (<= s / 2, about 1.6e-2 here).  The last term of the bound,
    4e-3 * 2^-10 |y| = 3.9e-6 |y|, is the float32 slack: numpy's float32 LayerNorm is within 6.6e-7 of fp64 at these
    shapes (printed below; |y| reaches 4.5), and y * (127 / max) rounds with 2^-23 relative error (1.2e-7 |y|)."""
    rows = 37
    rng = np.random.default_rng(d)
    x = h16(rng.standard_normal((rows, d)) * 3 + 1)
    x[20] = h16(x[20] * 8)
    g = h16(1 + 0.1 * rng.standard_normal(d))
    b = h16(0.1 * rng.standard_normal(d))
    y = gr.layernorm64(x, g, b)
    f32_err = np.abs(gr.layernorm32(x, g, b).astype(np.float64) - y)
    print(f"d={d}: numpy float32 LayerNorm error max {f32_err.max():.2e}, max |y| {np.abs(y).max():.2f}")
    amax = np.abs(y).max(-1)
    for frag in (0, 1):
        q, s = quant_rows_dev(kmodel, x, ln=(g, b), frag=frag)
        s = s.astype(np.float64)
        assert (np.abs(q) <= 127).all()
        assert (np.abs(s - amax / 127) <= gr.ulp16(amax) / 127).all(), (d, frag)
        err = np.abs(q * s[:, None] - y)
        bound = s[:, None] / 2 + gr.ulp16(y) / 2 + 4e-3 * 2.0 ** -10 * np.abs(y)
        print(f"d={d} frag={frag}: worst |q s - y| / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all(), (d, frag, np.argwhere(err > bound)[:4])
        if frag == 0:
            q0, s0 = q, s
    assert np.array_equal(q, q0) and np.array_equal(s, s0)


@pytest.mark.parametrize("rows", [5, 37])
@pytest.mark.parametrize("d", [128, 1536])
def test_layernorm_fragment_major(model, rows, d):
    """the fragment-major LayerNorm output (what the decoder linears read) holds the bits of the row-major one; the
    last 16-row tile is partial"""
    L, lib = _lib()
    rng = np.random.default_rng(rows + d)
    x = h16(rng.standard_normal((rows, d)) * 3 + 1)
    g = h16(1 + 0.1 * rng.standard_normal(d))
    b = h16(0.1 * rng.standard_normal(d))
    out = {}
    for frag in (0, 1):
        out[frag] = np.empty_like(x)
        L.check(lib.fw_test_layernorm_frag(model._replicas[0].handle, _p(x), _p(g), _p(b), rows, d, frag, _p(out[frag])))
    assert np.abs(out[0] - gr.layernorm64(x, g, b)).max() < 4e-3
    assert np.array_equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------------------------
# the hook's own bounds check
# ------------------------------------------------------------------------------------------------------------------
def test_gemm_ex_refuses_a_description_outside_its_buffers(model):
    """a buffer one element shorter than the furthest element the launch touches: FW_EINVAL, nothing launched (the
    output keeps the sentinel); the exact fit of the read-only buffers runs"""
    L, _ = _lib()
    batch, N, K, lda, ldc = 2, 260, 64, 72, 264
    a_bs, c_bs = M * lda + 16, M * ldc + 8
    rng = np.random.default_rng(3)
    A, W, b = operands(rng, batch, M, N, K)
    r = h16(rng.standard_normal((batch, M, N)))
    Abuf, Rbuf = strided(A, lda, a_bs), strided(r, ldc, c_bs)          # exact fits: no tail
    a_need = a_bs + (M - 1) * lda + K
    r_need = c_need = c_bs + (M - 1) * ldc + N
    assert Abuf.size == a_need and Rbuf.size == r_need
    common = dict(res=Rbuf, ldr=ldc, r_bs=c_bs)
    for short in ("a", "r", "c", "c_off", "trans", "frag"):
        C = gr.sentinel_buffer(2 * 320 * 320 + TAIL)          # (no described c_elems exceeds the real buffer)
        kw = dict(common)
        if short == "a":
            kw["a_elems"] = a_need - 1
        elif short == "r":
            kw["r_elems"] = r_need - 1
        elif short == "c":
            kw["c_elems"] = c_need - 1
        elif short == "c_off":
            kw.update(c_off=8, c_elems=c_need + 7)
        elif short == "trans":
            kw = dict(trans=1, c_elems=c_bs + (N - 1) * ldc + M - 1)
        else:       # fragment-major: a chunk's block of [N / 64][320 * 64] halves, the last key group written whole
            kw = dict(trans=0, head_rows=320, c_elems=320 * 320 + 4 * 320 * 64 + 10 * 2048 - 1)
        n = 320 if short == "frag" else N
        w = np.zeros((n, K), np.float32) if short == "frag" else W
        rc = gemm_ex(model, Abuf, lda, a_bs, w, None if short == "frag" else b, C, ldc if short != "frag" else n,
                     c_bs if short != "frag" else 320 * 320, n, K, batch, **kw)
        assert rc == L.FW_EINVAL, (short, rc)
        assert (C == SENTINEL).all(), short
    C = gr.sentinel_buffer(c_need + TAIL)
    assert gemm_ex(model, Abuf, lda, a_bs, W, b, C, ldc, c_bs, N, K, batch, **common) == L.FW_OK
    out = gr.view3(C, 0, batch, c_bs, M, ldc, N)
    assert rel_err(out, gr.gemm64(A, W, b, 0, r)) < 2e-3
    # strides the epilogue's 16-byte stores could not start from
    assert gemm_ex(model, Abuf, lda, a_bs, W, b, C, ldc, c_bs, N, K, batch, c_off=4) == L.FW_EINVAL
    with pytest.raises(ValueError):
        L.check(gemm_ex(model, Abuf, lda, a_bs, W, b, C, ldc, c_bs, N, K, batch, a_elems=a_need - 1))
