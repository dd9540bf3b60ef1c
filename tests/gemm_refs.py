"""numpy helpers of tests/test_gpu_gemm_forms.py and tests/test_gemm_refs.py: strided views of the flat buffers
fw_test_gemm_ex takes, float32 emulations of the encoder GEMM's epilogue arithmetic, fp16 spacing, the exact-erf GELU
and the tile-order rule of launch_gemm (gemm.hip), restated.  No GPU here."""
import math

import numpy as np
from numpy.lib.stride_tricks import as_strided

SENTINEL = -1234.0          # exact in fp16; what every output buffer holds before a launch
TILE = 256                  # gemm.hip: GB_M = GB_N


def h16(x):
    """round to fp16, keep float32 (what the engine stores)"""
    return np.asarray(x).astype(np.float16).astype(np.float32)


def ulp16(g):
    """fp16 spacing at |g|: 2^(floor(log2 |g|) - 10), and 2^-24 (the subnormal spacing) below 2^-14"""
    g = np.abs(np.asarray(g, np.float64))
    _, e = np.frexp(g)                                          # |g| = m 2^e, m in [0.5, 1); frexp(0) = (0, 0)
    return np.ldexp(1.0, np.where(g > 0, np.maximum(e - 11, -24), -24))


# ---- strided views -----------------------------------------------------------------------------------------------
def view3(buf, off, n0, s0, n1, s1, n2):
    """buf[off + i * s0 + j * s1 + k], (i, j, k) < (n0, n1, n2): a view of a flat array (rows may overlap)"""
    last = off + (n0 - 1) * s0 + (n1 - 1) * s1 + n2 - 1
    assert buf.ndim == 1 and off >= 0 and last < buf.size, (off, last, buf.size)
    it = buf.itemsize
    return as_strided(buf[off:], shape=(n0, n1, n2), strides=(s0 * it, s1 * it, it), writeable=True)


def sentinel_buffer(n):
    return np.full(n, SENTINEL, np.float32)


def untouched(buf, *views):
    """mask of the elements of `buf` no view covers, computed by writing through the views into a copy of zeros"""
    mark = np.zeros(buf.size, np.float32)
    for mk in views:
        mk(mark)[...] = 1.0
    return mark == 0.0


# ---- references --------------------------------------------------------------------------------------------------
def gelu64(x):
    from scipy.special import erf
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def gelu32(x):
    """the kernels' formula (common.h: gelu_erf) in numpy float32"""
    from scipy.special import erf
    x = np.asarray(x, np.float32)
    er = erf(x * np.float32(0.70710678118654752440)).astype(np.float32)
    return (np.float32(0.5) * x) * (np.float32(1.0) + er)


def gelu_tanh64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def all_normal_fp16():
    """all 65 536 fp16 bit patterns as float32 [65536]; non-finite and subnormal patterns replaced by 0"""
    x = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
    ok = np.isfinite(x) & (np.abs(x) >= 2.0 ** -14)
    return np.where(ok, x, np.float32(0.0))


def gelu_f32_constant():
    """max |gelu32 - gelu64| / (2^-24 max(1, |x|)) over every normal fp16 x: the float32 evaluation error of the
    formula, in units of the bound's second term"""
    x = all_normal_fp16()
    return float((np.abs(gelu32(x).astype(np.float64) - gelu64(x)) / (2.0 ** -24 * np.maximum(1.0, np.abs(x)))).max())


# 4 x the value gelu_f32_constant() measures (1.6 on numpy / scipy float32): device erff may differ from scipy's by a
# few ulps.  tests/test_gemm_refs.py holds the measurement to this constant.
GELU_C = 6.4


def gelu_bound(x):
    """|out - gelu64(x)| <= 0.5 ulp16(g) + GELU_C 2^-24 max(1, |x|): one fp16 rounding of a float32 evaluation"""
    g = gelu64(x)
    return 0.5 * ulp16(g) + GELU_C * 2.0 ** -24 * np.maximum(1.0, np.abs(np.asarray(x, np.float64)))


def gemm64(A, W, bias=None, act=0, res=None):
    """fp64 y = act(A W^T + bias) + res on [..., M, K] x [N, K]"""
    y = np.asarray(A, np.float64) @ np.asarray(W, np.float64).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if act:
        y = gelu64(y)
    if res is not None:
        y = y + np.asarray(res, np.float64)
    return y


def quant_rows32(x):
    """float32 emulation of the row quantiser (the one of tests/test_gpu_int8.py): codes int64, scales float32"""
    amax = np.abs(x).max(axis=-1).astype(np.float32)
    inv = np.where(amax > 0, np.float32(127.0) / np.where(amax > 0, amax, 1), 0).astype(np.float32)
    ds = np.where(amax > 0, amax / np.float32(127.0), 1).astype(np.float32)
    q = np.rint(x.astype(np.float32) * inv[..., None]).astype(np.int64)
    return q, ds


def int8_linear32(aq, a_s, wq, w_s, bias=None, act=0, res=None):
    """the int8 GEMM's epilogue in float32 on exact integer sums: ((acc * a_s) * w_s + bias -> act) + res, unrounded"""
    acc = (aq @ wq.T).astype(np.float32)
    y = acc * a_s[..., :, None].astype(np.float32) * w_s[None, :].astype(np.float32)
    if bias is not None:
        y = y + bias.astype(np.float32)
    if act:
        y = gelu32(y)
    if res is not None:
        y = y + res.astype(np.float32)
    return y


def layernorm64(x, g, b):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def layernorm32(x, g, b):
    x = np.asarray(x, np.float32)
    d = np.float32(x.shape[-1])
    mu = x.sum(-1, keepdims=True, dtype=np.float32) / d
    var = ((x - mu) ** 2).sum(-1, keepdims=True, dtype=np.float32) / d
    return (x - mu) * (np.float32(1.0) / np.sqrt(var + np.float32(1e-5))) * np.asarray(g, np.float32) + np.asarray(b, np.float32)


# ---- the one-rounding contract -----------------------------------------------------------------------------------
def one_hot_operands(rng, M, N, K):
    """A [M][K] with a single nonzero per row (column m % K), W [N][K], bias [N], res [M][N]: fp16 values with
    magnitudes in [2^-10, 8] (no fp16 subnormal reaches the matrix unit) and random signs.  The accumulator of
    (m, n) is then the ONE exact product a[m] * W[n][m % K] (11 + 11 significand bits fit float32)."""
    def vals(shape):
        mag = np.exp2(rng.uniform(-10.0, 3.0, shape))
        v = h16(mag * rng.choice([-1.0, 1.0], shape))
        return np.clip(np.abs(v), 2.0 ** -10, 8.0).astype(np.float32) * np.sign(v).astype(np.float32)
    a = vals(M)
    A = np.zeros((M, K), np.float32)
    A[np.arange(M), np.arange(M) % K] = a
    return A, a, vals((N, K)), vals(N), vals((M, N))


def one_rounding(a, W, K, bias=None, res=None):
    """f16(f32(f32(a w) + b) + r): the contract y = fp16(act(acc + bias) + res) with act = identity, IEEE float32"""
    M = a.shape[0]
    v = a.astype(np.float32)[:, None] * W[:, np.arange(M) % K].T.astype(np.float32)      # exact
    if bias is not None:
        v = v + bias.astype(np.float32)
    if res is not None:
        v = v + res.astype(np.float32)
    return h16(v)


def two_roundings(a, W, K, bias=None, res=None):
    """the defect the contract excludes: rounded to fp16 BEFORE the residual is added"""
    M = a.shape[0]
    v = a.astype(np.float32)[:, None] * W[:, np.arange(M) % K].T.astype(np.float32)
    if bias is not None:
        v = v + bias.astype(np.float32)
    v = h16(v)
    if res is not None:
        v = v + res.astype(np.float32)
    return h16(v)


# ---- launch_gemm's tile order, restated --------------------------------------------------------------------------
def tile_order(M, N, batch, n_layers=1):
    """(blk_n, blk_m, panels in the last band, grid) of the blocked tile order for a launch (gemm.hip: launch_gemm)"""
    nMt, nNt = -(-M // TILE), -(-N // TILE) * n_layers
    n_mp = nMt * batch
    bn, best = 1, 1 << 30
    for c in range(1, min(nNt, 16) + 1):
        if nNt % c:
            continue
        cost = c + (32 + c - 1) // c
        if cost <= best:
            best, bn = cost, c
    bm = max(32 // bn, 1)
    last = n_mp - (n_mp - 1) // bm * bm
    return bn, bm, last, n_mp * nNt
