"""The references of tests/test_gpu_gemm_forms.py, checked on the CPU: each of its bit-level and bound checks must
tell the defect it is aimed at from the contract, and the constants it relies on are measured here."""
import numpy as np

import gemm_refs as gr


def test_one_rounding_check_discriminates():
    """the inputs of the one-rounding test separate y = fp16(acc + bias + res) from the form that rounds to fp16
    before the residual is added: at least 10 % of the elements differ (measured 23 % on N(0, 1) operands; the
    log-uniform magnitudes used here give more, printed below)"""
    for M, N, K in ((300, 260, 64), (300, 260, 128), (80, 256, 128), (333, 256, 128)):
        rng = np.random.default_rng(M + N + K)
        A, a, W, b, r = gr.one_hot_operands(rng, M, N, K)
        for x in (a, W, b, r):
            assert (np.abs(x) >= 2.0 ** -10).all() and (np.abs(x) <= 8.0).all() and np.array_equal(x, gr.h16(x))
        assert (np.count_nonzero(A, axis=1) == 1).all()
        # the accumulator the matrix unit forms is the one exact product
        assert np.array_equal(A.astype(np.float64) @ W.T.astype(np.float64),
                              (a.astype(np.float64)[:, None] * W[:, np.arange(M) % K].T.astype(np.float64)))
        one, two = gr.one_rounding(a, W, K, b, r), gr.two_roundings(a, W, K, b, r)
        frac = float((one != two).mean())
        print(f"{M}x{N}x{K}: a second rounding changes {100 * frac:.1f} % of the elements")
        assert frac >= 0.10


def test_gelu_bound_constant_and_tanh_gelu_violates_it():
    """measures the float32 evaluation error of 0.5 x (1 + erf(x / sqrt 2)) over every normal fp16 x in units of
    2^-24 max(1, |x|) — 1.6 with numpy / scipy float32 — and holds gemm_refs.GELU_C to 4 x that value (6.4).  The exact
    GELU rounded once to fp16 meets the bound everywhere; the tanh approximation does not (up to 919 fp16 ulps off)."""
    x = gr.all_normal_fp16()
    assert x.size == 65536 and np.count_nonzero(x) == 2 * 30 * 1024
    meas = gr.gelu_f32_constant()
    print(f"float32 GELU evaluation error: {meas:.3f} x 2^-24 max(1, |x|); c = {gr.GELU_C}")
    assert meas <= gr.GELU_C / 4.0 and meas >= gr.GELU_C / 8.0       # c is 4 x the measurement, not a loose guess
    g = gr.gelu64(x)
    bound = gr.gelu_bound(x)
    assert (np.abs(gr.h16(gr.gelu32(x)).astype(np.float64) - g) <= bound).all()
    tanh_err = np.abs(gr.h16(gr.gelu_tanh64(x)).astype(np.float64) - g)
    bad = tanh_err > bound
    print(f"tanh GELU: {int(bad.sum())} inputs outside the bound, worst {float((tanh_err / gr.ulp16(g)).max()):.0f} fp16 ulps")
    assert bad.sum() > 1000 and (tanh_err / gr.ulp16(g)).max() > 100


def test_ulp16():
    for v, u in ((1.0, 2.0 ** -10), (1.999, 2.0 ** -10), (2.0, 2.0 ** -9), (0.75, 2.0 ** -11), (2.0 ** -14, 2.0 ** -24),
                 (2.0 ** -15, 2.0 ** -24), (0.0, 2.0 ** -24), (-1234.0, 1.0), (65504.0, 32.0)):
        assert gr.ulp16(v) == u, (v, gr.ulp16(v), u)
    x = np.abs(gr.all_normal_fp16()[1:0x7bff])
    nxt = np.arange(2, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)
    ok = x >= 2.0 ** -14
    assert np.array_equal(gr.ulp16(x[ok]), (nxt - x)[ok])


def test_tile_order_rule_gives_two_bands():
    """the shapes of the tile-order test: launch_gemm's rule gives blk_n x blk_m = 2x16, 3x10, 5x6, 7x4, each with a
    short last band, grids of 36, 42, 40, 42 (36 and 42: the remainder path of the XCD remap); the layered cross-K/V
    shape gives blk_n = 5 across 2-tile layers and bands of 6 + 2"""
    want = {(260, 9): (2, 16, 2, 36), (516, 7): (3, 10, 4, 42), (1028, 4): (5, 6, 2, 40), (1540, 3): (7, 4, 2, 42)}
    for (N, batch), w in want.items():
        assert gr.tile_order(300, N, batch) == w, (N, batch)
    assert gr.tile_order(300, 320, 4, n_layers=5) == (5, 6, 2, 80)


def test_cross_kv_frag_index_is_a_permutation():
    """host-only hook: the fragment-major K and V^T positions of (key, column) fill a chunk's block exactly once"""
    from faster_whisper_amd import _lib
    lib = _lib.load()
    for vt in (0, 1):
        for kvp, N in ((32, 64), (320, 320), (96, 128)):
            idx = np.full((kvp, N), -1, np.int64)
            assert lib.fw_test_cross_kv_frag_index(vt, kvp, N, _lib.ptr(idx)) == _lib.FW_OK
            assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(kvp * N))
            # a head's block is contiguous: [N / 64][kvp * 64]
            assert np.array_equal(idx // (kvp * 64), np.broadcast_to(np.arange(N) // 64, (kvp, N)))
    k = np.empty((320, 320), np.int64)
    v = np.empty((320, 320), np.int64)
    lib.fw_test_cross_kv_frag_index(0, 320, 320, _lib.ptr(k))
    lib.fw_test_cross_kv_frag_index(1, 320, 320, _lib.ptr(v))
    assert not np.array_equal(k, v)
    assert lib.fw_test_cross_kv_frag_index(0, 300, 320, _lib.ptr(k)) == _lib.FW_EINVAL
    assert lib.fw_test_cross_kv_frag_index(0, 320, 100, _lib.ptr(k)) == _lib.FW_EINVAL
