"""Host-side integer logic of the batched path (no GPU): prompt construction, suppress set,
timestamp splitting, pad_or_trim, chunk partitioning, result records.  Expected values are
worked out by hand from the reference's rules (transcribe.py:1024-1101, :1532-1565, :1884-1907)."""
import numpy as np
import pytest

from faster_whisper_amd import get_config
from faster_whisper_amd.sharding import decode_records, encode_records, partition
from faster_whisper_amd.transcribe import (Tokenizer, WhisperModel, get_compression_ratio, get_suppressed_tokens,
                                           pad_or_trim)


def _bare_model(cfg):
    m = WhisperModel.__new__(WhisperModel)
    m.max_length = 448
    m.time_precision = 0.02
    m.input_stride = 2
    m.frames_per_second = 100
    m.tokens_per_second = 50
    return m


def test_tokenizer_special_ids_and_sot_sequence():
    v3 = get_config("large-v3")
    tok = Tokenizer(None, v3, True, task="transcribe", language="fr")
    assert tok.sot_sequence == [50258, 50259 + 6, 50360]   # fr is the 7th language of the vocabulary
    assert tok.timestamp_begin == 50365 and tok.no_timestamps == 50364
    en = get_config("tiny.en")
    tok_en = Tokenizer(None, en, False)
    assert tok_en.sot_sequence == [50257]
    with pytest.raises(ValueError):
        Tokenizer(None, v3, True, task="nope", language="en")
    with pytest.raises(ValueError):
        Tokenizer(None, v3, True, task="transcribe", language="xx")


def test_get_prompt():
    cfg = get_config("large-v3")
    m = _bare_model(cfg)
    tok = Tokenizer(None, cfg, True, task="transcribe", language="en")
    assert m.get_prompt(tok, [], without_timestamps=True) == [50258, 50259, 50360, 50364]
    assert m.get_prompt(tok, [], without_timestamps=False) == [50258, 50259, 50360]
    prev = list(range(1000, 1300))
    p = m.get_prompt(tok, prev, without_timestamps=True)
    assert p[0] == cfg.sot_prev and p[1:224] == prev[-223:] and p[224:] == [50258, 50259, 50360, 50364]


def test_suppressed_tokens_matches_reference_rule():
    en = get_config("tiny.en")
    tok = Tokenizer(None, en, False)
    got = get_suppressed_tokens(tok, [-1])
    # without a vocabulary the non-speech set is empty; the six specials are pinned by the
    # reference's tests/test_tokenizer.py:110
    assert got == (50257, 50357, 50358, 50359, 50360, 50361)
    assert get_suppressed_tokens(tok, [5, 3]) == (3, 5, 50257, 50357, 50358, 50359, 50360, 50361)


def test_split_segments_by_timestamps():
    cfg = get_config("large-v3")
    m = _bare_model(cfg)
    tok = Tokenizer(None, cfg, True, task="transcribe", language="en")
    tb = cfg.timestamp_begin
    # <0.00> a b <2.00><2.00> c <4.50>   -> two segments, single timestamp ending
    tokens = [tb, 11, 12, tb + 100, tb + 100, 13, tb + 225]
    segs, seek, single = m._split_segments_by_timestamps(tok, tokens, time_offset=30.0, segment_size=3000,
                                                         segment_duration=30.0, seek=0)
    assert single is True and seek == 3000
    assert [s["tokens"] for s in segs] == [[tb, 11, 12, tb + 100], [tb + 100, 13, tb + 225]]
    assert segs[0]["start"] == pytest.approx(30.0) and segs[0]["end"] == pytest.approx(32.0)
    assert segs[1]["start"] == pytest.approx(32.0) and segs[1]["end"] == pytest.approx(34.5)
    # consecutive timestamps but no single-timestamp ending: seek advances to the last pair
    tokens = [tb, 11, tb + 50, tb + 50, 12, 13]
    segs, seek, single = m._split_segments_by_timestamps(tok, tokens, 0.0, 3000, 30.0, 0)
    assert single is False and len(segs) == 1 and seek == 50 * 2
    # no consecutive timestamps: one segment, duration from the last timestamp
    tokens = [11, 12, tb + 200]
    segs, seek, _ = m._split_segments_by_timestamps(tok, tokens, 60.0, 3000, 30.0, 0)
    assert len(segs) == 1 and segs[0]["end"] == pytest.approx(64.0) and seek == 3000
    # text only: whole chunk
    segs, seek, _ = m._split_segments_by_timestamps(tok, [11, 12], 0.0, 2500, 25.0, 0)
    assert segs[0]["start"] == 0.0 and segs[0]["end"] == 25.0 and seek == 2500


def test_pad_or_trim_and_compression_ratio():
    a = np.arange(12, dtype=np.float32).reshape(2, 6)
    assert pad_or_trim(a, 4).shape == (2, 4) and np.array_equal(pad_or_trim(a, 4), a[:, :4])
    p = pad_or_trim(a, 9)
    assert p.shape == (2, 9) and np.array_equal(p[:, :6], a) and float(np.abs(p[:, 6:]).max()) == 0.0
    assert get_compression_ratio("a" * 100) > 5


def test_partition_is_contiguous_and_balanced():
    for n, w in [(120, 8), (10, 4), (3, 8), (0, 2), (17, 1)]:
        parts = partition(n, w)
        assert len(parts) == w and parts[0][0] == 0 and parts[-1][1] == n
        assert all(parts[i][1] == parts[i + 1][0] for i in range(w - 1))
        sizes = [b - a for a, b in parts]
        assert max(sizes) - min(sizes) <= 1
    assert partition(120, 8)[3] == (45, 60)


def test_result_records_roundtrip():
    class R:
        def __init__(self, ids, s, n):
            self.sequences_ids, self.scores, self.no_speech_prob = [ids], [s], n
    rs = [R([1, 2, 3], -0.25, 0.5), R([], -1.5, 0.0), R(list(range(40)), 0.0, 1.0)]
    rec = encode_records(rs, 32)
    assert rec.shape == (3, 37) and rec.dtype == np.int32   # 1 + 32 ids + 2 float64
    back = decode_records(rec, 32)
    assert back[0] == ([1, 2, 3], -0.25, 0.5) and back[1] == ([], -1.5, 0.0)
    assert back[2][0] == list(range(32))   # truncated to max_len


def test_bench_pipeline_measure_runs_on_a_scripted_backend():
    """bench.py's secondary end-to-end number: exercised here without a GPU (scripted backend), and a broken
    backend must be reported, never raised"""
    import bench
    from oracle import micro_tokenizer
    from oracle.scripted_backend import ScriptedBackend
    cfg = get_config("micro")
    backend = ScriptedBackend(cfg, micro_tokenizer.build())
    backend.inter_threads = 3
    r = bench.pipeline_rtf(backend, cfg, 7, 2, 5, 20)
    assert r["segments"] == 7 and r["tokens"] == 7 * 20 and r["audio_s"] == 210.0 and r["value"] > 0
    assert "error" in bench.pipeline_rtf(object(), cfg, 2, 2, 5, 20)


def test_idle_decode_group_splits_known_work_evenly():
    """Round 5: the run size an IDLE two-lane decode group leads with (csrc/decoder.hip: idle_lead_chunks, through the
    host-only hook fw_test_idle_lead_chunks — no device involved).  The reference's replica pool decodes batches side by
    side (transcribe.py:645-657); here the batches of the workers share decode runs, and a group with no run in progress
    starts its first run at its even share of the work it knows of instead of waiting for 90 % of a run's capacity."""
    from faster_whisper_amd import _lib
    f = _lib.load().fw_test_idle_lead_chunks
    cap = 320                                       # chunks one run takes (1 600 rows at beam 5)
    # the driver's burst: 20 batches of 16 in flight — k queued, 20 - k still encoding -> lead at 10 batches
    for k in range(1, 21):
        assert f(16 * k, k, 20 - k, cap, 16) == 160
    # all 32 workers in flight: 512 chunks > one run -> two runs of 256 (the plain rule would wait for 288)
    assert f(16, 1, 31, cap, 16) == 256
    # more than two runs' worth: ceil(1 000 / 320) = 4 runs of 250
    assert f(200, 10, 40, cap, 20) == 250
    # a lone caller / nothing else on its way: its own batch, at least one max_batch
    assert f(16, 1, 0, cap, 16) == 16
    assert f(3, 1, 0, cap, 16) == 16
    # ragged batches: the pending requests are counted at the average size of the queued ones
    assert f(11 + 16, 2, 2, cap, 16) == (27 + 2 * 13 + 1) // 2
    # degenerate arguments do not divide by zero
    assert f(0, 0, 0, 0, 1) == 1 and f(16, 0, -3, cap, 16) == 16


def test_run_capacity_is_stated_once():
    """What a decode lane holds of runs led by one call (csrc/decoder.hip: RunCapacity, through the host-only hook
    fw_test_run_capacity — no device involved): rows per encoder chunk, whether the call alone fits the lane (the entry
    refusal of fw_generate), the chunks the leader waits for and the chunks the run is filled to.  The reference is the
    arithmetic the entry check, the leader's wait and the gather loop each spelt out on their own before they shared it,
    restated here; 1 600 = the rows above which the decoder linears start a second round of workgroups."""
    import ctypes as C
    from faster_whisper_amd import _lib
    lib = _lib.load()

    def got(cap, max_batch, max_beam, self_cap, B, sampling, beam, nh, ctx):
        rpc, want, run_cap = C.c_int64(), C.c_int64(), C.c_int64()
        fits = lib.fw_test_run_capacity(cap, max_batch, max_beam, self_cap, B, int(sampling), beam, nh, ctx,
                                        C.byref(rpc), C.byref(want), C.byref(run_cap))
        return fits, rpc.value, want.value, run_cap.value

    def ref(cap, max_batch, max_beam, self_cap, B, sampling, beam, nh, ctx):
        rpc = max(1, nh) if sampling else beam
        rows = B * nh if sampling else B * beam
        fits = int(not (rows > cap * max_beam or rows * ctx > self_cap))
        run_cap = min(cap, max(B, self_cap // (rpc * ctx)))
        if not sampling:
            want = min(cap, max(max_batch, 1600 // max(1, beam)))
            run_cap = min(run_cap, max(max_batch, 1600 // max(1, beam)))
        else:
            want = 0                                   # the leader of a run of sampling calls does not wait
            run_cap = min(run_cap, max(B, cap * max_beam // max(1, nh)))
        return fits, rpc, want, run_cap

    # anchors worked by hand: (lane chunks, max_batch, max_beam, self capacity, B, sampling, beam, hypotheses, context)
    assert got(400, 16, 5, 400 * 5 * 448, 16, False, 5, 1, 448) == (1, 5, 320, 320)      # 1 600 rows bind
    assert got(320, 16, 5, 320 * 5 * 448, 16, False, 5, 1, 448)[3] == 320
    assert got(64, 16, 5, 64 * 5 * 448, 16, True, 1, 8, 448) == (1, 8, 0, 40)            # 8 rows per chunk; the lane's rows bind
    n = 0
    for cap, max_batch, max_beam in ((4, 4, 5), (16, 16, 5), (64, 16, 5), (320, 16, 5), (400, 16, 5), (409, 16, 5), (24, 8, 1)):
        for nts in (8, 104, 448):                      # positions per cache row at full row capacity
            self_cap = cap * max_beam * nts
            for B in (1, 3, max_batch):
                for ctx in (8, 104, 448):
                    for beam in {1, 2, max_beam}:
                        for nh in {1, beam}:
                            args = (cap, max_batch, max_beam, self_cap, B, False, beam, nh, ctx)
                            assert got(*args) == ref(*args), args
                            n += 1
                    for nh in (1, 5, 8, 40):
                        args = (cap, max_batch, max_beam, self_cap, B, True, 1, nh, ctx)
                        assert got(*args) == ref(*args), args
                        n += 1
    assert n > 1000


def test_decoder_linear_plan_states_the_products_choice():
    """Which kernel form a decoder linear takes (csrc/dec_kernels.hip: dec_linear_plan, through the host-only hook
    fw_test_dec_linear_plan — no device involved).  The GPU tests force a form and compare bits; this one states which form
    the PRODUCT chooses, as literal expectations: the measured crossover rows of the table, the fit conditions of the
    GEMM-shaped kernel (a rule whose shape does not fit K stays skinny), the tile grouping and the wave count."""
    import ctypes as C
    from faster_whisper_amd import _lib
    lib = _lib.load()
    REFUSED = (0, -1, 0, 0, 0, 0)

    def plan(R, N, K, form=0, ldo=None, ldr=0, int8=0):
        out = (C.c_int32 * 6)()
        assert lib.fw_test_dec_linear_plan(R, N, K, N if ldo is None else ldo, ldr, int8, form, out) == 0
        return tuple(out)

    def one(waves=4):
        return (1, -1, 1, 1, 10, waves)       # skinny, one 16 x 16 tile per workgroup, 10 k-steps in flight

    def two(waves=4):
        return (1, -1, 2, 2, 5, waves)        # skinny, 2 x 2 tiles

    def big(cfg, slices=4):
        return (2, cfg, 0, 0, 0, slices)

    want = {
        (3840, 1280): {639: two(), 640: big(2), 1279: big(2), 1280: big(0)},                          # large-v3 qkv
        (1280, 1280): {5: one(), 16: one(), 17: one(), 96: one(), 97: two(), 1087: two(), 1088: big(1)},   # d x d
        (5120, 1280): {16: one(), 17: two(), 511: two(), 512: big(2), 1280: big(0)},                  # ffn1
        (1280, 5120): {80: one(8), 831: two(8), 832: big(1, 8)},                                      # ffn2
        (1152, 384): {640: big(2), 1280: two()},      # tiny qkv: the rule's cfg 0 does not fit K = 384 -> skinny, not cfg 2
        (384, 1536): {832: two(), 1088: big(1)},      # tiny ffn2 has the role d x d
        (2048, 512): {512: two(), 1088: big(1)},      # base ffn1 has the role d x d
    }
    for (N, K), rows in want.items():
        for R, w in rows.items():
            assert plan(R, N, K) == w, (R, N, K)
    # the shapes tests/test_gpu_gemm_forms.py: BIG_REFUSED states: K = 128 takes workgroup shape 2 only, K = 256 all three
    for R in (80, 333):
        assert [plan(R, 256, 128, form=10 + c) for c in range(3)] == [REFUSED, REFUSED, big(2)]
        assert [plan(R, 256, 256, form=10 + c) for c in range(3)] == [big(0), big(1), big(2)]
    assert plan(1088, 1280, 1280, ldo=1284) == two()             # row segments of the output not 16 bytes
    assert plan(1088, 1280, 1280, ldr=1284) == two()             # ... of the residual
    assert plan(1088, 1280, 1280, ldr=1280) == big(1)
    assert plan(1088, 1280, 1280, form=11, ldo=1284) == REFUSED  # a forced form that does not fit is refused
    for form in (0, 5, 6, 7, 10, 11, 12):
        assert plan(80, 1280, 1296, form=form) == REFUSED        # K % 32 != 0
        assert plan(0, 1280, 1280, form=form) == REFUSED
    assert plan(80, 1280, 1280, form=13) == REFUSED and plan(80, 1280, 1280, form=2) == REFUSED   # no such form
    # forced skinny forms: 5 groups by row count whatever the table says, 6 / 7 are one tile / 2 x 2 at any row count
    assert plan(1088, 1280, 1280, form=5) == two() and plan(80, 1280, 1280, form=5) == one()
    for R in (1, 80, 1088, 2000):
        assert plan(R, 1280, 1280, form=6) == one() and plan(R, 1280, 1280, form=7) == two()
        assert plan(R, 1280, 5120, form=6) == one(8) and plan(R, 1280, 5120, form=7) == two(8)
    # int8_float16: 4 x 4 tiles from 1 024 rows when N % 64 == 0, 2 x 2 tiles otherwise; k-steps of 64
    assert plan(1023, 1280, 1280, int8=1) == two() and plan(1024, 1280, 1280, int8=1) == (1, -1, 4, 4, 5, 4)
    assert plan(1024, 1280, 5120, int8=1) == (1, -1, 4, 4, 3, 8)
    assert plan(1024, 1312, 1280, int8=1) == two()
    assert plan(80, 1280, 1312, int8=1) == REFUSED and plan(0, 1280, 1280, int8=1) == REFUSED
    # what bench.py prices by: the exported row count of a role = the lowest row count at which the plan of that role's
    # large-v3 shape leaves the 2 x 2 grouping (fp16: for the GEMM-shaped kernel; int8: for 4 x 4 tiles)
    shapes = ((3840, 1280), (1280, 1280), (5120, 1280), (1280, 5120))
    for role, (N, K) in enumerate(shapes):
        first_big = next(R for R in range(1, 4096) if plan(R, N, K)[0] == 2)
        assert lib.fw_dec_big_min_rows_of(role, 0) == first_big == (640, 1088, 512, 832)[role]
        first_44 = next(R for R in range(1, 4096) if plan(R, N, K, int8=1)[2] == 4)
        assert lib.fw_dec_big_min_rows_of(role, 1) == first_44 == 1024
    assert lib.fw_dec_big_min_rows() == lib.fw_dec_big_min_rows_of(-1, 0) == 512


def test_encoder_gemm_plan_states_the_products_choice():
    """What the encoder GEMM's launcher does for a launch (csrc/gemm.hip: gemm_plan, through the host-only hook
    fw_test_gemm_plan — no device involved).  The GPU tests compare the blocked tile order and the staged V^T epilogue with
    their knob-off forms bit for bit; this one states, as literal expectations, which tile-order block, epilogue and
    instantiation the PRODUCT chooses for the encoder's own launches (large-v3: d = 1280, 32 decoder layers; tiny: d = 384,
    4 decoder layers; T = 1500, conv1's M = 3000; one chunk and 16), and which shapes it refuses.  The tile is 256 x 256."""
    import ctypes as C
    from faster_whisper_amd import _lib
    lib = _lib.load()
    REFUSED = (-1, 0, 0, 0, 0, 0, 0, 0, 0)
    F16, F16_T, I8, I8_T, LAYERED, LAYERED_T = range(6)      # the instantiations: trans + 2 * int8, layered 4 + trans

    def plan(M, N, K, batch=1, lda=None, ldw=None, a_bs=None, ldc=None, c_bs=None, trans=0, int8=0, head_rows=0,
             n_layers=1, res=0):
        lda = K if lda is None else lda
        ldc = ((M + 63) // 64 * 64 if trans else N) if ldc is None else ldc
        out = (C.c_int32 * 9)()
        assert lib.fw_test_gemm_plan(M, N, K, batch, lda, K if ldw is None else ldw, M * lda if a_bs is None else a_bs,
                                     ldc, (N if trans else M) * ldc if c_bs is None else c_bs, trans, int8, head_rows,
                                     n_layers, res, out) == 0
        return tuple(out)

    def want(kernel, nMt, nNt, batch, blk, vt_stage=0, n_layers=1):
        """blk = (n tiles, m panels) of the tile-order block"""
        return (kernel, nMt, nNt, nNt // n_layers, nMt * batch, blk[0], blk[1], vt_stage, nMt * nNt * batch)

    T, kvp, t_pad = 1500, 1504, 1536
    for batch in (1, 16):
        for int8 in (0, 1):
            lin, lin_t = (I8, I8_T) if int8 else (F16, F16_T)
            # ---- large-v3: every width is a multiple of 5 n tiles -> blocks of 5 n tiles x 6 m panels
            d = 1280
            kw = dict(batch=batch, int8=int8)
            assert plan(T, 2 * d, d, **kw) == want(lin, 6, 10, batch, (5, 6))                              # Q|K
            # V^T: the staged epilogue is the fp16 one's
            assert plan(T, d, d, trans=1, ldc=t_pad, **kw) == want(lin_t, 6, 5, batch, (5, 6), vt_stage=1 - int8)
            assert plan(T, d, d, res=1, **kw) == want(lin, 6, 5, batch, (5, 6))                            # out
            assert plan(T, 4 * d, d, **kw) == want(lin, 6, 20, batch, (5, 6))                              # ffn1
            assert plan(T, d, 4 * d, res=1, **kw) == want(lin, 6, 5, batch, (5, 6))                        # ffn2
            # ---- tiny: 3 x 10 for Q|K, 2 x 16 for the d-wide outputs, 6 x 5 for ffn1
            d = 384
            assert plan(T, 2 * d, d, **kw) == want(lin, 6, 3, batch, (3, 10))
            assert plan(T, d, d, trans=1, ldc=t_pad, **kw) == want(lin_t, 6, 2, batch, (2, 16), vt_stage=1 - int8)
            assert plan(T, d, d, res=1, **kw) == want(lin, 6, 2, batch, (2, 16))
            assert plan(T, 4 * d, d, **kw) == want(lin, 6, 6, batch, (6, 5))
            assert plan(T, d, 4 * d, res=1, **kw) == want(lin, 6, 2, batch, (2, 16))
        # the convolutions are fp16 GEMMs in both compute types: conv1 over the padded mel image (128 channels, K = 3 x 128,
        # rows one channel row apart), conv2 over the padded conv1 image (K = 3 d, rows 2 d apart)
        for d, blk in ((1280, (5, 6)), (384, (2, 16))):
            nNt = -(-d // 256)
            assert plan(3000, d, 384, batch=batch, lda=128, a_bs=3002 * 128, c_bs=3002 * d) == want(F16, 12, nNt, batch, blk)
            assert plan(T, d, 3 * d, batch=batch, lda=2 * d, a_bs=3002 * d, res=1) == want(F16, 6, nNt, batch, blk)
            # cross-attention K / V^T, fragment-major (head_rows), one launch per layer (int8_float16, knob 6 off) ...
            for int8 in (0, 1):
                assert plan(T, d, d, batch=batch, c_bs=d * kvp, head_rows=kvp, int8=int8) == \
                    want(I8 if int8 else F16, 6, nNt, batch, blk)
                assert plan(T, d, d, batch=batch, trans=1, ldc=kvp, c_bs=d * kvp, head_rows=kvp, int8=int8) == \
                    want(I8_T if int8 else F16_T, 6, nNt, batch, blk)
        # ... and all decoder layers in one launch (fp16): 32 x 5 = 160 n tiles / 4 x 2 = 8 n tiles -> 8 x 4
        for d, L in ((1280, 32), (384, 4)):
            nNt = -(-d // 256) * L
            kw = dict(batch=batch, c_bs=d * kvp, head_rows=kvp, n_layers=L)
            assert plan(T, d, d, **kw) == want(LAYERED, 6, nNt, batch, (8, 4), n_layers=L)
            assert plan(T, d, d, trans=1, ldc=kvp, **kw) == want(LAYERED_T, 6, nNt, batch, (8, 4), n_layers=L)
    # one m panel or one n tile: nothing to block
    assert plan(256, 1280, 1280) == want(F16, 1, 5, 1, (0, 0))
    assert plan(257, 1280, 1280) == want(F16, 2, 5, 1, (5, 6))
    assert plan(256, 1280, 1280, batch=2) == want(F16, 1, 5, 2, (5, 6))
    assert plan(1500, 256, 1280, batch=16) == want(F16, 6, 1, 16, (0, 0))
    # a width with no divisor but 1 up to 16 (17 n tiles): blocks of 1 x 32
    assert plan(1500, 17 * 256, 128) == want(F16, 6, 17, 1, (1, 32))
    # the staged V^T epilogue: trans, fp16, plain layout, ldc and the chunk stride multiples of 8 halves
    assert plan(300, 128, 128, trans=1, ldc=304)[7] == 1 and plan(300, 128, 128, trans=1, ldc=304, batch=2)[7] == 1
    assert plan(300, 128, 128, trans=1, ldc=300)[7] == 0 and plan(300, 128, 128, trans=1, ldc=304, c_bs=128 * 304 + 4)[7] == 0
    assert plan(300, 128, 128, ldc=304)[7] == 0 and plan(300, 128, 128, trans=1, ldc=304, int8=1)[7] == 0
    assert plan(300, 128, 128, trans=1, ldc=320, c_bs=128 * 320, head_rows=320)[7] == 0
    # the knobs' off settings (the references of the GPU bit-identity tests): no staging, n fastest across the width
    try:
        _lib.check(lib.fw_test_knob(5, 0))
        assert plan(T, 1280, 1280, trans=1, ldc=t_pad, batch=16) == want(F16_T, 6, 5, 16, (5, 6), vt_stage=0)
        _lib.check(lib.fw_test_knob(5, 1))
        _lib.check(lib.fw_test_knob(1, 0))
        assert plan(T, 1280, 1280, trans=1, ldc=t_pad, batch=16) == want(F16_T, 6, 5, 16, (0, 0), vt_stage=1)
        assert plan(T, 1280, 1280, batch=16, c_bs=1280 * kvp, head_rows=kvp, n_layers=32) == \
            want(LAYERED, 6, 160, 16, (0, 0), n_layers=32)
    finally:
        _lib.check(lib.fw_test_knob(5, 1))
        _lib.check(lib.fw_test_knob(1, 1))
    assert plan(T, 1280, 1280, trans=1, ldc=t_pad, batch=16) == want(F16_T, 6, 5, 16, (5, 6), vt_stage=1)
    # ---- refusals (nothing is launched): K rows of whole 128-byte lines
    assert plan(300, 128, 64) == want(F16, 2, 1, 1, (0, 0)) and plan(300, 128, 96) == REFUSED and plan(300, 128, 0) == REFUSED
    assert plan(300, 128, 128, int8=1) == want(I8, 2, 1, 1, (0, 0)) and plan(300, 128, 64, int8=1) == REFUSED
    # 16-byte aligned rows of A and W and chunks of A (8 halves, 16 codes)
    assert plan(300, 128, 128, lda=136) != REFUSED and plan(300, 128, 128, lda=132) == REFUSED
    assert plan(300, 128, 128, ldw=136) != REFUSED and plan(300, 128, 128, ldw=132) == REFUSED
    assert plan(300, 128, 128, a_bs=300 * 128 + 8) != REFUSED and plan(300, 128, 128, a_bs=300 * 128 + 4) == REFUSED
    assert plan(300, 128, 128, lda=144, int8=1) != REFUSED and plan(300, 128, 128, lda=136, int8=1) == REFUSED
    # row-major output: N, ldc and the chunk stride multiples of 4; the transposed one takes any
    assert plan(300, 260, 128) != REFUSED and plan(300, 258, 128, ldc=260) == REFUSED
    assert plan(300, 260, 128, ldc=262) == REFUSED and plan(300, 260, 128, c_bs=300 * 260 + 2) == REFUSED
    assert plan(300, 258, 128, trans=1, ldc=301, c_bs=258 * 301 + 1) == want(F16_T, 2, 2, 1, (2, 16))
    # int8 codes need the weight scale; the layered launch is fp16 without a residual
    assert plan(300, 128, 128, int8=2) == REFUSED and plan(300, 128, 128, trans=1, int8=2) == REFUSED
    assert plan(300, 128, 128, n_layers=2, int8=1) == REFUSED and plan(300, 128, 128, n_layers=2, res=1) == REFUSED
    # ---- the six instantiations
    assert [plan(300, 128, 128, trans=t, int8=i)[0] for i in (0, 1) for t in (0, 1)] == [F16, F16_T, I8, I8_T]
    assert [plan(300, 128, 128, trans=t, n_layers=2)[0] for t in (0, 1)] == [LAYERED, LAYERED_T]
    assert plan(300, 128, 128, n_layers=1, res=1)[0] == F16


def test_self_attention_form_is_stated_once():
    """The form the decode self-attention takes (csrc/dec_kernels.hip: self_attn_form, through the host-only hook
    fw_test_self_attn_form): 1 where the second form is unusable (slot-table stride not a multiple of 4, a layer's cache
    of 4 GB or more), else by launch size — 2 (latency) up to 8 rows per chunk and 768 workgroups, 3 (throughput) beyond."""
    from faster_whisper_amd import _lib
    f = _lib.load().fw_test_self_attn_form

    def form(n_ctx=448, cache_ctx=448, d=1280, R_total=1600, kmul=5, H=20, chunks=16, knob=0):
        return f(n_ctx, cache_ctx, d, R_total, kmul, H, chunks, knob)

    assert form(n_ctx=446, cache_ctx=446) == 1 and form(n_ctx=446, cache_ctx=446, knob=3) == 1
    # 4096 slots x 512 positions x 1024 x 2 bytes = 2^32 exactly
    assert form(cache_ctx=512, n_ctx=512, d=1024, R_total=4096) == 1
    assert form(cache_ctx=512, n_ctx=512, d=1024, R_total=4095) == 2
    assert form(chunks=38) == 2 and form(chunks=39) == 3            # 20 heads x 38 = 760 <= 768 < 780
    assert form(kmul=8) == 2 and form(kmul=9) == 3
    assert form(kmul=9, knob=2) == 3 and form(kmul=8, knob=2, chunks=400) == 2
    assert form(knob=1) == 1 and form(knob=3) == 3


def test_speech_timestamps_skip_ahead_equals_every_window():
    """round 6: get_speech_timestamps jumps over the windows that cannot change its state (an 8 h recording is 900 000
    windows); the plain walk over every window — the reference's loop, vad.py:85-160 — must give the same spans for any
    probabilities and options: run lengths around every duration threshold, probabilities inside the hysteresis band,
    over-long speech with and without a cut candidate"""
    from faster_whisper_amd.vad import VadOptions, get_speech_timestamps
    rng = np.random.default_rng(2024)
    n_cases = 0
    for case in range(400):
        n = int(rng.integers(1, 1500))
        kind = case % 4
        if kind == 0:                                   # i.i.d. noise around the thresholds
            p = rng.uniform(0.2, 0.8, n)
        elif kind == 1:                                 # long runs of speech / silence / in-band values
            p = np.empty(n)
            i = 0
            while i < n:
                run = int(rng.integers(1, 120))
                p[i:i + run] = rng.choice([0.02, 0.3, 0.42, 0.6, 0.97]) + rng.uniform(-0.01, 0.01)
                i += run
        elif kind == 2:                                 # mostly speech with short dips: exercises the max-duration cuts
            p = np.full(n, 0.9)
            for _ in range(int(rng.integers(0, 12))):
                a = int(rng.integers(0, n))
                p[a:a + int(rng.integers(1, 9))] = rng.choice([0.1, 0.4])
        else:                                           # mostly silence with bursts
            p = np.full(n, 0.05)
            for _ in range(int(rng.integers(0, 10))):
                a = int(rng.integers(0, n))
                p[a:a + int(rng.integers(1, 200))] = 0.8
        opts = VadOptions(threshold=float(rng.choice([0.5, 0.35, 0.6])),
                          neg_threshold=None if rng.random() < 0.6 else float(rng.choice([0.2, 0.3])),
                          min_speech_duration_ms=int(rng.choice([0, 100, 250])),
                          max_speech_duration_s=float(rng.choice([float("inf"), 30.0, 4.0, 1.5])),
                          min_silence_duration_ms=int(rng.choice([160, 2000, 500, 64])),
                          speech_pad_ms=int(rng.choice([400, 30, 0])))
        audio = np.zeros(512 * n - int(rng.integers(0, 512)) if n > 1 else 300, np.float32)
        probs = p[:len(audio) // 512 + 1] if len(audio) // 512 + 1 <= n else p
        fast = get_speech_timestamps(audio, opts, speech_probs=probs)
        slow = get_speech_timestamps(audio, opts, speech_probs=probs, _every_window=True)
        assert fast == slow, (case, opts, fast[:3], slow[:3])
        n_cases += bool(slow)
    assert n_cases > 200          # most cases do produce spans
