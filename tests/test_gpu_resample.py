"""fw_resample_dev (csrc/resample.hip) on the GPU against the host converter faster_whisper_amd.audio.resample /
_to_s16_float (numpy, fp64): same samples unquantised within one float32 ulp, the same s16 waveform exactly, through
decode_audio(device_index=) and through the pipelines' FWAMD_RESAMPLE_DEVICE=1 opt-in."""
import functools
import io
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN, make_model
from faster_whisper_amd import audio
from test_resample_filter import numpy_filter

pytestmark = pytest.mark.gpu

CASES = [(48000, 12347, 1), (44100, 12347, 2), (22050, 12347, 3), (11025, 5003, 4), (8000, 4099, 5), (96000, 20011, 6),
         (32000, 7001, 7), (44100, 1, 8), (44100, 2, 8), (44100, 100, 8), (48000, 1, 8), (8000, 1, 8), (44100, 0, 8)]
CLIPPING = (44100, 12347, 2, 5.0)          # 2 256 of its 4 480 outputs clip
LONG = (44100, 13_500_000, 9)              # 4 897 960 outputs: m * down crosses 2^31


def sig(n, rate, seed, gain=1.0):
    rng = np.random.default_rng(seed); t = np.arange(n, dtype=np.float64) / rate
    return (gain * (0.2 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440.0 * t))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host(rate, n, seed, gain=1.0):
    """(input, the host's fp64 sums, host resample, its s16 form), computed once and never written to"""
    x = sig(n, rate, seed, gain)
    y = audio.resample(x, rate, 16000)
    y64 = audio._resample_f64(x, rate, 16000, 32, 9.0) if n else np.zeros(0)
    assert np.array_equal(y64.astype(np.float32), y)
    q = audio._to_s16_float(y)
    for a in (x, y64, y, q):
        a.setflags(write=False)
    return x, y64, y, q


def tie_distance(y64):
    """smallest distance of the host's fp64 y * 32768 to a half-integer, where rint could go either way"""
    v = y64 * 32768.0
    return float(np.abs(v - np.floor(v) - 0.5).min())


def float32_margin(y64, y):
    """The host path rounds its fp64 sum to float32 (`resample` returns float32) BEFORE _to_s16_float, so the s16 value can
    also turn on which float32 the sum rounds to.  Over the samples whose float32 neighbour on the sum's side quantises to
    another s16 step: (how many, the smallest distance of the fp64 sum to the midpoint of the two float32 values)."""
    toward = np.where(y64 > y, np.inf, -np.inf).astype(np.float32)
    other = np.nextafter(y, toward)
    at_stake = audio._to_s16_float(other) != audio._to_s16_float(y)
    mid = (y.astype(np.float64) + other.astype(np.float64)) / 2
    d = np.abs(mid - y64)[at_stake]
    return int(at_stake.sum()), float(d.min()) if d.size else np.inf


def fp64_sum_bound(rate, x):
    """what two fp64 evaluations of one output can differ by, whatever their order: 2 * taps * 2^-53 * sum |h_i x_i|, taken
    with the largest |x| and the phase with the largest sum |h_i|"""
    h, up, down = numpy_filter(rate, 16000, 32, 9.0)
    phases = [np.abs(h[j::up]) for j in range(up)]
    return 2 * max(p.size for p in phases) * 2.0 ** -53 * max(float(p.sum()) for p in phases) * float(np.abs(x).max())


def assert_s16_equal(case, x, y64, y, q):
    d = tie_distance(y64)
    n_stake, margin = float32_margin(y64, y)
    bound = fp64_sum_bound(case[0], x)
    got = audio.resample_device(x, case[0], 16000, quantize_s16=True)
    bad = int((got != q).sum()) if got.shape == q.shape else -1
    clipped = int((np.abs(y64) * 32768.0 > 32767.5).sum())
    print(f"{case}: {q.size} outputs, {clipped} clipped, distance to a rounding tie {d:.3e}; {n_stake} samples turn on the "
          f"float32 rounding, nearest {margin:.3e} from its boundary (fp64 sums agree within {bound:.1e}); {bad} samples differ")
    # no tie on the host side, in either rounding step: a mismatch has no excuse
    assert d > 1e-8
    assert margin > bound
    assert got.dtype == np.float32 and got.shape == q.shape
    assert np.array_equal(got, q)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_parity_unquantised(case):
    rate, n, seed = case
    x, _, y, _ = host(rate, n, seed)
    got = audio.resample_device(x, rate, 16000)
    assert got.dtype == y.dtype == np.float32 and got.shape == y.shape
    if n == 0:
        return
    err = np.abs(got.astype(np.float64) - y.astype(np.float64))
    ulp = np.spacing(np.abs(y)).astype(np.float64)
    print(f"{case}: {y.size} outputs, {int((err > 0).sum())} differ, worst {float((err / ulp).max()):.2f} ulp")
    # both sides sum in fp64 (they differ by ~1e-14 relative) and round once to float32: equal except on a rounding boundary
    assert np.all(err <= ulp)


@pytest.mark.parametrize("case", CASES + [CLIPPING], ids=lambda c: "-".join(str(v) for v in c[:2] + c[3:]))
def test_parity_quantised_is_exact(case):
    x, y64, y, q = host(*case)
    if x.size == 0:
        got = audio.resample_device(x, case[0], 16000, quantize_s16=True)
        assert got.dtype == np.float32 and got.shape == (0,)
        return
    assert_s16_equal(case, x, y64, y, q)


def test_clipping_case_clips():
    _, y64, _, q = host(*CLIPPING)
    assert q.size == 4480 and int((np.abs(y64) * 32768.0 > 32767.5).sum()) == 2256
    assert q.max() == np.float32(32767 / 32768) and q.min() == np.float32(-1.0)


def test_64_bit_indexing():
    rate, n, seed = LONG
    x = sig(n, rate, seed)
    y64 = audio._resample_f64(x, rate, 16000, 32, 9.0)
    y = y64.astype(np.float32)                                    # = audio.resample(x, rate, 16000), computed once
    assert y.size == 4_897_960 and (y.size - 1) * 441 > 2 ** 31
    assert float(np.abs(y).max()) * 32768.0 < 32767.0            # nothing clips
    assert_s16_equal(LONG, x, y64, y, audio._to_s16_float(y))


@pytest.mark.parametrize("quantize", [False, True])
def test_blocking_does_not_change_a_bit(monkeypatch, quantize):
    rate, n, seed = 44100, 12347, 2
    x = host(rate, n, seed)[0]
    monkeypatch.delenv("FWAMD_RESAMPLE_BLOCK", raising=False)
    ref = audio.resample_device(x, rate, 16000, quantize_s16=quantize)
    again = audio.resample_device(x, rate, 16000, quantize_s16=quantize)
    assert ref.tobytes() == again.tobytes()
    for block in (1, 7, 256, 4096):
        monkeypatch.setenv("FWAMD_RESAMPLE_BLOCK", str(block))
        got = audio.resample_device(x, rate, 16000, quantize_s16=quantize)
        assert got.tobytes() == ref.tobytes(), block
    monkeypatch.setenv("FWAMD_RESAMPLE_BLOCK", "0")
    with pytest.raises(ValueError):
        audio.resample_device(x, rate, 16000)


def test_same_rate_copies_or_quantises():
    x = host(44100, 12347, 2, 5.0)[0]
    assert np.array_equal(audio.resample_device(x, 16000, 16000), x)
    assert np.array_equal(audio.resample_device(x, 16000, 16000, quantize_s16=True), audio._to_s16_float(x))


def wav_bytes(channels, rate):
    """16-bit PCM WAVE of float channels in [-1, 1)"""
    pcm = np.stack([np.clip(np.rint(c.astype(np.float64) * 32768.0), -32768, 32767) for c in channels], axis=1)
    body = pcm.astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, len(channels), rate, rate * 2 * len(channels), 2 * len(channels), 16)
    return (b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt))
            + fmt + b"data" + struct.pack("<I", len(body)) + body)


def test_decode_audio_on_the_device_equals_the_host_path():
    data = wav_bytes([sig(12347, 44100, 2), sig(12347, 44100, 3)], 44100)
    mono_host, mono_dev = audio.decode_audio(data), audio.decode_audio(data, device_index=0)
    assert mono_dev.dtype == np.float32 and mono_dev.shape == mono_host.shape == (4480,)
    assert np.array_equal(mono_dev, mono_host)
    host_lr, dev_lr = audio.decode_audio(data, split_stereo=True), audio.decode_audio(data, split_stereo=True, device_index=0)
    assert len(dev_lr) == 2 and not np.array_equal(host_lr[0], host_lr[1])
    for h, d in zip(host_lr, dev_lr):
        assert d.dtype == np.float32 and np.array_equal(d, h)
    one = wav_bytes([sig(5003, 44100, 4)], 44100)                 # one channel, duplicated by split_stereo
    for h, d in zip(audio.decode_audio(one, split_stereo=True), audio.decode_audio(one, split_stereo=True, device_index=0)):
        assert np.array_equal(d, h)
    flac = os.path.join(GOLDEN, "flac_jfk_head.flac")
    for rate in (8000, 22050, 16000):
        h, d = audio.decode_audio(flac, sampling_rate=rate), audio.decode_audio(flac, sampling_rate=rate, device_index=0)
        assert h.size > 0 and np.array_equal(d, h), rate
    with open(flac, "rb") as f:                                    # file objects too
        assert np.array_equal(audio.decode_audio(io.BytesIO(f.read()), device_index=0), audio.decode_audio(flac))


def test_pipeline_opt_in(tmp_path, monkeypatch):
    import logging
    from faster_whisper_amd.transcribe import BatchedInferencePipeline, FeatureExtractor, WhisperModel
    cfg, _, backend = make_model("micro")
    wm = WhisperModel.__new__(WhisperModel)                       # the host front end around conftest's model
    wm.logger = logging.getLogger("faster_whisper")
    wm.model, wm.hf_tokenizer = backend, None
    wm.feature_extractor = FeatureExtractor(feature_size=cfg.n_mels, backend=backend)
    wm.input_stride, wm.time_precision, wm.max_length = 2, 0.02, 448
    wm.num_samples_per_token, wm.frames_per_second, wm.tokens_per_second = 320, 100, 50
    path = str(tmp_path / "clip_22050.wav")
    with open(path, "wb") as f:
        f.write(wav_bytes([sig(66150, 22050, 4)], 22050))
    pipe = BatchedInferencePipeline(wm)
    kw = dict(vad_filter=False, batch_size=2, language="en", beam_size=2, max_new_tokens=10)

    def run():
        segs, info = pipe.transcribe(path, **kw)
        segs = list(segs)
        assert len(segs) >= 1 and info.duration == pytest.approx(3.0)
        return [(s.tokens, s.start, s.end, s.seek) for s in segs]

    monkeypatch.delenv("FWAMD_RESAMPLE_DEVICE", raising=False)
    plain = run()
    monkeypatch.setenv("FWAMD_RESAMPLE_DEVICE", "1")

    def no_host_resampler(*a, **k):
        raise AssertionError("the opt-in run called the host resampler")
    monkeypatch.setattr(audio, "resample", no_host_resampler)
    opted = run()
    assert opted == plain
    seq = list(wm.transcribe(path, language="en", beam_size=1, max_new_tokens=6)[0])    # the sequential driver opts in too
    assert len(seq) >= 1
    monkeypatch.delenv("FWAMD_RESAMPLE_DEVICE")
    with pytest.raises(AssertionError):                            # unset: the host resampler, as before
        pipe.transcribe(path, **kw)
