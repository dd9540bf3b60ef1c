"""fw_resample_filter (host code of csrc/resample.hip, no GPU): the prototype filter of the device rate converter is the one
faster_whisper_amd/audio.py::resample designs in numpy; fw_resample_dev refuses bad arguments and a missing device."""
import ctypes as C
from math import gcd

import numpy as np
import pytest

from faster_whisper_amd import _lib, audio


def numpy_filter(rate_in, rate_out, taps_per_phase, beta):
    """the filter design of audio.py::resample, restated"""
    g = gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    big = max(up, down)
    half = taps_per_phase * big // 2
    t = np.arange(-half, half + 1, dtype=np.float64)
    cutoff = 0.5 / big
    h = 2 * cutoff * np.sinc(2 * cutoff * t) * np.kaiser(t.size, beta)
    h *= up / h.sum()
    return h, up, down


def c_filter(rate_in, rate_out, taps_per_phase, beta):
    lib = _lib.load()
    n_h, up, down = C.c_int64(), C.c_int32(), C.c_int32()
    _lib.check(lib.fw_resample_filter(rate_in, rate_out, taps_per_phase, beta, None, C.byref(n_h), C.byref(up),
                                      C.byref(down)))
    h = np.full(n_h.value, np.nan)
    n2, up2, down2 = C.c_int64(), C.c_int32(), C.c_int32()
    _lib.check(lib.fw_resample_filter(rate_in, rate_out, taps_per_phase, beta, _lib.ptr(h), C.byref(n2), C.byref(up2),
                                      C.byref(down2)))
    assert (n2.value, up2.value, down2.value) == (n_h.value, up.value, down.value)
    return h, up.value, down.value


@pytest.mark.parametrize("rate_in,taps,beta", [(44100, 32, 9.0), (48000, 32, 9.0), (22050, 32, 9.0), (11025, 32, 9.0),
                                               (8000, 32, 9.0), (96000, 32, 9.0), (44100, 16, 6.0)])
def test_filter_equals_the_numpy_design(rate_in, taps, beta):
    h_np, up_np, down_np = numpy_filter(rate_in, 16000, taps, beta)
    h_c, up, down = c_filter(rate_in, 16000, taps, beta)
    assert (up, down) == (up_np, down_np)
    assert h_c.shape == h_np.shape
    err = float(np.abs(h_c - h_np).max())
    print(f"{rate_in} -> 16000, {taps} taps, beta {beta}: up {up} down {down}, {h_c.size} taps, peak {h_np.max():.6f}, "
          f"max |h_c - h_np| {err:.3e}")
    # both sides are ulp-accurate fp64 formulas and the peak of h is about up / big <= 1 (1.000005 at 8000 -> 16000: the
    # scaling to sum = up); a formula error shows at 1e-6 or more
    assert err <= 1e-13


def test_missing_device_raises_runtime_error():
    x = np.zeros(441, dtype=np.float32)
    with pytest.raises(RuntimeError):
        audio.resample_device(x, 44100, 16000, device_index=10000)
    with pytest.raises(RuntimeError):
        audio.resample_device(x, 16000, 16000, device_index=10000, quantize_s16=True)


def test_bad_arguments_raise_value_error():
    lib = _lib.load()
    x = np.zeros(441, dtype=np.float32)
    out = np.zeros(160, dtype=np.float32)

    def call(rate_in=44100, rate_out=16000, taps=32, xp=_lib.ptr(x), n=441, op=_lib.ptr(out), n_out=160):
        _lib.check(lib.fw_resample_dev(10000, xp, n, rate_in, rate_out, taps, 9.0, 0, op, n_out))

    for kw in ({"rate_in": 0}, {"rate_in": -44100}, {"rate_out": 0}, {"rate_out": -1}, {"taps": 1}, {"taps": 0},
               {"n_out": 159}, {"n_out": 161}, {"xp": None}, {"op": None}, {"n": -1, "n_out": 0}):
        with pytest.raises(ValueError):
            call(**kw)
    # an empty signal is no error and needs neither pointers nor a device
    assert lib.fw_resample_dev(10000, None, 0, 44100, 16000, 32, 9.0, 1, None, 0) == _lib.FW_OK
    with pytest.raises(ValueError):
        call(n=0, n_out=1)
    n_h, up, down = C.c_int64(), C.c_int32(), C.c_int32()
    for rate_in, rate_out, taps in ((0, 16000, 32), (44100, -16000, 32), (44100, 16000, 1)):
        with pytest.raises(ValueError):
            _lib.check(lib.fw_resample_filter(rate_in, rate_out, taps, 9.0, None, C.byref(n_h), C.byref(up), C.byref(down)))
    with pytest.raises(ValueError):
        audio.resample_device(np.zeros((4, 2), dtype=np.float32), 44100, 16000)


def test_decode_audio_device_index_is_keyword_only():
    import inspect
    p = inspect.signature(audio.decode_audio).parameters["device_index"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert list(inspect.signature(audio.decode_audio).parameters)[-1] == "device_index"
