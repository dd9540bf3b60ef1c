"""The Silero network over N recordings in one device call (csrc/vad.hip: fw_vad_forward_audio_batch_dev — one front-end
launch over the windows of all recordings, one recurrence workgroup per recording) against N single-recording calls
(fw_vad_forward_audio_dev, which tests/test_gpu_vad.py pins to the oracle): probabilities and the final LSTM state of
every recording must be the same BITS — the two forms share their arithmetic, so there is no tolerance here."""
import numpy as np
import pytest

from test_gpu_vad import _audio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from faster_whisper_amd import vad
    from test_vad_network import synthetic_weights
    return vad.SileroVADModel(weights=synthetic_weights(5), device="cuda")


def _recordings(windows, seed=100):
    return [_audio(max(n, 10), seed=seed + i)[:512 * n] for i, n in enumerate(windows)]


def _states(n_rec, seed):
    """zeros (seed None) or a distinct non-zero LSTM state per recording"""
    if seed is None:
        return np.zeros((n_rec, 128), np.float32), np.zeros((n_rec, 128), np.float32)
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.9, 0.9, (n_rec, 128)).astype(np.float32),
            rng.uniform(-2.0, 2.0, (n_rec, 128)).astype(np.float32))


def _single_calls(dev, recs, h0, c0):
    from faster_whisper_amd import _lib
    lib = _lib.load()
    out = []
    for r, a in enumerate(recs):
        a = np.ascontiguousarray(a)
        h, c = h0[r].copy(), c0[r].copy()
        p = np.empty(a.shape[0] // 512, np.float32)
        _lib.check(lib.fw_vad_forward_audio_dev(dev._handle, 0, _lib.ptr(a), a.shape[0], _lib.ptr(h), _lib.ptr(c),
                                                _lib.ptr(p)))
        out.append((p, h, c))
    return out


def _batch_call(dev, recs, h0, c0):
    from faster_whisper_amd import _lib
    lib = _lib.load()
    offsets = np.zeros(len(recs) + 1, np.int64)
    offsets[1:] = np.cumsum([a.shape[0] for a in recs])
    audio = np.ascontiguousarray(np.concatenate(recs)) if recs else np.zeros(0, np.float32)
    h, c = h0.copy(), c0.copy()
    p = np.full(int(offsets[-1]) // 512, np.nan, np.float32)
    _lib.check(lib.fw_vad_forward_audio_batch_dev(dev._handle, 0, _lib.ptr(audio), _lib.ptr(offsets), len(recs),
                                                  _lib.ptr(h), _lib.ptr(c), _lib.ptr(p)))
    return [(p[a // 512:b // 512], h[r], c[r]) for r, (a, b) in enumerate(zip(offsets[:-1], offsets[1:]))]


def _assert_same(got, want):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        for name, x, y in zip(("probs", "h", "c"), g, w):
            assert x.shape == y.shape and np.array_equal(x, y), (r, name, np.abs(x - y).max() if x.size else None)


@pytest.mark.parametrize("state_seed", [None, 9], ids=["zero_state", "given_state"])
def test_ragged_recordings_equal_the_single_calls(dev, state_seed):
    """1-window recordings: zero context AND zeroed tail at once; the empty one: state untouched, no output; neighbours of
    different lengths: no context leaks across a boundary"""
    windows = (1, 2, 37, 800, 0, 1, 5)
    recs = _recordings(windows)
    h0, c0 = _states(len(recs), state_seed)
    want = _single_calls(dev, recs, h0, c0)
    assert want[4][0].shape == (0,) and np.array_equal(want[4][1], h0[4])   # the empty recording: nothing happens
    got = _batch_call(dev, recs, h0, c0)
    _assert_same(got, want)
    assert all(np.isfinite(g[0]).all() for g in got)                 # every probability was written
    if state_seed is None:
        assert np.abs(got[3][1]).max() > 0                           # (the state does move)


def test_more_recordings_than_compute_units(dev):
    recs = _recordings((3,) * 300, seed=1000)
    h0, c0 = _states(300, None)
    _assert_same(_batch_call(dev, recs, h0, c0), _single_calls(dev, recs, h0, c0))


def test_groups_of_recordings_equal_the_single_calls(dev):
    """more windows than one group holds (FW_VAD_BATCH_MAX_WINDOWS = 131 072): the call runs [0] and then [1, 2, 3] through
    the same buffers, the second group with a non-zero first window and an empty recording in it"""
    base = _audio(1000, seed=21)
    recs = [np.tile(base, 70), np.tile(base[::-1].copy(), 66), base[:0], base[:512 * 5].copy()]
    assert sum(r.shape[0] for r in recs) // 512 > 131072 > recs[0].shape[0] // 512
    h0, c0 = _states(4, 3)
    _assert_same(_batch_call(dev, recs, h0, c0), _single_calls(dev, recs, h0, c0))


def test_one_recording_equals_the_single_call(dev):
    recs = _recordings((41,), seed=7)
    h0, c0 = _states(1, 4)
    _assert_same(_batch_call(dev, recs, h0, c0), _single_calls(dev, recs, h0, c0))


def test_no_recordings_and_bad_arguments(dev):
    """argument checks only: each of these returns before anything is started on the device"""
    from faster_whisper_amd import _lib
    lib = _lib.load()
    a = np.zeros(2048, np.float32)
    h = np.full((3, 128), 0.25, np.float32)
    c = np.full((3, 128), -0.5, np.float32)
    p = np.full(4, np.nan, np.float32)

    def call(offsets, n_rec, audio=a, hh=h, cc=c, pp=p, handle=None):
        off = None if offsets is None else _lib.ptr(np.asarray(offsets, np.int64))
        return lib.fw_vad_forward_audio_batch_dev(dev._handle if handle is None else handle, 0,
                                                  None if audio is None else _lib.ptr(audio), off, n_rec,
                                                  None if hh is None else _lib.ptr(hh),
                                                  None if cc is None else _lib.ptr(cc),
                                                  None if pp is None else _lib.ptr(pp))

    assert call([0], 0) == _lib.FW_OK
    assert call([0, 0, 0, 0], 3) == _lib.FW_OK                           # three empty recordings
    assert call([0, 1024, 512, 2048], 3) == _lib.FW_EINVAL               # decreasing
    assert call([0, 700, 1024, 2048], 3) == _lib.FW_EINVAL               # not a multiple of 512
    assert call([0, 512, 1024, 2048], -1) == _lib.FW_EINVAL
    assert call(None, 3) == _lib.FW_EINVAL
    assert call([0, 512, 1024, 2048], 3, audio=None) == _lib.FW_EINVAL
    assert call([0, 512, 1024, 2048], 3, hh=None) == _lib.FW_EINVAL
    assert call([0, 512, 1024, 2048], 3, cc=None) == _lib.FW_EINVAL
    assert call([0, 512, 1024, 2048], 3, pp=None) == _lib.FW_EINVAL
    assert lib.fw_vad_forward_audio_batch_dev(dev._handle, 99, _lib.ptr(a), _lib.ptr(np.asarray([0, 512, 1024, 2048], np.int64)),
                                              3, _lib.ptr(h), _lib.ptr(c), _lib.ptr(p)) == _lib.FW_ENODEV
    with pytest.raises(ValueError):
        _lib.check(call([0, 512, 256, 2048], 3))
    assert np.isnan(p).all() and (h == 0.25).all() and (c == -0.5).all()  # nothing was touched


def test_forward_many_equals_the_per_recording_calls(dev):
    recs = _recordings((4, 1, 0, 19), seed=50)
    got = dev.forward_many(recs)
    assert len(got) == 4 and got[2].shape == (0,)
    for a, g in zip(recs, got):
        if a.shape[0]:
            assert np.array_equal(g, dev(a))
    assert dev.forward_many([]) == []
