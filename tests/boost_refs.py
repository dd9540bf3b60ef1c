"""Phrase boosting (include/fwamd.h: fw_boost) restated in numpy, from the wording of the contract alone.

A boost list is N phrases; phrase j is a token-id sequence p_j[0 .. L_j) with one float b_j.  For a row whose generated
history is h[0 .. n), the pair (j, k), 0 <= k < L_j, matches when k <= n and h[n - k .. n) == p_j[0 .. k) (k = 0 always
matches).  The boost of an id v is the MAXIMUM b_j over the matching pairs with p_j[k] == v — fp32 max, never a sum — and
logit[v] += boost(v) is ONE fp32 add; ids without a matching pair keep their bits.

Also here: the ctypes plumbing the boost tests share (building a list, calling the two row hooks)."""
import ctypes as C

import numpy as np

from faster_whisper_amd import _lib

MAX_PHRASES, MAX_LEN, MAX_TOKENS = 1024, 32, 4096


def boost_of_row(phrases, boosts, hist):
    """{id: boost} of one row: the fp32 maximum over the matching pairs of every id that has one"""
    hist = [int(t) for t in hist]
    n = len(hist)
    out = {}
    for p, b in zip(phrases, boosts):
        b = np.float32(b)
        for k in range(len(p)):
            if k <= n and hist[n - k:] == [int(t) for t in p[:k]]:
                v = int(p[k])
                out[v] = b if v not in out else np.maximum(out[v], b)
    return out


def boost_rows(logits, phrases, boosts, hists):
    """logits [rows][V] float32 -> a boosted copy: one fp32 add per boosted id, every other value untouched"""
    out = np.array(logits, dtype=np.float32, copy=True)
    assert out.ndim == 2 and out.shape[0] == len(hists)
    for r, hist in enumerate(hists):
        for v, b in boost_of_row(phrases, boosts, hist).items():
            out[r, v] = np.float32(out[r, v] + b)
    return out


# ---- the library side ----
def ragged(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.int32)
    for i, s in enumerate(seqs):
        offs[i + 1] = offs[i] + len(s)
    flat = np.zeros(max(1, int(offs[-1])), dtype=np.int32)
    for i, s in enumerate(seqs):
        flat[offs[i]:offs[i + 1]] = np.asarray(s, dtype=np.int32)
    return flat, offs


def create_rc(n_vocab, phrases, boosts):
    """fw_boost_create on a list -> (status code, handle); the caller frees a handle it got"""
    lib = _lib.load()
    flat, offs = ragged(phrases)
    b = np.asarray(list(boosts) or [0.0], dtype=np.float32)
    h = C.c_void_p()
    rc = lib.fw_boost_create(int(n_vocab), _lib.as_i32p(flat), _lib.as_i32p(offs), len(phrases), _lib.as_f32p(b), C.byref(h))
    return rc, h


class Boost:
    """a boost list that frees itself"""

    def __init__(self, n_vocab, phrases, boosts):
        rc, self.handle = create_rc(n_vocab, phrases, boosts)
        _lib.check(rc)

    def __del__(self):
        if getattr(self, "handle", None):
            _lib.load().fw_boost_free(self.handle)
            self.handle = None


def rows_host(logits, hists, boost):
    """fw_test_boost_rows_host: the compiled table walked in plain C++ -> the boosted copy"""
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = ragged(hists)
    _lib.check(_lib.load().fw_test_boost_rows_host(_lib.ptr(out), out.shape[0], _lib.ptr(flat), _lib.ptr(offs), boost.handle))
    return out


def rows_gpu(model_handle, logits, hists, boost, form, K=1, done=None):
    """fw_test_boost_rows: ONE launch of dec_boost_kernel in row form `form` -> the whole logits as the launch left them"""
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = ragged(hists)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    _lib.check(_lib.load().fw_test_boost_rows(model_handle, _lib.ptr(out), out.shape[0], _lib.ptr(flat), _lib.ptr(offs), K,
                                              None if dn is None else _lib.ptr(dn), form, boost.handle))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
