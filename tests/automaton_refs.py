"""The plain walk that states automaton-constrained decoding, and wrappers of fw_automaton_create and its three hooks."""
import ctypes as C

import numpy as np

from constrain_refs import bits, ragged  # noqa: F401  (re-exported)
from faster_whisper_amd import _lib


def state_after(csr, ids, ts_begin):
    """delta*(0, the ids below ts_begin), None when undefined"""
    offs, toks, tgts, _ = csr
    s = 0
    for t in ids:
        if t >= ts_begin:
            continue
        edge = [i for i in range(offs[s], offs[s + 1]) if toks[i] == t]
        if not edge:
            return None
        s = tgts[edge[0]]
    return s


def automaton_rows(logits, csr, hists, eot, ts_begin, with_ts, skipped=()):
    """the contract, row by row: kept ids keep their bits, every other one is -inf; skipped rows are untouched"""
    offs, toks, _, acc = csr
    out = np.full_like(logits, -np.inf)
    for r, h in enumerate(hists):
        s = state_after(csr, h, ts_begin)
        keep = list(range(ts_begin, logits.shape[1])) if with_ts else []
        if s is not None:
            keep += [t for t in toks[offs[s]:offs[s + 1]] if t < ts_begin] + ([eot] if acc[s] else [])
        out[r, keep] = logits[r, keep]
        if r in skipped:
            out[r] = logits[r]
    return out


def create_rc(n_vocab, csr, n_states=None):
    """fw_automaton_create -> (status code, handle); the caller frees a handle it got"""
    offs, toks, tgts, acc = (np.ascontiguousarray(a if len(a) else [0], dtype=np.int32) for a in csr)
    h = C.c_void_p()
    rc = _lib.load().fw_automaton_create(int(n_vocab), len(csr[3]) if n_states is None else n_states, _lib.as_i32p(offs),
                                         _lib.as_i32p(toks), _lib.as_i32p(tgts), _lib.as_i32p(acc), C.byref(h))
    return rc, h


class Automaton:
    """a compiled automaton that frees itself"""

    def __init__(self, n_vocab, csr):
        rc, self.handle = create_rc(n_vocab, csr)
        _lib.check(rc)

    def table(self):
        n = C.c_int32()
        _lib.check(_lib.load().fw_test_automaton_table(self.handle, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        _lib.check(_lib.load().fw_test_automaton_table(self.handle, _lib.ptr(out), n.value, C.byref(n)))
        return out

    def __del__(self):
        if getattr(self, "handle", None):
            _lib.load().fw_automaton_free(self.handle)
            self.handle = None


def rows_host(logits, hists, automaton, eot, ts_begin, with_ts):
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = ragged(hists)
    _lib.check(_lib.load().fw_test_automaton_rows_host(_lib.ptr(out), out.shape[0], out.shape[1], eot, ts_begin, int(with_ts),
                                                       _lib.ptr(flat), _lib.ptr(offs), automaton.handle))
    return out


def rows_gpu(model_handle, logits, hists, automaton, eot, ts_begin, with_ts, form, K=1, done=None, staging=0):
    """fw_test_automaton_rows: ONE launch of dec_automaton_kernel -> the whole logits as it left them"""
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = ragged(hists)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    _lib.check(_lib.load().fw_test_automaton_rows(model_handle, _lib.ptr(out), out.shape[0], out.shape[1], eot, ts_begin,
                                                  int(with_ts), _lib.ptr(flat), _lib.ptr(offs), K,
                                                  None if dn is None else _lib.ptr(dn), form, automaton.handle, staging, 0,
                                                  None))
    return out
