"""Constrained decoding (include/fwamd.h: fw_constraint) restated in numpy, from the wording of the contract alone.

A constraint list is N phrases of token ids, p_j[0 .. L_j).  For one logits row with generated history h[0 .. n), let
t[0 .. m) be h without its ids >= ts_begin.  M = {j : m <= L_j and p_j[0 .. m) == t}; the allowed text ids are
A = {p_j[m] : j in M, m < L_j}; <eot> is allowed iff some j in M has L_j == m.  Every id v < ts_begin that is neither in A
nor an allowed <eot> becomes -inf; the ids >= ts_begin become -inf unless the timestamp rules are on; every other value keeps
its bits and nothing is added.

Also here: a mirror of the validation (create time and call time) and the ctypes plumbing the constraint tests share."""
import ctypes as C

import numpy as np

from faster_whisper_amd import _lib

MAX_PHRASES, MAX_LEN, MAX_TOKENS = 1024, 32, 4096


def allowed_of_row(phrases, hist, eot, ts_begin):
    """(the set A restricted to ids < ts_begin, whether <eot> is allowed) for one row"""
    t = [int(x) for x in hist if int(x) < ts_begin]
    m = len(t)
    allowed, eot_ok = set(), False
    for p in phrases:
        p = [int(x) for x in p]
        if m <= len(p) and p[:m] == t:
            if m < len(p):
                if p[m] < ts_begin:
                    allowed.add(p[m])
            else:
                eot_ok = True
    return allowed, eot_ok


def keep_mask(phrases, hist, V, eot, ts_begin, with_ts):
    """bool [V]: the ids of one row that keep their bits"""
    allowed, eot_ok = allowed_of_row(phrases, hist, eot, ts_begin)
    keep = np.zeros(V, dtype=bool)
    if allowed:
        keep[sorted(allowed)] = True
    if eot_ok:
        keep[eot] = True
    keep[ts_begin:] = bool(with_ts)
    return keep


def constrain_rows(logits, phrases, hists, eot, ts_begin, with_ts):
    """logits [rows][V] float32 -> a constrained copy: -inf where the mask is clear, every other value untouched"""
    out = np.array(logits, dtype=np.float32, copy=True)
    assert out.ndim == 2 and out.shape[0] == len(hists)
    for r, hist in enumerate(hists):
        out[r, ~keep_mask(phrases, hist, out.shape[1], eot, ts_begin, with_ts)] = -np.inf
    return out


def in_list(phrases, ids, ts_begin):
    """the guarantee: ids without its timestamps -> 'phrase' (a whole phrase), 'prefix' (a proper prefix of one and no whole
    phrase), or None"""
    t = [int(x) for x in ids if int(x) < ts_begin]
    ps = [[int(x) for x in p] for p in phrases]
    if t in ps:
        return "phrase"
    return "prefix" if any(len(p) > len(t) and p[:len(t)] == t for p in ps) else None


# ---- the validation, mirrored ----
def create_error(n_vocab, phrases):
    """why fw_constraint_create refuses the list, or None"""
    if n_vocab < 1:
        return "n_vocab"
    if len(phrases) > MAX_PHRASES:
        return "too many phrases"
    total = 0
    for p in phrases:
        if not 1 <= len(p) <= MAX_LEN:
            return "phrase length"
        total += len(p)
        if total > MAX_TOKENS:
            return "too many tokens"
    if any(not 0 <= int(t) < n_vocab for p in phrases for t in p):
        return "id outside the vocabulary"
    return None


def call_error(phrases, list_vocab, n_vocab, eot, suppress, suppress_blank, suppress_begin, ngram, min_new):
    """why fw_generate_constrain refuses the call, or None (an empty list is refused for another vocabulary only)"""
    if list_vocab != n_vocab:
        return "vocabulary"
    if not phrases:
        return None
    if ngram > 0:
        return "no_repeat_ngram_size"
    if min_new > 0:
        return "min_new_tokens"
    for p in phrases:
        for i, t in enumerate(p):
            if t >= eot:
                return "id >= eot"
            if t in set(suppress):
                return "suppressed id"
            if i == 0 and suppress_blank and t in set(suppress_begin):
                return "suppress_blank"
    return None


# ---- the library side ----
def ragged(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.int32)
    for i, s in enumerate(seqs):
        offs[i + 1] = offs[i] + len(s)
    flat = np.zeros(max(1, int(offs[-1])), dtype=np.int32)
    for i, s in enumerate(seqs):
        flat[offs[i]:offs[i + 1]] = np.asarray(s, dtype=np.int32)
    return flat, offs


def create_rc(n_vocab, phrases):
    """fw_constraint_create on a list -> (status code, handle); the caller frees a handle it got"""
    lib = _lib.load()
    flat, offs = ragged(phrases)
    h = C.c_void_p()
    rc = lib.fw_constraint_create(int(n_vocab), _lib.as_i32p(flat), _lib.as_i32p(offs), len(phrases), C.byref(h))
    return rc, h


class Constraint:
    """a constraint list that frees itself"""

    def __init__(self, n_vocab, phrases):
        rc, self.handle = create_rc(n_vocab, phrases)
        _lib.check(rc)

    def table(self):
        """the compiled table: int32 words"""
        lib = _lib.load()
        n = C.c_int32()
        _lib.check(lib.fw_test_constraint_table(self.handle, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        _lib.check(lib.fw_test_constraint_table(self.handle, _lib.ptr(out), n.value, C.byref(n)))
        return out

    def __del__(self):
        if getattr(self, "handle", None):
            _lib.load().fw_constraint_free(self.handle)
            self.handle = None


def rows_host(logits, hists, constraint, eot, ts_begin, with_ts):
    """fw_test_constrain_rows_host: the compiled table walked in plain C++ -> the constrained copy"""
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = ragged(hists)
    _lib.check(_lib.load().fw_test_constrain_rows_host(_lib.ptr(out), out.shape[0], out.shape[1], eot, ts_begin, int(with_ts),
                                                       _lib.ptr(flat), _lib.ptr(offs), constraint.handle))
    return out


def rows_gpu(model_handle, logits, hists, constraint, eot, ts_begin, with_ts, form, K=1, done=None):
    """fw_test_constrain_rows: ONE launch of dec_constrain_kernel in row form `form` -> the whole logits as it left them"""
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = ragged(hists)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    _lib.check(_lib.load().fw_test_constrain_rows(model_handle, _lib.ptr(out), out.shape[0], out.shape[1], eot, ts_begin,
                                                  int(with_ts), _lib.ptr(flat), _lib.ptr(offs), K,
                                                  None if dn is None else _lib.ptr(dn), form, constraint.handle))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
