"""What the tests of the large boost form (fw_boost_create_large, dec_boost_trie_kernel) share beside tests/boost_refs.py —
whose numpy restatement of phrase boosting knows no limits and is the reference here too: the ctypes plumbing, and the lists
and histories that the host and the GPU tests both walk."""
import ctypes as C

import numpy as np

import boost_refs as br
from faster_whisper_amd import _lib


def create_rc(n_vocab, phrases, boosts):
    """fw_boost_create_large on a list -> (status code, handle); the caller frees a handle it got"""
    flat, offs = br.ragged(phrases)
    b = np.asarray(list(boosts) or [0.0], dtype=np.float32)
    h = C.c_void_p()
    return _lib.load().fw_boost_create_large(int(n_vocab), _lib.as_i32p(flat), _lib.as_i32p(offs), len(phrases), _lib.as_f32p(b),
                                             C.byref(h)), h


class LargeBoost(br.Boost):
    def __init__(self, n_vocab, phrases, boosts):
        rc, self.handle = create_rc(n_vocab, phrases, boosts)
        _lib.check(rc)


def table(boost):
    """the compiled table of a list of either form"""
    n = C.c_int32()
    _lib.check(_lib.load().fw_test_boost_table(boost.handle, None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=np.int32)
    _lib.check(_lib.load().fw_test_boost_table(boost.handle, _lib.as_i32p(out), n.value, C.byref(n)))
    return out


def rows(logits, hists, boost, model_handle=None, form=0, K=1, done=None):
    """fw_test_boost_trie_rows_host, or with a model's handle ONE launch of dec_boost_trie_kernel -> the boosted copy"""
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = br.ragged(hists)
    head = (_lib.ptr(out), out.shape[0], _lib.ptr(flat), _lib.ptr(offs))
    if model_handle is None:
        _lib.check(_lib.load().fw_test_boost_trie_rows_host(*head, boost.handle))
    else:
        dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
        _lib.check(_lib.load().fw_test_boost_trie_rows(model_handle, *head, K, None if dn is None else _lib.ptr(dn), form,
                                                       boost.handle))
    return out


def edge_list(V):
    """(phrases, boosts, histories): [a, a, a] met by [a, a] (the maximum, not the sum); id z reached from the root, from
    [y] and from [x, y] with boosts -1, 2.5 and -3; a 32-token phrase ending in V - 1 against histories of 0, 1, 30, 31, 32
    and 40 ids that end with as much of it as fits, as they are and with their FIRST id changed (up to 31 ids that breaks
    the match at its earliest token, beyond it lies in front of what counts); V - 1 and 0 as first tokens"""
    rng = np.random.default_rng(V)
    a, x, y, z = 33, 40, 41, 42
    long = [int(t) for t in rng.choice(np.arange(100, 400), size=32, replace=False)]
    long[-1] = V - 1
    phrases = [[a, a, a], [z], [y, z], [x, y, z], long, [V - 1, 7], [0], [long[0], 0], [y, 0]]
    boosts = [1.5, -1.0, 2.5, -3.0, 3.0, 0.25, 0.75, -0.5, 4.0]
    hists = [[a, a], [9, x, y], [y], [x, y, a, a]]
    for n in (0, 1, 30, 31, 32, 40):
        hit = [int(t) for t in rng.integers(8, 400, size=n - min(n, 31))] + long[:min(n, 31)]
        hists += [hit, [hit[0] % 399 + 1] + hit[1:] if n else []]
    return phrases, boosts, hists


def wide_list(V, seed=1):
    """300 first tokens (more than a wave's 64 pairs and a workgroup's 256 threads), one of which, q, is followed by 300
    second tokens — [q]'s node is searched 64 slices at a time and its edges are strided over — with third tokens that
    collide with first ones under other boosts; histories of 5 ids that end in q, in q and a second token, or in neither"""
    rng = np.random.default_rng(seed)
    first, second = ([int(t) for t in rng.choice(V, size=300, replace=False)] for _ in range(2))
    q = first[17]
    phrases = [[t] for t in first] + [[q, s, first[i]] for i, s in enumerate(second)]
    hists = [[1, 2, 3, 4, q], [1, 2, 3, q, second[0]], [1, 2, 3, q, second[299]], [1, 2, q, second[150], 5], [1, 2, 3, 4, 5], [q] * 5]
    return phrases, rng.uniform(-3, 6, size=600).astype(np.float32), hists


def random_list(V, count, seed=2):
    """`count` phrases of 1 .. 6 ids over 40 ids — prefixes, suffix overlaps and duplicates in plenty — and six histories
    of 12 such ids"""
    rng = np.random.default_rng(seed)
    ids = rng.choice(V, size=40, replace=False)
    phrases = [[int(t) for t in rng.choice(ids, size=rng.integers(1, 7))] for _ in range(count)]
    return phrases, rng.uniform(-3, 6, size=count).astype(np.float32), [[int(t) for t in rng.choice(ids, size=12)] for _ in range(6)]
