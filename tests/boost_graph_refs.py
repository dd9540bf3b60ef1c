"""Revocable phrase boosting (include/fwamd.h: fw_boost_create_revocable) restated in Python from the wording of the
contract alone — a dict trie, a breadth-first pass for the failure links, np.float32 arithmetic in the stated order — and
what its tests share beside it: the ctypes plumbing, and one list and one set of histories that the host and the GPU tests
both walk."""
import ctypes as C
from collections import deque

import numpy as np

import boost_refs as br
from faster_whisper_amd import _lib

F = np.float32


class Graph:
    """child[u] {id: node}, G, E, val, fail per node; node 0 is the root"""

    def __init__(self, phrases, boosts):
        child, w, term, parent = [{}], [F(0)], [False], [0]
        for p, b in zip(phrases, boosts):
            u, b = 0, F(b)
            for t in p:
                v = child[u].get(int(t))
                if v is None:
                    v = len(child)
                    child[u][int(t)] = v
                    child.append({}), w.append(b), term.append(False), parent.append(u)
                elif b > w[v] or (b == w[v] and not np.signbit(b)):
                    w[v] = b
                u = v
            term[u] = True
        n = len(child)
        G, E, fail = [F(0)] * n, [F(0)] * n, [0] * n
        for v in range(1, n):   # (a parent is created in front of its children)
            through = F(G[parent[v]] + w[v])
            G[v], E[v] = (F(0), through) if term[v] else (through, F(0))   # (E holds C(v) for now)
        queue = deque([0])
        while queue:
            u = queue.popleft()
            for t, v in child[u].items():
                f = fail[u]
                while f and t not in child[f]:
                    f = fail[f]
                fail[v] = child[f].get(t, 0) if u else 0
                E[v] = F(E[v] + E[fail[v]])
                queue.append(v)
        self.child, self.G, self.E, self.fail = child, G, E, fail
        self.val = [F(g + e) for g, e in zip(G, E)]

    def state(self, hist, ts_begin):
        """the deepest node whose string is a suffix of the history's text ids"""
        t, s = [int(x) for x in hist if x < ts_begin], 0
        for k in range(1, min(len(t), 32) + 1):
            u = 0
            for x in t[len(t) - k:]:
                u = self.child[u].get(x)
                if u is None:
                    break
            else:
                s = u
        return s

    def step(self, s, v):
        """u' of the contract: where id v leads from state s"""
        while s and v not in self.child[s]:
            s = self.fail[s]
        return self.child[s].get(v, 0)

    def rows(self, logits, hists, eot, ts_begin):
        out = np.array(logits, dtype=np.float32, copy=True)
        for r, h in enumerate(hists):
            s = self.state(h, ts_begin)
            chain = [s]
            while chain[-1]:
                chain.append(self.fail[chain[-1]])
            edge_ids = {v for u in chain for v in self.child[u] if v <= eot}
            for v in range(eot + 1):
                if v in edge_ids or self.G[s] != 0:
                    out[r, v] = F(out[r, v] + F(self.val[self.step(s, v)] - self.G[s]))
        return out


# ---- the library side ----
def create_rc(n_vocab, phrases, boosts):
    """fw_boost_create_revocable on a list -> (status code, handle); the caller frees a handle it got"""
    flat, offs = br.ragged(phrases)
    b = np.asarray(list(boosts) or [0.0], dtype=np.float32)
    h = C.c_void_p()
    return _lib.load().fw_boost_create_revocable(int(n_vocab), _lib.as_i32p(flat), _lib.as_i32p(offs), len(phrases),
                                                 _lib.as_f32p(b), C.byref(h)), h


class Revocable(br.Boost):
    def __init__(self, n_vocab, phrases, boosts):
        rc, self.handle = create_rc(n_vocab, phrases, boosts)
        _lib.check(rc)


def rows(logits, hists, boost, eot, ts_begin, model_handle=None, form=0, K=1, done=None):
    """fw_test_boost_graph_rows_host, or with a model's handle ONE launch of dec_boost_graph_kernel -> the whole logits"""
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = br.ragged(hists)
    geo = (out.shape[0], out.shape[1], eot, ts_begin, _lib.ptr(flat), _lib.ptr(offs))
    if model_handle is None:
        _lib.check(_lib.load().fw_test_boost_graph_rows_host(_lib.ptr(out), *geo, boost.handle))
    else:
        dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
        _lib.check(_lib.load().fw_test_boost_graph_rows(model_handle, _lib.ptr(out), *geo, K, None if dn is None else _lib.ptr(dn),
                                                        form, boost.handle))
    return out


def geometry(V):
    """(<eot>, first timestamp) a few dozen below V"""
    return V - 40, V - 30


def edge_list(V, n_text_ctx=448):
    """(phrases, boosts, histories) for a vocabulary of V ids with geometry(V): shared prefixes ([a, b, c], [a, b, d]), a
    phrase that is a prefix of another ([a, b]) and one that is a proper suffix of another ([b, c]: the E of a failure
    target), [p, p, q] against [p, p, p], a 32-token phrase, a one-token phrase, 600 first tokens and a node Q with 300
    out-edges, some of them ids that are first tokens too; histories: empty, one id, timestamps between the text, exactly 32
    and more than 32 text ids, a text id behind 70 timestamps (the second ballot round), one of n_text_ctx - 1 ids"""
    rng = np.random.default_rng(V)
    eot, ts = geometry(V)
    a, b, c, d, p, q, z = 33, 34, 35, 36, 40, 41, 42
    long = [int(t) for t in rng.choice(np.arange(100, 400), size=32, replace=False)]
    first = [int(t) for t in rng.choice(np.arange(50, eot), size=600, replace=False)]
    Q, second = first[17], [int(t) for t in rng.choice(np.arange(50, eot), size=300, replace=False)]
    phrases = [[a, b, c], [a, b, d], [a, b], [b, c], [p, p, q], long, [z], [long[5], long[6], z], [eot - 1, 0]]
    phrases += [[t] for t in first[:300]] + [[t, a] for t in first[300:]] + [[Q, t, b] for t in second]
    boosts = list(rng.uniform(-2, 6, size=len(phrases)).astype(np.float32))
    stamp = lambda i: ts + i % (V - ts)
    text = lambda n: [int(t) for t in rng.integers(0, 30, size=n)]
    hists = [[], [a], [z], [b], [a, b], [7, a, b], [p, p, p], [p, p], [a, stamp(2), b, stamp(0), stamp(5)], [stamp(1), stamp(2)],
             text(1) + long[:31], long, text(8) + long, text(20) + long[:20], text(3) + long[:7], [a] + [stamp(i) for i in range(70)],
             text(1) + [Q], [Q, second[299]], [Q, second[0], 3], text(n_text_ctx - 4) + [stamp(3), a, b]]
    return phrases, boosts, hists
