"""Language-model fusion (include/fwamd.h: fw_ngram) restated in float64 from the wording of the contract, the per-element
bound of its N + 2 float32 roundings, the one model per order the kernel tests share, and wrappers of fw_ngram_create and
its three hooks.  A model here: dict(order, n_vocab, eos, unk, scale, bonus, grams) with grams[k - 1] = {ids: (p, bo)},
BOS = n_vocab, every value already rounded to float32."""
import ctypes as C

import numpy as np

from constrain_refs import ragged
from faster_whisper_amd import _lib

f32 = lambda x: float(np.float32(x))   # noqa: E731


def fused_rows(logits, m, hists, eot, ts_begin, skipped=()):
    """-> (logit + scale * score + bonus in float64, the bound per element); rows in `skipped` and ids > eot: (logit, 0)"""
    N, grams = m["order"], m["grams"]
    want, bound = logits.astype(np.float64), np.zeros(logits.shape)
    uni = np.full(eot + 1, m["unk"])
    for (v,), (p, _) in grams[0].items():
        if v <= eot:
            uni[v] = p
    for r, h in enumerate(hists):
        if r in skipped:
            continue
        s = [m["n_vocab"]] + [t for t in h if t < ts_begin]
        K = min(N - 1, len(s))
        score, terms, acc, mag = uni.copy(), np.abs(uni), 0.0, 0.0
        above = []                                   # (acc, |acc|) in front of level k, for k = K .. 1
        for k in range(K, 0, -1):
            above.append((acc, mag))
            bo = grams[k - 1].get(tuple(s[-k:]), (0.0, 0.0))[1]
            acc, mag = acc + bo, mag + abs(bo)
        score, terms = score + acc, terms + mag
        for k in range(1, K + 1):                    # the longer context overwrites the shorter
            a, g = above[K - k]
            for gram, (p, _) in grams[k].items():
                if gram[:-1] == tuple(s[-k:]):
                    score[gram[-1]], terms[gram[-1]] = a + p, g + abs(p)
        lg = want[r, :eot + 1].copy()
        want[r, :eot + 1] = lg + m["scale"] * score + m["bonus"]
        with np.errstate(invalid="ignore"):
            bound[r, :eot + 1] = (N + 3) * 2.0 ** -24 * (np.abs(lg) + abs(m["scale"]) * terms + abs(m["bonus"]))
    return want, bound


def check(got, logits, want, bound):
    """untouched ids (bound 0) and -inf logits bit for bit, every other id within its bound"""
    exact = (bound == 0) | np.isinf(logits)
    assert np.array_equal(got[exact].view(np.uint32), logits[exact].view(np.uint32))
    err = np.abs(got[~exact].astype(np.float64) - want[~exact])
    assert np.all(err <= bound[~exact]), float(np.max(err / bound[~exact]))


def model_of_order(N, V, eot, tsb, seed=3):
    """One model per order with: contexts of 1, 65 and 300 successors, an id explicit at two levels of one chain, a context
    that is only a path, n-grams that begin with BOS, eos among the successors -> (model, histories)"""
    rng = np.random.default_rng(seed + N)
    val = lambda: f32(-rng.uniform(0.1, 9.0))   # noqa: E731
    BOS, F = V, tuple(range(50, 50 + N - 1))
    grams = [dict() for _ in range(N)]
    for v in list(range(0, eot, 3)) + [eot]:
        grams[0][(v,)] = (val(), val() if N > 1 and v != eot else 0.0)
    if N > 1:
        grams[0][(BOS,)] = (0.0, val())
        for ctx, n in (((10,), 1), ((11,), 65), ((12,), 300), ((BOS,), 3)):
            for v in sorted(set(rng.choice(eot, size=n - 1, replace=False).tolist()) | {eot if n > 1 else 7})[:n]:
                grams[1][ctx + (v,)] = (val(), val() if N > 2 else 0.0)
        grams[1][(F[-1], 7)] = (val(), 0.0)                       # 7: explicit under c_1 and, below, under c_{N-1}
    if N > 2:
        for v in [7, eot] + list(range(200, 263)):
            grams[N - 1][F + (v,)] = (val(), 0.0)                 # (for N = 5: F[-2:] and F[-3:] exist only as a path)
        grams[1][F[-2:]] = (val(), val())                         # c_2 of that chain is an n-gram with a back-off
        grams[2][(60, 61, 9)] = (val(), 0.0)                      # 61 has no unigram: the context (61,) is only a path
        grams[2][(BOS, 70, 8)] = (val(), 0.0)
    long = [int(t) for pair in zip(rng.integers(0, eot, 20), rng.integers(tsb, V, 20)) for t in pair]
    if F:
        long[-2 * len(F)::2] = F                                  # ..., F[0], ts, F[1], ts: a timestamp last
    hists = [[], [10], [11], [12], [70], list(F), [60, 61], long, [11, 100], [100]]
    m = dict(order=N, n_vocab=V, eos=eot, unk=f32(-11.5), scale=f32(0.7), bonus=f32(0.3), grams=grams)
    return m, hists


def create_rc(m, **over):
    """fw_ngram_create -> (status code, handle); the caller frees a handle it got"""
    a = dict(m, **over)
    ids = np.asarray([t for level in a["grams"] for g in level for t in g] or [0], dtype=np.int32)
    lp = np.asarray([p for level in a["grams"] for p, _ in level.values()] or [0], dtype=np.float32)
    bo = np.asarray([b for level in a["grams"] for _, b in level.values()] or [0], dtype=np.float32)
    counts = np.asarray([len(level) for level in a["grams"]] + [0] * 5, dtype=np.int32)
    h = C.c_void_p()
    rc = _lib.load().fw_ngram_create(a["n_vocab"], a["order"], _lib.as_i32p(counts), _lib.as_i32p(ids), _lib.as_f32p(lp),
                                     _lib.as_f32p(bo), a["unk"], a["scale"], a["bonus"], a["eos"], C.byref(h))
    return rc, h


class Model:
    """a compiled model that frees itself"""

    def __init__(self, m, **over):
        rc, self.handle = create_rc(m, **over)
        _lib.check(rc)

    def table(self):
        n = C.c_int32()
        _lib.check(_lib.load().fw_test_ngram_table(self.handle, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        _lib.check(_lib.load().fw_test_ngram_table(self.handle, _lib.ptr(out), n.value, C.byref(n)))
        return out

    def __del__(self):
        if getattr(self, "handle", None):
            _lib.load().fw_ngram_free(self.handle)
            self.handle = None


def rows_host(logits, hists, lm, eot, ts_begin):
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = ragged(hists)
    _lib.check(_lib.load().fw_test_ngram_rows_host(_lib.ptr(out), out.shape[0], out.shape[1], eot, ts_begin, _lib.ptr(flat),
                                                   _lib.ptr(offs), lm.handle))
    return out


def rows_gpu(model_handle, logits, hists, lm, eot, ts_begin, form, K=1, done=None):
    """fw_test_ngram_rows: ONE launch of dec_ngram_kernel -> the whole logits as it left them"""
    out = np.ascontiguousarray(logits, dtype=np.float32).copy()
    flat, offs = ragged(hists)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    _lib.check(_lib.load().fw_test_ngram_rows(model_handle, _lib.ptr(out), out.shape[0], out.shape[1], eot, ts_begin,
                                              _lib.ptr(flat), _lib.ptr(offs), K, None if dn is None else _lib.ptr(dn), form,
                                              lm.handle, 0, None))
    return out


def logits_of(rows, V, seed=0):
    """random rows with -inf entries (one of them where every model has an explicit n-gram) and one row of zeros"""
    lg = (np.random.default_rng(seed).standard_normal((rows, V)) * 4).astype(np.float32)
    lg[:, [3, 7, V - 130, V - 1]] = -np.inf
    lg[rows // 2] = 0.0
    return lg
