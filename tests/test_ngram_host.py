"""Language-model fusion on the host (no GPU): the plain C++ walk of the compiled table against the float64 restatement of
tests/ngram_refs.py, what fw_ngram_create refuses, byte-equal tables, and the two ways to an NgramLM."""
import copy
import math

import numpy as np
import pytest

import ngram_refs as nr
from faster_whisper_amd import _lib
from faster_whisper_amd.ngram import BOS, EOS, UNK, NgramLM


@pytest.mark.parametrize("N", [1, 2, 3, 5])
@pytest.mark.parametrize("V", [1021, 1022, 1023, 1024])
def test_host_walk_against_the_reference(V, N):
    eot, tsb = V - 120, V - 80
    m, hists = nr.model_of_order(N, V, eot, tsb)
    logits = nr.logits_of(len(hists), V)
    got = nr.rows_host(logits, hists, nr.Model(m), eot, tsb)
    nr.check(got, logits, *nr.fused_rows(logits, m, hists, eot, tsb))


def _with(m, order, gram, value):
    m = copy.deepcopy(m)
    m["grams"][order - 1][gram] = value
    return m


BASE = nr.model_of_order(3, 1000, 900, 940)[0]
REFUSED = {
    "order 0": dict(BASE, order=0),
    "order 6": dict(BASE, order=6),
    "id outside": _with(BASE, 2, (5, 1001), (-1.0, 0.0)),
    "negative id": _with(BASE, 1, (-1,), (-1.0, 0.0)),
    "BOS second": _with(BASE, 2, (5, 1000), (-1.0, 0.0)),
    "BOS with a probability": _with(BASE, 1, (1000,), (-1.0, -1.0)),
    "eos inside a context": _with(BASE, 3, (5, 900, 6), (-1.0, 0.0)),
    "infinite p": _with(BASE, 2, (5, 6), (-math.inf, 0.0)),
    "nan back-off": _with(BASE, 1, (4,), (-1.0, math.nan)),
    "infinite unk": dict(BASE, unk=-math.inf),
    "nan scale": dict(BASE, scale=math.nan),
    "infinite bonus": dict(BASE, bonus=math.inf),
    "eos outside": dict(BASE, eos=1000),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_create_refuses(name):
    rc, h = nr.create_rc(REFUSED[name])
    assert rc == _lib.FW_EINVAL and not h.value, _lib.load().fw_last_error()


def test_create_refuses_duplicates_null_pointers_and_too_many_ngrams():
    lib, h = _lib.load(), nr.C.c_void_p()
    one, two = np.asarray([1, 2], dtype=np.int32), np.asarray([0, 2], dtype=np.int32)
    ids, same, val = np.asarray([5, 6, 5, 6], dtype=np.int32), np.asarray([5, 5], dtype=np.int32), np.zeros(4, dtype=np.float32) - 1
    args = lambda counts, i, p, b: (100, 2, _lib.as_i32p(counts), i, p, b, -9.0, 1.0, 0.0, 60, nr.C.byref(h))   # noqa: E731
    for bad in (args(two, _lib.as_i32p(ids), _lib.as_f32p(val), _lib.as_f32p(val)),          # (5, 6) twice
                args(np.asarray([2, 0], dtype=np.int32), _lib.as_i32p(same), _lib.as_f32p(val), _lib.as_f32p(val)),
                args(one, None, _lib.as_f32p(val), _lib.as_f32p(val)), args(one, _lib.as_i32p(ids), _lib.as_f32p(val), None),
                args(np.asarray([0, (1 << 20) + 1], dtype=np.int32), _lib.as_i32p(ids), _lib.as_f32p(val), _lib.as_f32p(val))):
        assert lib.fw_ngram_create(*bad) == _lib.FW_EINVAL and not h.value


def test_equal_arguments_give_equal_tables_and_the_strength_is_part_of_them():
    m = nr.model_of_order(3, 1021, 901, 941)[0]
    a, b = nr.Model(m).table(), nr.Model(copy.deepcopy(m)).table()
    assert a.size % 4 == 0 and np.array_equal(a, b)
    assert not np.array_equal(a, nr.Model(m, scale=nr.f32(0.8)).table())
    assert not np.array_equal(a, nr.Model(m, bonus=nr.f32(0.4)).table())


ARPA = """\\data\\
ngram 1=5
ngram 2=2

\\1-grams:
-99 <s> -0.5
-1.0 </s>
-2.0 <unk>
-0.25 17 -0.125
-0.75 42
\\2-grams:
-0.5 <s> 17
-0.1 17 </s>
\\end\\
"""


def test_from_arpa():
    lm = NgramLM.from_arpa(ARPA)
    ln10 = math.log(10.0)
    assert lm.order == 2 and lm.unk_logprob == -2.0 * ln10
    assert lm.grams[0] == {(BOS,): (0.0, -0.5 * ln10), (EOS,): (-ln10, 0.0), (17,): (-0.25 * ln10, -0.125 * ln10),
                           (42,): (-0.75 * ln10, 0.0)}
    assert lm.grams[1] == {(BOS, 17): (-0.5 * ln10, 0.0), (17, EOS): (-0.1 * ln10, 0.0)}
    assert lm.score([BOS], 17) == -0.5 * ln10 and lm.score([17], 42) == -0.125 * ln10 + -0.75 * ln10
    counts, ids, lp, _ = lm.arrays(100, 60)
    assert counts.tolist() == [4, 2] and ids.tolist() == [100, 60, 17, 42, 100, 17, 17, 60] and lp[0] == 0.0
    assert UNK not in {w for level in lm.grams for g in level for w in g}


def test_train_sums_to_one_and_compiles():
    seqs = [[5, 6, 7, 5, 6], [5, 6, 9], [7, 5, 9, 9, 6]]
    lm = NgramLM.train(seqs, 3)
    events = sorted({t for s in seqs for t in s}) + [EOS]
    contexts = {(BOS,) + tuple(s)[:i] for s in seqs for i in range(len(s) + 1)} | {tuple(s)[i:j] for s in seqs
                                                                                  for i in range(len(s)) for j in range(i, len(s) + 1)}
    for ctx in contexts:
        unk = lm.score(ctx, "never seen")
        total = sum(math.exp(lm.score(ctx, w)) for w in events) + math.exp(unk)
        assert abs(total - 1.0) < 1e-9, (ctx, total)
    counts, *_ = lm.arrays(100, 60)
    assert counts.tolist() == [len(level) for level in lm.grams]
    m = dict(order=3, n_vocab=100, eos=60, unk=lm.unk_logprob, scale=1.0, bonus=0.0,
             grams=[{tuple({BOS: 100, EOS: 60}.get(w, w) for w in g): v for g, v in level.items()} for level in lm.grams])
    assert nr.Model(m).table()[0] == 3
