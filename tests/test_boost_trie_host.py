"""fw_boost_create_large on the host (no GPU): its limits and FW_EINVAL cases, the compiled table as a function of the
(phrase, boost) SET, and the trie walked in plain C++ (fw_test_boost_trie_rows_host) against the numpy restatement of phrase
boosting (tests/boost_refs.py) and, for lists fw_boost_create takes too, against its table's walk — bit for bit."""
import numpy as np
import pytest

import boost_refs as br
import boost_trie_refs as bt
from faster_whisper_amd import _lib

MAX_PHRASES, MAX_TOKENS = 65536, 524288


@pytest.mark.parametrize("phrases, boost, ok", [
    ([[1]] * MAX_PHRASES, 1.0, True), ([[1]] * (MAX_PHRASES + 1), 1.0, False),
    ([[3] * 32] * (MAX_TOKENS // 32), 1.0, True), ([[3] * 32] * (MAX_TOKENS // 32) + [[3]], 1.0, False),
    ([[3] * 33], 1.0, False), ([[1], []], 1.0, False), ([[10]], 1.0, False), ([[-1]], 1.0, False),
    ([[1]], float("nan"), False), ([[1]], float("inf"), False), ([], 1.0, True),
])
def test_limits_and_refusals(phrases, boost, ok):
    rc, h = bt.create_rc(10, phrases, [boost] * len(phrases))
    assert rc == (_lib.FW_OK if ok else _lib.FW_EINVAL) and bool(h) == ok
    if h:
        _lib.load().fw_boost_free(h)
    assert bt.create_rc(0, [[0]], [1.0])[0] == _lib.FW_EINVAL


def test_table_depends_on_the_set_alone():
    phrases, boosts, _ = bt.random_list(1913, 500)
    base = bt.table(bt.LargeBoost(1913, phrases, boosts))
    twice = list(np.random.default_rng(0).permutation(len(phrases))) + list(range(100))
    assert np.array_equal(base, bt.table(bt.LargeBoost(1913, [phrases[i] for i in twice], [boosts[i] for i in twice])))
    other = boosts.copy()
    other[int(np.argmax(boosts))] += 1
    assert not np.array_equal(base, bt.table(bt.LargeBoost(1913, phrases, other)))
    # the header word that says which form a table holds: the entry list has n_vocab there
    assert base[3] == -1 and bt.table(br.Boost(1913, phrases, boosts))[3] == 1913


@pytest.mark.parametrize("make", [lambda: bt.edge_list(1913), lambda: bt.edge_list(1914), lambda: bt.wide_list(1913),
                                  lambda: bt.random_list(1913, 700), lambda: bt.random_list(1913, 5000)],
                         ids=["edge", "edge-even", "wide", "random-700", "random-5000"])
def test_host_walk_is_the_definition(make):
    phrases, boosts, hists = make()
    V = 1913 + (max(max(p) for p in phrases) == 1913)
    lg = (np.random.default_rng(4).standard_normal((len(hists), V)) * 4).astype(np.float32)
    want = br.boost_rows(lg, phrases, boosts, hists)
    assert np.array_equal(br.bits(bt.rows(lg, hists, bt.LargeBoost(V, phrases, boosts))), br.bits(want))
    if len(phrases) <= br.MAX_PHRASES and sum(len(p) for p in phrases) <= br.MAX_TOKENS:
        assert np.array_equal(br.bits(br.rows_host(lg, hists, br.Boost(V, phrases, boosts))), br.bits(want))
