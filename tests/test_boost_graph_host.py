"""fw_boost_create_revocable on the host (no GPU): its FW_EINVAL cases, the compiled table as a function of the (phrase,
boost) SET, the context graph walked in plain C++ (fw_test_boost_graph_rows_host) against the Python restatement of the
contract (tests/boost_graph_refs.py) bit for bit, and the telescoping identity along random hypotheses."""
import numpy as np
import pytest

import boost_graph_refs as bg
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
    rc, h = bg.create_rc(10, phrases, [boost] * len(phrases))
    assert rc == (_lib.FW_OK if ok else _lib.FW_EINVAL) and bool(h) == ok
    if h:
        _lib.load().fw_boost_free(h)
    assert bg.create_rc(0, [[0]], [1.0])[0] == _lib.FW_EINVAL


def test_table_depends_on_the_set_alone_and_on_the_form():
    phrases, boosts, _ = bt.random_list(1913, 500)
    base = bt.table(bg.Revocable(1913, phrases, boosts))
    twice = list(np.random.default_rng(0).permutation(len(phrases))) + list(range(100))
    assert np.array_equal(base, bt.table(bg.Revocable(1913, [phrases[i] for i in twice], [boosts[i] for i in twice])))
    other = boosts.copy()
    other[int(np.argmax(boosts))] += 1
    assert not np.array_equal(base, bt.table(bg.Revocable(1913, phrases, other)))
    assert not np.array_equal(base, bt.table(bt.LargeBoost(1913, phrases, boosts)))


def test_a_phrase_id_from_eot_up_and_another_vocabulary_are_refused():
    lg, boost = np.zeros((1, 1030), dtype=np.float32), bg.Revocable(1030, [[5, 6], [7, 990, 8]], [1.0, 2.0])
    assert bg.rows(lg, [[]], boost, 991, 1000).shape == lg.shape
    for V, eot in ((1030, 990), (1030, 989), (1029, 995)):
        with pytest.raises(ValueError, match="phrase 1 holds id 990" if V == 1030 else "vocabulary of 1030"):
            bg.rows(lg[:, :V], [[]], boost, eot, 1000)


@pytest.mark.parametrize("V", [1027, 1030])
def test_host_walk_is_the_contract(V):
    phrases, boosts, hists = bg.edge_list(V)
    eot, ts = bg.geometry(V)
    lg = (np.random.default_rng(4).standard_normal((len(hists), V)) * 4).astype(np.float32)
    lg[:, ::7] = -np.inf
    graph = bg.Graph(phrases, boosts)
    want = graph.rows(lg, hists, eot, ts)
    got = bg.rows(lg, hists, bg.Revocable(V, phrases, boosts), eot, ts)
    assert np.array_equal(br.bits(got), br.bits(want)), np.argwhere(br.bits(got) != br.bits(want))[:8]
    held = np.asarray([graph.G[graph.state(h, ts)] != 0 for h in hists])
    assert held.any() and not held.all() and np.array_equal(br.bits(got[:, eot + 1:]), br.bits(lg[:, eot + 1:]))
    assert np.isneginf(got[:, ::7]).all()


def test_the_deltas_of_a_hypothesis_telescope():
    """boosts in quarters, so every fp32 sum is exact: the deltas of a hypothesis's own tokens add up to the completions it
    banked plus what its last state holds"""
    rng = np.random.default_rng(3)
    ids = [int(t) for t in rng.choice(900, size=6, replace=False)]
    phrases = [[int(t) for t in rng.choice(ids, size=rng.integers(1, 5))] for _ in range(40)]
    boosts = rng.integers(-4, 16, size=40) / 4.0
    graph, boost = bg.Graph(phrases, boosts), bg.Revocable(1000, phrases, boosts)
    for _ in range(5):
        hyp = [int(t) for t in rng.choice(ids + [950, 951], size=60)]   # (950, 951: text that no phrase holds)
        out = bg.rows(np.zeros((60, 1000), dtype=np.float32), [hyp[:i] for i in range(60)], boost, 960, 970)
        s, banked = 0, 0.0
        for v in hyp:
            s = graph.step(s, v)
            banked += float(graph.E[s])
        assert sum(float(out[i, v]) for i, v in enumerate(hyp)) == banked + float(graph.G[s]) and banked != 0
