"""dec_boost_trie_kernel alone, through fw_test_boost_trie_rows (include/fwamd_test.h), against the numpy restatement of
phrase boosting (tests/boost_refs.py): the WHOLE logits of every launch are compared as uint32 — the boosted ids carry one
fp32 add, every other value (the next row's first ids behind a boosted V - 1 among them) the caller's bits.  Both row forms,
vocabularies of all four residues mod 4 (a row starts at r * V floats), on the lists of tests/boost_trie_refs.py; for lists
fw_boost_create takes too, dec_boost_kernel's rows are the same bits."""
import numpy as np
import pytest

import boost_refs as br
import boost_trie_refs as bt

pytestmark = pytest.mark.gpu

FORMS = [0, 1]


@pytest.fixture(scope="module")
def handle():
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    assert cfg.n_vocab == 1913
    model = Whisper("synthetic:boost-trie", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    yield model._replicas[0].handle
    del model


def _check(handle, V, phrases, boosts, hists, form):
    """the rows of one history length per launch (form 0 takes one n); returns the logits and the reference"""
    lg = (np.random.default_rng(len(hists)).standard_normal((len(hists), V)) * 4).astype(np.float32)
    want = br.boost_rows(lg, phrases, boosts, hists)
    boost = bt.LargeBoost(V, phrases, boosts)
    old = br.Boost(V, phrases, boosts) if V == 1913 and len(phrases) <= br.MAX_PHRASES else None
    for n in sorted({len(h) for h in hists}):
        sel = [r for r, h in enumerate(hists) if len(h) == n]
        got = bt.rows(lg[sel], [hists[r] for r in sel], boost, handle, form)
        assert np.array_equal(br.bits(got), br.bits(want[sel])), (n, np.argwhere(br.bits(got) != br.bits(want[sel]))[:8])
        if old is not None:
            assert np.array_equal(br.bits(br.rows_gpu(handle, lg[sel], [hists[r] for r in sel], old, form)), br.bits(got))
    return lg, want


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("V", [1913, 1914, 1915, 1916])
def test_edges_at_every_row_alignment(handle, V, form):
    lg, want = _check(handle, V, *bt.edge_list(V), form)
    assert want[0, 33] == np.float32(lg[0, 33] + np.float32(1.5))      # [a, a, a] behind [a, a]: once
    assert want[1, 42] == np.float32(lg[1, 42] + np.float32(2.5))      # z from three depths: the largest
    for r in (12, 13, 14):                                            # 32, 40 ids: the 31 that count still match
        assert want[r, V - 1] == np.float32(lg[r, V - 1] + np.float32(3.0))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("make", [lambda: bt.wide_list(1913), lambda: bt.wide_list(1915, seed=3), lambda: bt.random_list(1913, 700),
                                  lambda: bt.random_list(1914, 5000)], ids=["wide", "wide-odd", "random-700", "random-5000"])
def test_wide_nodes_and_random_lists(handle, make, form):
    phrases, boosts, hists = make()
    _check(handle, 1913 + max(0, max(max(p) for p in phrases) - 1912), phrases, boosts, hists, form)


def test_done_chunks_and_rows_without_target_keep_their_bits(handle):
    """R = 10, K = 5 in the step form, six ragged rows in the score form: the skipped rows keep the caller's bits"""
    rng = np.random.default_rng(7)
    phrases, boosts = [[20, 21, 22], [21], [0]], [2.0, -1.0, 0.75]
    boost = bt.LargeBoost(1913, phrases, boosts)
    hists = [[int(t) for t in rng.integers(19, 23, size=5)] for _ in range(10)]
    lg = (rng.standard_normal((10, 1913)) * 4).astype(np.float32)
    want = br.boost_rows(lg, phrases, boosts, hists)
    for done in ([0, 1], [1, 0]):
        keep = np.repeat(np.asarray(done, dtype=bool), 5)[:, None]
        assert np.array_equal(br.bits(bt.rows(lg, hists, boost, handle, 0, K=5, done=done)), br.bits(np.where(keep, lg, want)))
    hists = [[], [20], [9, 20, 21], [21] * 40, [20, 21], list(range(100, 547))]
    done = np.asarray([0, 0, 0, 0, 1, 0], dtype=bool)
    want = np.where(done[:, None], lg[:6], br.boost_rows(lg[:6], phrases, boosts, hists))
    assert np.array_equal(br.bits(bt.rows(lg[:6], hists, boost, handle, 1, done=done.astype(np.int32))), br.bits(want))
