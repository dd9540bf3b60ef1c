"""dec_boost_graph_kernel alone, through fw_test_boost_graph_rows (include/fwamd_test.h), against the host walk and the
Python restatement of the contract (tests/boost_graph_refs.py): the WHOLE logits of every launch are compared as uint32.
Both row forms, vocabularies of all four residues mod 4 (a row starts at r * V floats: every alignment of the dense pass,
its head and its tail), on the list and the histories of boost_graph_refs.edge_list, -inf logits among them."""
import numpy as np
import pytest

import boost_graph_refs as bg
import boost_refs as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    assert cfg.n_text_ctx == 448
    model = Whisper("synthetic:boost-graph", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    yield model._replicas[0].handle
    del model


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("V", [1027, 1028, 1029, 1030])
def test_kernel_host_walk_and_contract_agree(handle, V, form):
    phrases, boosts, hists = bg.edge_list(V)
    eot, ts = bg.geometry(V)
    lg = (np.random.default_rng(V).standard_normal((len(hists), V)) * 4).astype(np.float32)
    lg[:, ::7] = -np.inf
    graph, boost = bg.Graph(phrases, boosts), bg.Revocable(V, phrases, boosts)
    want = graph.rows(lg, hists, eot, ts)
    assert np.array_equal(br.bits(bg.rows(lg, hists, boost, eot, ts)), br.bits(want))
    held = [graph.G[graph.state(h, ts)] != 0 for h in hists]
    assert any(held) and not all(held)
    for n in sorted({len(h) for h in hists}):   # (form 0 takes one history length per launch)
        sel = [r for r, h in enumerate(hists) if len(h) == n]
        got = bg.rows(lg[sel], [hists[r] for r in sel], boost, eot, ts, handle, form)
        assert np.array_equal(br.bits(got), br.bits(want[sel])), (n, np.argwhere(br.bits(got) != br.bits(want[sel]))[:8])


def test_done_chunks_and_rows_without_target_keep_their_bits(handle):
    """R = 10, K = 5 in the step form, six ragged rows in the score form: the skipped rows keep the caller's bits"""
    rng = np.random.default_rng(7)
    V, (eot, ts) = 1029, bg.geometry(1029)
    phrases, boosts = [[20, 21, 22], [21], [22, 20]], [2.0, -1.0, 0.75]
    graph, boost = bg.Graph(phrases, boosts), bg.Revocable(V, phrases, boosts)
    hists = [[int(t) for t in rng.integers(19, 23, size=5)] for _ in range(10)]
    lg = (rng.standard_normal((10, V)) * 4).astype(np.float32)
    want = graph.rows(lg, hists, eot, ts)
    for done in ([0, 1], [1, 0]):
        keep = np.repeat(np.asarray(done, dtype=bool), 5)[:, None]
        got = bg.rows(lg, hists, boost, eot, ts, handle, 0, K=5, done=done)
        assert np.array_equal(br.bits(got), br.bits(np.where(keep, lg, want)))
    hists = [[], [20], [9, 20, 21], [21] * 40, [20, 21], [ts + 1, 22] + [ts] * 90]
    done = np.asarray([0, 0, 0, 0, 1, 0], dtype=bool)
    want = np.where(done[:, None], lg[:6], graph.rows(lg[:6], hists, eot, ts))
    assert np.array_equal(br.bits(bg.rows(lg[:6], hists, boost, eot, ts, handle, 1, done=done.astype(np.int32))), br.bits(want))
