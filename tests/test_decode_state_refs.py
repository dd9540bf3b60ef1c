"""The references of tests/decode_state_refs.py checked on their own (CPU only): the beam-update reference against
brute-force enumeration where nothing is pruned, the align reference against the oracle's median filter, the embedding
reference against torch half addition."""
import itertools

import numpy as np

from decode_state_refs import (FIN_CAP, align_post_fp32, align_post_ref, beam_state, beam_update_ref, embed_ref,
                               finished_list, run_chain, toy_table)


def test_beam_ref_equals_exhaustive_enumeration():
    """V = 3 (token 2 = <eot>), K = 16, budget 3: 2K = 32 candidates hold every continuation, so nothing is pruned and
    the finished set is ALL 15 sequences (1 + 2 + 12), in finishing order, with their cum and score"""
    V, K, budget, eot, lp_pow = 3, 16, 3, 2, 0.6
    logp = toy_table(3, V)
    final = run_chain(logp, 1, K, 8, 2, budget, FIN_CAP - K, lp_pow, eot)
    got = finished_list(final, 0)
    # brute force: every sequence that ends in <eot> or reaches the budget; cum = sequential fp32 sum
    want = []
    for n in range(budget):                       # finishing step
        at_step = []
        for seq in itertools.product(range(V), repeat=n + 1):
            if eot in seq[:-1] or (seq[-1] != eot and n + 1 < budget):
                continue
            cum, prev = np.float32(0), V
            for t in seq:
                cum = np.float32(cum + logp[prev, t])
                prev = t
            toks = [t for t in seq if t != eot]
            at_step.append((toks, float(cum), float(cum) / max(len(toks), 1) ** lp_pow))
        assert len({c for _, c, _ in at_step}) == len(at_step)       # no ties: the order within a step is decided
        want += sorted(at_step, key=lambda h: -h[1])
    assert len(want) == 15
    assert [g[0] for g in got] == [w[0] for w in want]
    assert [g[1] for g in got] == [w[1] for w in want]
    np.testing.assert_allclose([g[2] for g in got], [w[2] for w in want], rtol=1e-15)
    assert final["done"][0] == 1 and final["n_done"][0] == 1


def test_beam_ref_hand_cases():
    """the walk's branches on one hand-written step: K = 2, <eot> = 9; the candidates of row 0 / row 1 tie at -1"""
    K, NT, P, step, eot = 2, 8, 2, 1, 9
    st = beam_state(1, K, NT, step, P, [[4], [5]], [[0, 0], [1, 1]], [-0.5, -0.75], -7, -99.0)
    cv = np.array([[-1.0, -2.0, -3.0, -np.inf], [-1.0, -1.5, -np.inf, -np.inf]], np.float32)
    ct = np.array([[9, 6, 9, 0], [7, 9, 0, 0]], np.int32)
    # merged (2K = 4): (r0,-1,eot) (r1,-1,7) | (r1,-1.5,eot) (r0,-2,6): slot 0 finishes and takes the first non-eot
    # secondary (r0, 6), skipping the <eot> at -1.5 WITHOUT recording it; slot 1 lives
    out = beam_update_ref(st, cv, ct, K=K, P=P, step=step, budget=5, max_fin=4, lp_pow=1.0, eot=eot)
    assert finished_list(out, 0) == [([4], -1.0, -1.0)]
    assert out["hist2"][0, :, :2].tolist() == [[4, 6], [5, 7]]
    assert out["kvidx2"][0, :, :3].tolist() == [[0, 0, 0], [1, 1, 1]]
    assert out["cum2"][0].tolist() == [-2.0, -1.0] and out["cur_tok"].tolist() == [6, 7]
    assert (out["hist2"][1] == st["hist2"][1]).all() and (out["hist2"][0, :, 2:] == -7).all()
    assert out["done"][0] == 0 and out["n_done"][0] == 0
    # max_fin = 1: the chunk finishes, nothing but the finished list, n_fin, done and n_done changes
    fin = beam_update_ref(st, cv, ct, K=K, P=P, step=step, budget=5, max_fin=1, lp_pow=0.0, eot=eot)
    assert fin["done"][0] == 1 and fin["n_done"][0] == 1 and fin["n_fin"][0] == 1
    for k in ("hist2", "kvidx2", "cum2", "cur_tok"):
        assert np.array_equal(fin[k], st[k])
    # a chunk that is done on entry: untouched
    st["done"][0] = 1
    same = beam_update_ref(st, cv, ct, K=K, P=P, step=step, budget=5, max_fin=4, lp_pow=1.0, eot=eot)
    assert all(np.array_equal(same[k], st[k]) for k in st)


def test_align_ref_equals_oracle_median_filter():
    from oracle.whisper import _median_filter
    rng = np.random.default_rng(11)
    B, n_sel, cap, T = 2, 3, 7, 40
    x = rng.standard_normal((B, n_sel, cap, T))
    probs = np.exp(x) / np.exp(x).sum(axis=-1, keepdims=True)
    n_tok, nfr = [7, 4], [40, 23]
    for width in (1, 3, 7):
        mat = np.full((B, cap, T), 5.0)
        got = align_post_ref(probs, n_tok, nfr, width, mat)
        for b in range(B):
            w = probs[b, :, :n_tok[b], :nfr[b]]
            w = (w - w.mean(axis=-2, keepdims=True)) / w.std(axis=-2, keepdims=True)
            want = _median_filter(w, width).mean(axis=0)
            np.testing.assert_allclose(got[b, :n_tok[b], :nfr[b]], want, rtol=0, atol=1e-13)
            assert (got[b, n_tok[b]:] == 5.0).all() and (got[b, :, nfr[b]:] == 5.0).all()
        # and the float32 restatement is the same computation: it differs by float32 round-off only
        f32 = align_post_fp32(probs, n_tok, nfr, width, mat)
        assert np.abs(f32 - got).max() < 1e-4


def test_embed_ref_equals_torch_half_addition():
    import torch
    rng = np.random.default_rng(5)
    V, NT, d = 9, 6, 64
    emb = rng.standard_normal((V, d)).astype(np.float32)
    pos = (rng.standard_normal((NT, d)) * 4).astype(np.float32)
    tok = np.array([0, 8, 3, 3], np.int64)
    p = np.array([5, 0, 2, 2], np.int64)
    got = embed_ref(tok, emb, pos, p)
    # fp16 + fp16 in torch on the CPU: computed in float32, rounded once
    want = (torch.from_numpy(emb).half()[tok] + torch.from_numpy(pos).half()[p]).float().numpy()
    assert np.array_equal(got, want)
