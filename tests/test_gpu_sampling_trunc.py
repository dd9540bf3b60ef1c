"""Truncated sampling end to end (include/fwamd.h: fw_generate_trunc; generate(top_k=, top_p=)): the limits act on the draw
and on nothing else, a truncating call shares decode runs with other sampling calls whatever their limits, and every caller
gets its solo result bit for bit.  micro geometry, peaked synthetic weights (a few ids carry most of the mass at every step,
so that a nucleus closes inside the eight alternatives a call can return)."""
import math

import numpy as np
import pytest

from conftest import bench_audio
from test_gpu_sampling_runs import _batches, _behind_blocker, _prompt, _same

pytestmark = pytest.mark.gpu

N_ALT = 8
MARGIN = 1e-2               # as tests/sampling_trunc_refs.py: no summation order moves an id across a cut this far away


@pytest.fixture(scope="module")
def env():
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    w = synthetic_weights(cfg, seed=7, peaked=True)
    model = Whisper("synthetic:micro", device="cuda", files={"config": cfg, "weights": w}, max_batch_size=3, max_beam_size=5,
                    inter_threads=5)
    model.set_decode_lanes(1)
    batch = [bench_audio(480000, seed=60), bench_audio(250000, seed=61)]
    return cfg, model, batch, model.encode_pcm(batch)


def _kw(cfg, prompt, nh=1, T=1.0, seed=3, n_new=24, **more):
    return dict(beam_size=1, num_hypotheses=nh, sampling_topk=0, sampling_temperature=T, seed=seed, max_length=len(prompt) + n_new,
                suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_scores=True, return_no_speech_prob=True,
                return_alternatives=N_ALT, **more)


def _positions(res):
    """(id, its log-prob, the alternatives of its position) of every returned token and closing <eot> of a result list"""
    for r in res:
        for h, ids in enumerate(r.sequences_ids):
            for t, tok in enumerate(ids):
                yield tok, r.token_logprobs[h][t], r.token_alternatives[h][t]


def _ends(cfg, res):
    for r in res:
        for h in range(len(r.sequences_ids)):
            if r.end_alternatives[h] is not None:
                yield cfg.eot, r.end_logprobs[h], r.end_alternatives[h]


@pytest.mark.parametrize("top_k", [1, 2, 5])
def test_top_k_keeps_every_id_among_its_first_alternatives(env, top_k):
    cfg, model, batch, enc = env
    prompt = _prompt(cfg, 0)
    res = model.generate(enc, [prompt] * 2, top_k=top_k, **_kw(cfg, prompt, nh=3))
    n = 0
    for tok, lp, alts in list(_positions(res)) + list(_ends(cfg, res)):
        first = [i for i, _ in alts[:top_k]]
        assert tok in first, (top_k, tok, alts)
        # identity (1) of fw_generate_alt: the recorded log-prob is the plain one, bit for bit that of the alternative
        assert np.float32(lp).tobytes() == np.float32(dict(alts)[tok]).tobytes()
        n += 1
    assert n >= 6
    if top_k > 1:   # the limit is not the arg-max in disguise
        assert any(tok != alts[0][0] for tok, _, alts in _positions(res))


def test_top_k_1_is_the_greedy_call(env):
    cfg, model, batch, enc = env
    prompt = _prompt(cfg, 0)
    kw = _kw(cfg, prompt)
    got = model.generate(enc, [prompt] * 2, top_k=1, **kw)
    greedy = model.generate(enc, [prompt] * 2, **dict(kw, sampling_topk=1))
    for a, b in zip(got, greedy):
        assert a.sequences_ids == b.sequences_ids and a.token_logprobs == b.token_logprobs and a.end_logprobs == b.end_logprobs
        assert a.token_alternatives == b.token_alternatives


def _nucleus_of(alts, p):
    """the nucleus from the eight alternatives' log-probs (float64; they are log-probs of the whole distribution at T = 1, so
    exp(lp) is the mass itself and Z = 1): the ids kept, or None when it does not close inside the eight with the margin"""
    lp = np.asarray([v for _, v in alts], np.float64)
    w = np.where(np.isfinite(lp), np.exp(lp), 0.0)
    ahead = np.cumsum(w) - w
    total = w.sum()
    if total < p + MARGIN or np.abs(ahead - p).min() < MARGIN:
        return None
    keep = ahead < p
    keep[0] = True
    return [i for (i, _), k in zip(alts, keep) if k]


def test_nucleus_keeps_every_id_inside_it(env):
    cfg, model, batch, enc = env
    prompt = _prompt(cfg, 0)
    p = 0.8
    res = []
    for seed in (3, 4, 5):
        res += model.generate(enc, [prompt] * 2, top_p=p, **_kw(cfg, prompt, nh=3, seed=seed))
    pos = list(_positions(res)) + list(_ends(cfg, res))
    ok = 0
    sizes = []
    for tok, lp, alts in pos:
        kept = _nucleus_of(alts, p)
        if kept is None:
            continue
        ok += 1
        sizes.append(len(kept))
        assert tok in kept, (tok, kept, alts)
    print(f"nucleus p = {p}: {ok} of {len(pos)} positions close inside the {N_ALT} alternatives with the margin; "
          f"sizes {sorted(set(sizes))}")
    assert 2 * ok >= len(pos) and len(pos) >= 20
    assert any(tok != alts[0][0] for tok, _, alts in pos)


def test_divergence_identity(env):
    """a call with limits and the same call without share their ids up to the first position where they differ; there the plain
    call's id is outside the truncated call's kept set (read off its alternatives, equal in both calls up to there)"""
    cfg, model, batch, enc = env
    prompt = _prompt(cfg, 0)
    top_k = 2
    diverged = agreed5 = 0
    for seed in range(20, 32):
        kw = _kw(cfg, prompt, seed=seed)
        plain = model.generate(enc, [prompt] * 2, **kw)
        trunc = model.generate(enc, [prompt] * 2, top_k=top_k, **kw)
        for a, b in zip(plain, trunc):
            # (a hypothesis closed by <eot> has that step too; one cut at the budget has not)
            ia = a.sequences_ids[0] + ([cfg.eot] if a.end_alternatives[0] is not None else [])
            ib = b.sequences_ids[0] + ([cfg.eot] if b.end_alternatives[0] is not None else [])
            alts_a = a.token_alternatives[0] + [a.end_alternatives[0]]
            alts_b = b.token_alternatives[0] + [b.end_alternatives[0]]
            t = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), None)
            if t is None:
                assert ia == ib
                agreed5 += len(ia) >= 5
                continue
            diverged += 1
            agreed5 += t >= 5
            assert alts_a[:t + 1] == alts_b[:t + 1]                     # the same histories: the same distributions
            kept = [i for i, _ in alts_b[t][:top_k]]
            assert ib[t] in kept and ia[t] not in kept, (seed, t, ia[t], ib[t], alts_b[t])
    print(f"top_k = {top_k}: {diverged} pairs diverged, {agreed5} agreed for five positions or more")
    assert diverged >= 1 and agreed5 >= 1


def test_calls_with_different_limits_share_a_run_and_equal_solo(env):
    cfg, model, _, _ = env
    prompt = _prompt(cfg, 0)
    limits = [(0, 1.0), (5, 1.0), (0, 0.8), (3, 0.9)]
    temps, seeds = (0.6, 1.0, 1.0, 0.8), (7, 7, 11, 12)
    batches = _batches((2, 1, 3, 1))
    kws = []
    for (k, p), T, s in zip(limits, temps, seeds):
        kw = dict(_kw(cfg, prompt, nh=3, T=T, seed=s, n_new=12))
        if (k, p) != (0, 1.0):
            kw.update(top_k=k, top_p=p)
        kws.append(kw)
    solo = [model.generate(model.encode_pcm(b), [prompt] * len(b), **kw) for b, kw in zip(batches, kws)]

    def same(got, want, what):
        _same(got, want, what)
        for a, b in zip(got, want):
            assert a.token_alternatives == b.token_alternatives and a.end_alternatives == b.end_alternatives, what

    same(model.generate(model.encode_pcm(batches[3]), [prompt], **kws[3]), solo[3], "the same truncated call again")
    out, runs = _behind_blocker(model, cfg, batches, [prompt] * 4, kws)
    st = model.decode_stats()
    print(f"4 sampling calls with limits {limits} -> {runs} decode runs, largest {st['max_run_chunks']} chunks")
    assert runs < 4 and st["max_run_chunks"] > 3      # calls shared a run (the largest call has 3 chunks; all four: 7)
    for i in range(4):
        same(out[i], solo[i], f"call {i} {limits[i]}")


def test_wrong_limits_are_refused_before_anything_is_queued(env):
    cfg, model, batch, enc = env
    prompt = _prompt(cfg, 0)
    kw = _kw(cfg, prompt)
    st0 = model.decode_stats()
    bad = [dict(kw, top_k=-1), dict(kw, top_p=0.0), dict(kw, top_p=1.5), dict(kw, top_p=math.nan),
           dict(kw, beam_size=3, sampling_topk=1, top_k=5), dict(kw, beam_size=3, sampling_topk=1, top_p=0.9),
           dict(kw, sampling_topk=1, top_k=5), dict(kw, sampling_topk=1, top_p=0.9)]
    for b in bad:
        with pytest.raises(ValueError):
            model.generate(enc, [prompt] * 2, **b)
    with pytest.raises(ValueError):                                       # CTranslate2's own top-k keeps failing as it did
        model.generate(enc, [prompt] * 2, beam_size=1, sampling_topk=7)
    assert model.decode_stats() == st0
