"""generate / score with a boost list beyond fw_boost_create's limits (2 000 phrases: fw_boost_create_large, a ValueError
before there was one), end to end on the setup of tests/test_gpu_boost.py: score reproduces the greedy call and a beam call
returns; a small list in the large form gives the old form's bits; equal large lists share a decode run, another does not,
and every call gets its solo result."""
import numpy as np
import pytest

from test_gpu_alternatives import MODES, _batches, _behind_a_blocker, _group_model, _kw, _prompt, _same
from test_gpu_boost import A, B, C, _score_reproduces, setup  # noqa: F401

pytestmark = pytest.mark.gpu


def _catalogue(cfg, count=2000, seed=0):
    """`count` phrases over the text ids 10 .. 400 that no rule of the setup forbids, [A, B, C] among them"""
    from test_gpu_alternatives import _suppress
    rng = np.random.default_rng(seed)
    ids = np.asarray([t for t in range(10, 400) if t not in set(_suppress(cfg)) | set(cfg.suppress_begin)])
    return [[A, B, C]] + [[int(t) for t in rng.choice(ids, size=rng.integers(1, 4))] for _ in range(count - 1)]


def test_a_catalogue_decodes_and_score_reproduces_it(setup):
    cfg, model, enc = setup
    phrases = _catalogue(cfg)
    assert model.boost_list(phrases, [3.0] * len(phrases)).large
    _score_reproduces(cfg, model, enc, phrases, [3.0] * len(phrases))
    kw = _kw(cfg, "beam5")
    res = model.generate(enc, [_prompt(cfg)] * 3, boost=model.boost_list(phrases, [3.0] * len(phrases)), **kw)
    assert [r.sequences_ids for r in res] != [r.sequences_ids for r in model.generate(enc, [_prompt(cfg)] * 3, **kw)]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_small_list_in_the_large_form_gives_the_old_bits(setup, mode):
    from faster_whisper_amd.backend import BoostList
    cfg, model, enc = setup
    phrases, strengths = _catalogue(cfg, 300, seed=1), list(np.random.default_rng(1).uniform(-2, 5, size=300))
    old, large = model.boost_list(phrases, strengths), BoostList(cfg.n_vocab, phrases, strengths, large=True)
    assert large.large and not old.large
    kw = dict(_kw(cfg, mode), return_alternatives=3)
    _same(model.generate(enc, [_prompt(cfg)] * 3, boost=large, **kw), model.generate(enc, [_prompt(cfg)] * 3, boost=old, **kw),
          alternatives=True)


def test_equal_large_lists_share_a_run_and_another_does_not():
    cfg, model = _group_model()
    prompt = _prompt(cfg)
    base = dict(beam_size=5, num_hypotheses=3, max_length=len(prompt) + 10, length_penalty=0.0, return_scores=True,
                return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_alternatives=3)
    phrases = _catalogue(cfg)
    one = model.boost_list(phrases, [4.0] * len(phrases))
    twin = model.boost_list(phrases[::-1], [4.0] * len(phrases))
    other = model.boost_list(phrases, [4.5] * len(phrases))
    kws = [dict(base, boost=one), dict(base, boost=twin), dict(base, boost=other)]
    batches = _batches((3, 2, 3))
    solo = [model.generate(model.encode_pcm(b), [prompt] * len(b), **kw) for b, kw in zip(batches, kws)]
    out, runs = _behind_a_blocker(model, cfg, batches, [prompt] * 3, kws)
    assert runs == 2
    for o, s in zip(out, solo):
        _same(o, s, alternatives=True)
