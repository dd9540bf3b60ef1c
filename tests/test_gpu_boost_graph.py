"""generate / score with a revocable boost list (fw_boost_create_revocable) end to end, on the setup of
tests/test_gpu_boost.py: score reproduces the greedy call bit for bit; equal revocable lists share ONE decode run, a sticky
list of the same phrases and a plain call do not join it, and every call gets its solo bits; a phrase id from <eot> up is a
ValueError before anything is queued."""
import numpy as np
import pytest

from test_gpu_alternatives import _batches, _behind_a_blocker, _group_model, _kw, _prompt, _same
from test_gpu_boost import A, B, C, _bits, setup  # noqa: F401

pytestmark = pytest.mark.gpu

PHRASES, STRENGTHS = [[A], [B, C], [A, B, C], [C, A, B, 61]], [3.0, 2.5, 4.0, 6.0]


def test_score_reproduces_a_revocable_greedy_call(setup):
    cfg, model, enc = setup
    prompt = _prompt(cfg, True)
    kw = dict(_kw(cfg, "greedy", timestamps=True), repetition_penalty=1.2, no_repeat_ngram_size=3)
    rules = dict(suppress_tokens=kw["suppress_tokens"], repetition_penalty=1.2, no_repeat_ngram_size=3)
    boost = model.boost_list(PHRASES, STRENGTHS, revocable=True)
    assert boost.revocable and not boost.large
    res = model.generate(enc, [prompt] * 3, return_alternatives=2, boost=boost, **kw)
    base = model.generate(enc, [prompt] * 3, return_alternatives=2, **kw)
    assert [r.token_logprobs for r in res] != [r.token_logprobs for r in base]       # (the list did something)
    sc = model.score(enc, [prompt] * 3, [r.sequences_ids[0] for r in res], rules=True, boost=boost, **rules)
    for r, s in zip(res, sc):
        ids = r.sequences_ids[0]
        assert s.sequences_ids[0] == ids and len(ids) >= 1
        assert np.array_equal(_bits(s.token_logprobs[0]), _bits(r.token_logprobs[0]))
        assert s.best_ids[0][:len(ids)] == [alts[0][0] for alts in r.token_alternatives[0]] == ids
        assert np.array_equal(_bits(s.best_logprobs[0][:len(ids)]), _bits([alts[0][1] for alts in r.token_alternatives[0]]))


def test_equal_revocable_lists_share_a_run_and_other_forms_do_not():
    cfg, model = _group_model()
    prompt = _prompt(cfg)
    base = dict(beam_size=5, num_hypotheses=3, max_length=len(prompt) + 10, length_penalty=0.0, return_scores=True,
                return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_alternatives=3)
    one = model.boost_list(PHRASES, STRENGTHS, revocable=True)
    twin = model.boost_list(PHRASES[::-1] + PHRASES[:1], STRENGTHS[::-1] + STRENGTHS[:1], revocable=True)
    kws = [dict(base, boost=one), dict(base, boost=twin), dict(base, boost=model.boost_list(PHRASES, STRENGTHS)), dict(base)]
    batches = _batches((3, 2, 3, 2))
    solo = [model.generate(model.encode_pcm(b), [prompt] * len(b), **kw) for b, kw in zip(batches, kws)]
    out, runs = _behind_a_blocker(model, cfg, batches, [prompt] * 4, kws)
    assert runs == 3
    for o, s in zip(out, solo):
        _same(o, s, alternatives=True)


def test_a_phrase_id_from_eot_up_is_refused_before_anything_is_queued(setup):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    for bad in (cfg.eot, cfg.timestamp_begin + 3):
        boost = model.boost_list([[A], [B, bad]], [1.0, 1.0], revocable=True)
        with pytest.raises(ValueError, match=f"phrase 1 holds id {bad}"):
            model.generate(enc, [prompt] * 3, boost=boost, **_kw(cfg, "greedy"))
        with pytest.raises(ValueError, match=f"phrase 1 holds id {bad}"):
            model.score(enc, [prompt] * 3, [[A]] * 3, rules=True, boost=boost)
