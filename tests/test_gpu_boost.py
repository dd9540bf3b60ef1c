"""generate(..., boost=list) and score(..., boost=list) end to end on the GPU, on the setup of tests/test_gpu_alternatives.py
(the micro model of seed 11, three chunks, one of them short, that file's prompt and suppress list, 12 new tokens).
A, B, C are text ids outside the suppress list and outside suppress_begin.

  1. boost=None and an empty list are the call without them: ids, scores, no-speech values, log-probs, alternatives;
  2. phrase [A] at +1e4: every hypothesis is [A] * budget and every token log-prob is exactly 0.0 (greedy and sampling);
  3. phrase [A, B, C] at +1e4 with no_repeat_ngram_size=1: the best hypothesis of every chunk starts [A, B, C] — the boost
     comes before the rules (A stays boosted at every step and the n-gram rule forbids it from step 1 on) and every beam
     is matched against its own, reordered history;
  4. score(..., rules=True, boost=list) on the ids a boosted greedy call returned reproduces its token and end log-probs
     bit for bit, and its best ids are alternative 0;
  5. two calls with equal lists built separately (one behind a longer prompt) meet in ONE decode run, a call with another
     list and a plain call do not join them, and all four get their solo results;
  6. a list for another vocabulary and score(boost=..., rules=False) are ValueErrors.

Seen on an MI355X: test 4 — no hypothesis closes by <eot> with its boost at 3.0 (all cut at the budget: the end values
are then 0.0 / None on both sides), all three close with it at 6, 10 and 16, where the end values are compared too;
test 5 — the four calls took 3 decode runs."""
import numpy as np
import pytest

from conftest import bench_audio, make_model
from test_gpu_alternatives import MODES, NEW, _batches, _behind_a_blocker, _group_model, _kw, _prompt, _same, _suppress

pytestmark = pytest.mark.gpu

A, B, C = 20, 37, 55


@pytest.fixture(scope="module")
def setup():
    from faster_whisper_amd.backend import StorageView
    cfg, w, model = make_model("micro", seed=11, max_batch=4, max_beam=5)
    assert not {A, B, C} & (set(_suppress(cfg)) | set(cfg.suppress_begin)) and max(A, B, C) < cfg.eot
    chunks = [bench_audio(480000, seed=1), bench_audio(200000, seed=2), bench_audio(480000, seed=3)[::-1].copy()]
    enc = model.encode(StorageView.from_array(model.log_mel(chunks)))
    return cfg, model, enc


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_none_and_empty_list_change_nothing(setup, mode):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    kw = _kw(cfg, mode)
    base = model.generate(enc, [prompt] * 3, return_alternatives=4, **kw)
    empty = model.boost_list([], [])
    assert len(empty) == 0
    for boost in (None, empty):
        _same(model.generate(enc, [prompt] * 3, return_alternatives=4, boost=boost, **kw), base, alternatives=True)
    plain = model.generate(enc, [prompt] * 3, **kw)
    for boost in (None, empty):
        res = model.generate(enc, [prompt] * 3, boost=boost, **kw)
        assert [(r.sequences_ids, r.scores, r.no_speech_prob) for r in res] == \
               [(r.sequences_ids, r.scores, r.no_speech_prob) for r in plain]


@pytest.mark.parametrize("mode", ["greedy", "sampling"])
def test_a_huge_boost_decides_every_step(setup, mode):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    res = model.generate(enc, [prompt] * 3, return_token_logprobs=True, boost=model.boost_list([[A]], [1e4]), **_kw(cfg, mode))
    for r in res:
        assert len(r.sequences_ids) == MODES[mode].get("num_hypotheses", 1)
        for ids, lps in zip(r.sequences_ids, r.token_logprobs):
            assert ids == [A] * NEW
            assert lps == [0.0] * NEW


@pytest.mark.parametrize("mode", ["greedy", "beam5"])
def test_boost_comes_before_the_rules_on_every_beam(setup, mode):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    kw = dict(_kw(cfg, mode), no_repeat_ngram_size=1)
    assert kw["length_penalty"] == 0.0
    res = model.generate(enc, [prompt] * 3, boost=model.boost_list([[A, B, C]], [1e4]), **kw)
    for r in res:
        ids = r.sequences_ids[0]
        assert ids[:3] == [A, B, C], ids
        assert len(set(ids)) == len(ids)                  # (the n-gram rule of size 1 still holds: the rules win)


def _score_reproduces(cfg, model, enc, phrases, strengths):
    """a boosted greedy call with timestamps, repetition penalty and a 3-gram rule against score() with the same rules and
    list on the ids it returned; returns how many of the three hypotheses were closed by <eot>"""
    prompt = _prompt(cfg, True)
    kw = dict(_kw(cfg, "greedy", timestamps=True), repetition_penalty=1.2, no_repeat_ngram_size=3)
    rules = dict(suppress_tokens=kw["suppress_tokens"], repetition_penalty=1.2, no_repeat_ngram_size=3)
    boost = model.boost_list(phrases, strengths)
    base = model.generate(enc, [prompt] * 3, return_alternatives=2, **kw)
    res = model.generate(enc, [prompt] * 3, return_alternatives=2, boost=boost, **kw)
    assert [r.token_logprobs for r in res] != [r.token_logprobs for r in base]       # (the list did something)
    sc = model.score(enc, [prompt] * 3, [r.sequences_ids[0] for r in res], rules=True, boost=boost, **rules)
    closed = 0
    for r, s in zip(res, sc):
        ids = r.sequences_ids[0]
        assert s.sequences_ids[0] == ids and len(ids) >= 1
        assert np.array_equal(_bits(s.token_logprobs[0]), _bits(r.token_logprobs[0]))
        assert s.best_ids[0][:len(ids)] == [alts[0][0] for alts in r.token_alternatives[0]]
        assert np.array_equal(_bits(s.best_logprobs[0][:len(ids)]), _bits([alts[0][1] for alts in r.token_alternatives[0]]))
        if len(ids) < NEW:                                # closed by <eot>: the end values too
            closed += 1
            assert _bits(s.end_logprobs[0]) == _bits(r.end_logprobs[0])
            assert s.best_ids[0][len(ids)] == r.end_alternatives[0][0][0] == cfg.eot
            assert _bits(s.best_logprobs[0][len(ids)]) == _bits(r.end_alternatives[0][0][1])
        else:                                             # cut at the budget: no closing step
            assert r.end_logprobs[0] == 0.0 and r.end_alternatives[0] is None
    # without the list the score is that of the unboosted distribution: not the call's
    plain = model.score(enc, [prompt] * 3, [r.sequences_ids[0] for r in res], rules=True, **rules)
    assert [s.token_logprobs for s in plain] != [s.token_logprobs for s in sc]
    return closed


def test_score_reproduces_a_boosted_greedy_call(setup):
    """a modest list (3.0, phrases of 1 - 3 tokens, one behind a timestamp); then the same phrases with <eot> boosted harder
    and harder, so that hypotheses close by <eot> and the end values are compared too"""
    cfg, model, enc = setup
    phrases = [[A], [B, C], [A, B, C], [cfg.timestamp_begin + 10, A], [cfg.eot]]
    closed = [_score_reproduces(cfg, model, enc, phrases, [3.0] * 5)]
    for eot_boost in (6.0, 10.0, 16.0):
        closed.append(_score_reproduces(cfg, model, enc, phrases, [3.0] * 4 + [eot_boost]))
    print(f"hypotheses closed by <eot> with its boost at 3, 6, 10, 16: {closed} of 3 each")
    assert sum(closed) > 0


def test_equal_lists_share_a_run_and_others_do_not():
    cfg, model = _group_model()
    short = _prompt(cfg)
    longer = [cfg.sot_prev] + [10 + (7 * i) % 200 for i in range(17)] + short
    prompts = [short, longer, short, short]
    base = dict(beam_size=5, num_hypotheses=3, max_length=len(longer) + 10, length_penalty=0.0, return_scores=True,
                return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_alternatives=3)
    phrases, strengths = [[A, B], [C], [B, C, A]], [4.0, 2.0, 6.0]
    one, twin = model.boost_list(phrases, strengths), model.boost_list([list(p) for p in phrases], list(strengths))
    other = model.boost_list(phrases, [4.0, 2.0, 6.5])
    kws = [dict(base, boost=one), dict(base, boost=twin), dict(base, boost=other), dict(base)]
    batches = _batches((3, 2, 3, 2))
    solo = [model.generate(model.encode_pcm(b), [p] * len(b), **kw) for b, p, kw in zip(batches, prompts, kws)]
    assert [r.sequences_ids for r in solo[0]] != [r.sequences_ids for r in
                                                   model.generate(model.encode_pcm(batches[0]), [short] * 3, **base)]
    out, runs = _behind_a_blocker(model, cfg, batches, prompts, kws)
    print(f"4 calls (list, equal list behind a longer prompt, another list, none) -> {runs} decode run(s)")
    assert runs == 3
    for o, s in zip(out, solo):
        _same(o, s, alternatives=True)


def test_errors(setup):
    from faster_whisper_amd.backend import BoostList
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    foreign = BoostList(cfg.n_vocab + 1, [[A]], [1.0])
    with pytest.raises(ValueError):
        model.generate(enc, [prompt] * 3, boost=foreign, **_kw(cfg, "greedy"))
    with pytest.raises(ValueError):
        model.score(enc, [prompt] * 3, [[A]] * 3, rules=True, boost=foreign)
    with pytest.raises(ValueError):
        model.score(enc, [prompt] * 3, [[A]] * 3, rules=False, boost=model.boost_list([[A]], [1.0]))
    with pytest.raises(ValueError):
        model.boost_list([[cfg.n_vocab]], [1.0])
    with pytest.raises(ValueError):
        model.boost_list([[A]], [float("nan")])
