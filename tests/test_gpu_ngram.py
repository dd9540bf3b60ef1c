"""generate(..., lm=) and score(..., lm=) end to end on the GPU, on the setup of tests/test_gpu_constrain.py (the micro model
of seed 11, three chunks, 12 new tokens; A, B, C are text ids outside the suppress list): lm=NULL against the existing
entry point, scoring (with the model alone and with every kind of extra at once), the lane buffers that scoring and decode
runs share, run sharing, steering by a unigram model, the constraint behind the fusion, and the call-time
ValueErrors."""
import numpy as np
import pytest

import constrain_refs as cr
from faster_whisper_amd import backend
from faster_whisper_amd.grammar import Grammar
from faster_whisper_amd.ngram import BOS, EOS, NgramLM
from test_gpu_alternatives import MODES, NEW, _batches, _behind_a_blocker, _group_model, _kw, _prompt, _same, _suppress
from test_gpu_constrain import A, B, C, PH9, _bits, setup  # noqa: F401  (setup: the module fixture)

pytestmark = pytest.mark.gpu

# a trigram model over a handful of text ids: contexts with BOS, back-offs, </s>
TRI = NgramLM([{(BOS,): (0.0, -0.4), (EOS,): (-1.5, 0.0), (A,): (-1.0, -0.3), (B,): (-1.2, -0.2), (C,): (-2.0, -0.5)},
               {(BOS, A): (-0.2, -0.1), (A, B): (-0.3, -0.6), (B, C): (-0.4, 0.0), (C, EOS): (-0.1, 0.0)},
               {(BOS, A, B): (-0.05, 0.0), (A, B, C): (-0.02, 0.0), (B, C, EOS): (-0.01, 0.0)}], unk_logprob=-9.0)


def _kw_text(cfg, mode, timestamps=False):
    """_kw with the ids the fusion does not touch suppressed (the specials; without timestamp rules the timestamps too)"""
    kw = _kw(cfg, mode, timestamps=timestamps)
    rest = range(cfg.eot + 1, cfg.timestamp_begin if timestamps else cfg.n_vocab)
    return dict(kw, suppress_tokens=sorted(set(kw["suppress_tokens"]) | set(rest)))


def _through_lm(lib, head, outs, lp, alt, n_alt, top_k, top_p, boost_h, constraint_h, automaton_h=None, lm_h=None):
    return lib.fw_generate_lm, (*head, top_k, top_p, n_alt, boost_h, constraint_h, automaton_h, lm_h, *outs, *lp, *alt)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_no_model_is_the_existing_entry_point(setup, mode, monkeypatch):
    cfg, model, enc = setup
    kw = dict(_kw(cfg, mode), return_alternatives=4, boost=model.boost_list([[A, B]], [2.0]), constraint=model.constraint_list(PH9))
    want = model.generate(enc, [_prompt(cfg)] * 3, **kw)
    monkeypatch.setattr(backend, "_generate_call", _through_lm)
    _same(model.generate(enc, [_prompt(cfg)] * 3, **kw), want, alternatives=True)


def _assert_score_is_the_call(res, sc):
    for r, s in zip(res, sc):
        assert len(r.sequences_ids[0]) < NEW
        assert np.array_equal(_bits(s.token_logprobs[0]), _bits(r.token_logprobs[0]))
        assert _bits(s.end_logprobs[0]) == _bits(r.end_logprobs[0])
        alt0 = [a[0] for a in r.token_alternatives[0]] + [r.end_alternatives[0][0]]
        assert s.best_ids[0] == [i for i, _ in alt0]
        assert np.array_equal(_bits(s.best_logprobs[0]), _bits([v for _, v in alt0]))


@pytest.mark.parametrize("kinds", ["lm", "every kind"])
def test_score_reproduces_greedy(setup, kinds):
    """every kind: a boost list, the model and PH9 as a constraint list, then as the automaton of the same phrases in the
    list's place — a path that drops a kind or uploads another kind's table cannot give the other path's bits"""
    cfg, model, enc = setup
    prompt, lm = _prompt(cfg), model.ngram_lm(TRI, 10.0, 0.5)      # (strong enough to close every hypothesis on </s>)
    kw = _kw_text(cfg, "greedy")
    plain = model.generate(enc, [prompt] * 3, **kw)
    extras = [dict(lm=lm)]
    if kinds == "every kind":
        boost = model.boost_list([[A, B], [C]], [2.0, 1.5])
        extras = [dict(lm=lm, boost=boost, constraint=model.constraint_list(PH9)),
                  dict(lm=lm, boost=boost, automaton=model.automaton(Grammar.phrases(PH9)))]
    ids = []
    for ex in extras:
        res = model.generate(enc, [prompt] * 3, return_alternatives=2, **ex, **kw)
        ids.append([r.sequences_ids for r in res])
        assert ids[-1] != [r.sequences_ids for r in plain]                             # the extras do something
        sc = model.score(enc, [prompt] * 3, [r.sequences_ids[0] for r in res], rules=True, suppress_tokens=kw["suppress_tokens"], **ex)
        _assert_score_is_the_call(res, sc)
    assert all(i == ids[0] for i in ids)                   # the list and its automaton allow the same strings


# larger than every other model of this file: the lane's table buffer has to grow for it
BIG = NgramLM([{(BOS,): (0.0, -0.4), (EOS,): (-1.5, 0.0), **{(v,): (-1.0 - 0.01 * v, -0.3) for v in range(10, 60)}},
               {(v, v + 1): (-0.2, 0.0) for v in range(10, 59)}], unk_logprob=-9.0)


def test_scoring_and_runs_share_the_lane_buffers(setup):
    """score() keeps its tables where a decode run keeps its own: a score call with another boost list and a larger model
    (the buffer is replaced) between two equal generate calls changes nothing in the second, and the other way round"""
    cfg, model, enc = setup
    prompt, kw = _prompt(cfg), _kw_text(cfg, "greedy")
    gen = dict(kw, return_alternatives=2, boost=model.boost_list([[A, B]], [2.0]),
               lm=model.ngram_lm(NgramLM([{(A,): (-1.0, 0.0), (EOS,): (-1.5, 0.0)}], unk_logprob=-9.0), 2.0, 0.5))
    score = dict(rules=True, suppress_tokens=kw["suppress_tokens"], boost=model.boost_list([[B], [C, A]], [1.0, 3.0]),
                 lm=model.ngram_lm(BIG, 1.0))
    want = model.generate(enc, [prompt] * 3, **gen)
    sc = model.score(enc, [prompt] * 3, [[B, C]] * 3, **score)
    _same(model.generate(enc, [prompt] * 3, **gen), want, alternatives=True)
    for s, t in zip(model.score(enc, [prompt] * 3, [[B, C]] * 3, **score), sc):
        assert np.array_equal(_bits(s.token_logprobs[0]), _bits(t.token_logprobs[0])) and s.best_ids == t.best_ids


def test_equal_models_share_a_run_and_others_do_not():
    cfg, model = _group_model()
    short = _prompt(cfg)
    prompts = [short, [cfg.sot_prev] + [10 + (7 * i) % 200 for i in range(17)] + short, short, short]
    base = dict(beam_size=5, num_hypotheses=3, max_length=len(prompts[1]) + 10, length_penalty=0.0, return_scores=True,
                return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_alternatives=3)
    kws = [dict(base, lm=model.ngram_lm(TRI, 1.5, 0.25)), dict(base, lm=model.ngram_lm(TRI, 1.5, 0.25)),
           dict(base, lm=model.ngram_lm(TRI, 1.0, 0.25)), dict(base)]
    batches = _batches((3, 2, 3, 2))
    solo = [model.generate(model.encode_pcm(b), [p] * len(b), **kw) for b, p, kw in zip(batches, prompts, kws)]
    out, runs = _behind_a_blocker(model, cfg, batches, prompts, kws)
    assert runs == 3                       # (the two equal models share theirs; another scale and the plain call do not join)
    for o, s in zip(out, solo):
        _same(o, s, alternatives=True)


@pytest.mark.parametrize("mode,timestamps", [("greedy", False), ("beam5", False), ("beam5", True)])
def test_a_unigram_model_steers(setup, mode, timestamps):
    """S gets 0 and every other text id -1e6 at scale 1: far above any logit difference the micro model produces, which the
    recorded alternatives show — whatever is outside S, the timestamps and <eot> lies 1e5 below the best id, or is -inf"""
    cfg, model, enc = setup
    S = {A, B, C}
    lm = model.ngram_lm(NgramLM([{**{(v,): (0.0, 0.0) for v in S}, (EOS,): (0.0, 0.0)}], unk_logprob=-1e6), 1.0)
    kw = dict(_kw_text(cfg, mode, timestamps=timestamps), return_alternatives=8)
    res = model.generate(enc, [_prompt(cfg, timestamps)] * 3, lm=lm, **kw)
    ok = lambda t: t in S or t == cfg.eot or t >= cfg.timestamp_begin   # noqa: E731
    n_text = 0
    for r in res:
        for ids, alts in zip(r.sequences_ids, r.token_alternatives):
            assert all(ok(t) for t in ids), ids          # (an empty one: an unfilled beam slot, tests/test_gpu_constrain.py)
            n_text += sum(t in S for t in ids)
            for alt in alts:
                assert all(lp == -np.inf or lp < alt[0][1] - 1e5 for t, lp in alt if not ok(t)), alt
                assert sum(not ok(t) for t, _ in alt) >= 1 or timestamps        # (8 alternatives reach past S and <eot>)
    assert n_text > 0


def test_the_constraint_holds_behind_the_fusion(setup):
    cfg, model, enc = setup
    lm = model.ngram_lm(TRI, 3.0, 1.0)
    res = model.generate(enc, [_prompt(cfg)] * 3, lm=lm, constraint=model.constraint_list(PH9), **_kw(cfg, "beam5"))
    for r in res:
        for ids, score in zip(r.sequences_ids, r.scores):
            if ids:                                           # (an unfilled beam slot: tests/test_gpu_constrain.py)
                kind = cr.in_list(PH9, ids, cfg.timestamp_begin)
                assert np.isfinite(score) and (kind == "phrase" if len(ids) < NEW else kind is not None), (ids, kind)
    assert all(r.sequences_ids[0] for r in res)


REFUSED = {
    "another vocabulary": lambda cfg: backend.NgramFusion(cfg.n_vocab + 1, cfg.eot, TRI, 1.0),
    "eos_id is not <eot>": lambda cfg: backend.NgramFusion(cfg.n_vocab, cfg.eot - 1, TRI, 1.0),
    "an n-gram id above <eot>": lambda cfg: backend.NgramFusion(cfg.n_vocab, cfg.eot, NgramLM([{(cfg.eot + 1,): (-1.0, 0.0)}], -9.0), 1.0),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_errors(setup, name):
    cfg, model, enc = setup
    lm = REFUSED[name](cfg)
    with pytest.raises(ValueError):
        model.generate(enc, [_prompt(cfg)] * 3, lm=lm, **_kw(cfg, "greedy"))
    with pytest.raises(ValueError):
        model.score(enc, [_prompt(cfg)] * 3, [[A]] * 3, rules=True, lm=lm, suppress_tokens=_suppress(cfg))


def test_errors_of_the_call(setup):
    cfg, model, enc = setup
    lm = model.ngram_lm(TRI, 1.0)
    with pytest.raises(ValueError):
        model.score(enc, [_prompt(cfg)] * 3, [[A]] * 3, lm=lm)                    # needs rules=True
    with pytest.raises(TypeError):
        model.generate(enc, [_prompt(cfg)] * 3, lm=TRI, **_kw(cfg, "greedy"))     # an NgramLM is not an NgramFusion
    at, ct = model.automaton(Grammar.phrases(PH9)), model.constraint_list(PH9)    # both kinds: the first thing the engine checks
    with pytest.raises(ValueError, match="not both"):
        backend._lib.check(model._lib.fw_generate_lm(*_through_lm(
            model._lib, (None, None, None, None, 0, None), (None,) * 4, (None,) * 2, (None,) * 4, 0, 0, 1.0, None, ct._handle, at._handle, lm._handle)[1]))
    with pytest.raises(ValueError, match="not both"):
        backend._lib.check(model._lib.fw_score_lm(*(None,) * 6, 0, 0, None, None, ct._handle, at._handle, lm._handle, None, None, None))


def test_transcribe_needs_lm_scale():
    from faster_whisper_amd.transcribe import BatchedInferencePipeline, WhisperModel
    m, pipe = WhisperModel.__new__(WhisperModel), BatchedInferencePipeline.__new__(BatchedInferencePipeline)
    pipe.model = m
    audio = np.zeros(16000, dtype=np.float32)
    for entry, arg in ((m.transcribe, audio), (pipe.transcribe, audio), (m.transcribe_many, [audio]), (pipe.transcribe_many, [audio])):
        with pytest.raises(ValueError, match="lm_scale"):
            entry(arg, language_model=TRI)
