"""generate(..., automaton=) and score(..., automaton=) end to end on the GPU, on the setup of tests/test_gpu_constrain.py
(the micro model of seed 11, three chunks, 12 new tokens; A, B, C and the other ids are text ids outside the suppress list):
the phrase grammar against the constraint list bit for bit, the guarantee of include/fwamd.h, scoring, run sharing, the
call-time ValueErrors, and the boost in front."""
import numpy as np
import pytest

from faster_whisper_amd.grammar import Grammar
from test_gpu_alternatives import MODES, NEW, _batches, _behind_a_blocker, _group_model, _kw, _prompt, _same, _suppress
from test_gpu_constrain import A, B, C, PH9, _bits, setup  # noqa: F401  (setup: the module fixture)

pytestmark = pytest.mark.gpu

DIGITS = Grammar.repeat([[A], [B], [C, 21]], 2, 4)
COMMAND = Grammar.sequence([[[22], [23, 24]], [[A, B], [A, C], [25]]])
GRAMMARS = {"repeat": DIGITS, "sequence": COMMAND}
# with timestamps the pairs around the text use the budget up: strings of one or two ids, so that hypotheses still close
SHORT = {"repeat": Grammar.repeat([[A], [B]], 1, 2), "sequence": Grammar.sequence([[[22], [A]], [[B], [25]]])}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_phrase_grammar_is_the_constraint_list(setup, mode):
    cfg, model, enc = setup
    kw = dict(_kw(cfg, mode), return_alternatives=4)
    want = model.generate(enc, [_prompt(cfg)] * 3, constraint=model.constraint_list(PH9), **kw)
    got = model.generate(enc, [_prompt(cfg)] * 3, automaton=model.automaton(Grammar.phrases(PH9)), **kw)
    _same(got, want, alternatives=True)


@pytest.mark.parametrize("budget", [NEW, 3])
@pytest.mark.parametrize("mode,timestamps", [("beam5", False), ("sampling", False), ("beam5", True),
                                             ("sampling", True)])
@pytest.mark.parametrize("name", sorted(GRAMMARS))
def test_the_guarantee(setup, name, mode, timestamps, budget):
    cfg, model, enc = setup
    g, prompt = (SHORT if timestamps else GRAMMARS)[name], _prompt(cfg, timestamps)
    kw = dict(_kw(cfg, mode, timestamps=timestamps), max_length=len(prompt) + budget)
    res = model.generate(enc, [prompt] * 3, automaton=model.automaton(g), **kw)
    closed = 0
    for r in res:
        for ids, score in zip(r.sequences_ids, r.scores):
            if not ids:                                       # an unfilled beam slot (tests/test_gpu_constrain.py)
                continue
            assert np.isfinite(score) and len(ids) <= budget
            text = [t for t in ids if t < cfg.timestamp_begin]
            assert g.accepts(text) if len(ids) < budget else g.is_prefix(text), (ids, text)
            closed += len(ids) < budget
    print(f"[{name}, {mode}, timestamps={timestamps}, budget {budget}] {closed} closed on <eot>")
    assert any(r.sequences_ids[0] for r in res) and (closed > 0 or budget == 3)


def test_score_reproduces_greedy_and_leaving_the_language_is_minus_infinity(setup):
    cfg, model, enc = setup
    prompt, at = _prompt(cfg), model.automaton(DIGITS)
    rules = dict(suppress_tokens=_suppress(cfg))
    res = model.generate(enc, [prompt] * 3, automaton=at, return_token_logprobs=True, **_kw(cfg, "greedy"))
    sc = model.score(enc, [prompt] * 3, [r.sequences_ids[0] for r in res], rules=True, automaton=at, **rules)
    for r, s in zip(res, sc):
        assert len(r.sequences_ids[0]) < NEW and DIGITS.accepts(r.sequences_ids[0])
        assert np.array_equal(_bits(s.token_logprobs[0]), _bits(r.token_logprobs[0]))
        assert _bits(s.end_logprobs[0]) == _bits(r.end_logprobs[0])
    targets = [[[A, B, 22, A], [A, C, 21, B], [22], [A] * 5]] * 3              # leave at 2, never, at 0, at 4
    for s in model.score(enc, [prompt] * 3, targets, rules=True, automaton=at, **rules):
        for lps, end, q in zip(s.token_logprobs, s.end_logprobs, (2, None, 0, 4)):
            lps = np.asarray(lps + [end], dtype=np.float32)
            assert np.all(np.isfinite(lps[:q])) and (q is None or np.all(lps[q:] == -np.inf)), lps


def test_equal_automata_share_a_run_and_others_do_not():
    cfg, model = _group_model()
    short = _prompt(cfg)
    prompts = [short, [cfg.sot_prev] + [10 + (7 * i) % 200 for i in range(17)] + short, short, short]
    base = dict(beam_size=5, num_hypotheses=3, max_length=len(prompts[1]) + 10, length_penalty=0.0, return_scores=True,
                return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_alternatives=3)
    phrases = Grammar.phrases(PH9)
    kws = [dict(base, automaton=model.automaton(phrases)), dict(base, automaton=model.automaton(Grammar.phrases(PH9[::-1]))),
           dict(base, automaton=model.automaton(DIGITS)), dict(base)]
    batches = _batches((3, 2, 3, 2))
    solo = [model.generate(model.encode_pcm(b), [p] * len(b), **kw) for b, p, kw in zip(batches, prompts, kws)]
    out, runs = _behind_a_blocker(model, cfg, batches, prompts, kws)
    assert runs == 3                                                          # (the two equal automata share theirs)
    for o, s in zip(out, solo):
        _same(o, s, alternatives=True)


def test_errors(setup):
    from faster_whisper_amd.backend import Automaton
    cfg, model, enc = setup
    prompt, kw = _prompt(cfg), _kw(cfg, "greedy")
    sup = kw["suppress_tokens"]
    at = model.automaton(DIGITS)
    refused = [
        dict(automaton=Automaton(cfg.n_vocab + 1, DIGITS)),                       # another vocabulary
        dict(automaton=model.automaton(Grammar.phrases([[A, cfg.eot]]))),          # an edge id >= <eot>
        dict(automaton=model.automaton(Grammar.phrases([[A, sup[0]]]))),           # a suppressed edge id
        dict(automaton=model.automaton(Grammar.phrases([[cfg.suppress_begin[0], A]]))),   # suppress_blank, state 0
        dict(automaton=at, no_repeat_ngram_size=2),
        dict(automaton=at, min_new_tokens=1),
        dict(automaton=at, constraint=model.constraint_list(PH9)),                 # no call carries both
    ]
    for over in refused:
        with pytest.raises(ValueError):
            model.generate(enc, [prompt] * 3, **dict(kw, **over))
    with pytest.raises(ValueError):
        model.score(enc, [prompt] * 3, [[A]] * 3, automaton=at)                   # needs rules=True
    with pytest.raises(ValueError):
        model.score(enc, [prompt] * 3, [[A]] * 3, rules=True, automaton=at, no_repeat_ngram_size=2, suppress_tokens=sup)
    model.score(enc, [prompt] * 3, [[A]] * 3, rules=True, automaton=at, suppress_tokens=sup)
    with pytest.raises(TypeError):
        model.generate(enc, [prompt] * 3, automaton=DIGITS, **kw)                 # a Grammar is not an Automaton


def test_with_a_boost(setup):
    cfg, model, enc = setup
    prompt, kw, at = _prompt(cfg), _kw(cfg, "greedy"), model.automaton(DIGITS)
    base = model.generate(enc, [prompt] * 3, automaton=at, return_token_logprobs=True, **kw)
    off = model.generate(enc, [prompt] * 3, automaton=at, boost=model.boost_list([[30]], [1e4]), return_token_logprobs=True, **kw)
    _same(off, base)
    on = model.generate(enc, [prompt] * 3, automaton=at, boost=model.boost_list([[B]], [1e4]), **kw)
    assert all(r.sequences_ids[0] == [B] * 4 for r in on)
