"""generate(..., constraint=list) and score(..., constraint=list) end to end on the GPU, on the setup of
tests/test_gpu_alternatives.py (the micro model of seed 11, three chunks, one of them short, that file's prompt and suppress
list, 12 new tokens).  A, B, C and the other phrase ids are text ids outside the suppress list and outside suppress_begin.

  1. constraint=None and an empty list are the call without them, bit for bit, in all three MODES, with alternatives;
  2. THE GUARANTEE (include/fwamd.h): a hypothesis with a finite score, its timestamp ids removed, is a phrase of the list
     when it closed on <eot> and a prefix of one when the budget cut it — with <|notimestamps|> in greedy, beam 5 and
     sampling, with timestamps in greedy and beam 5, and with a budget shorter than every phrase (then a PROPER prefix);
  3. a single phrase [A, B, C]: every hypothesis is exactly that, every token log-prob and the end log-prob exactly 0.0;
     and what a beam search returns in the slots it cannot fill (below);
  4. the list {[A], [A, B]}: the alternatives at step 1 are {<eot>, B} then (0, -inf) twice, probabilities summing to 1;
  5. the constrained log-probs against the engine's own RAW distribution: raw[v] - logsumexp(raw[allowed]) in float64;
  6. score(..., rules=True, constraint=list) reproduces a greedy constrained call bit for bit; a target that leaves the
     list at position q is finite before q and -inf from q on, the end entry included;
  7. two calls with equal lists built separately share ONE decode run, another list and a plain call do not join;
  8. the call-time ValueErrors;
  9. with a boost: +1e4 on an unlisted id changes nothing at all; on one listed phrase among several it decides;
 10. score() with a boost AND a constraint list over position blocks (several positions per pass, blocks that start
     behind position 0, rows without a target) gives the bits of the same call at one position per pass.

UNFILLED SLOTS (test 3, found, not changed): a beam search that is asked for more hypotheses than the list lets finish —
num_hypotheses=3 with ONE phrase — ends as soon as no live beam is left (-inf candidates are never merged, so a dead beam
is never recorded), and the slots it cannot fill are what every call's outputs start as: an EMPTY sequence with score 0.0,
no token log-probs, end log-prob 0.0 and end alternatives None.  An empty sequence is never a real hypothesis here (a
phrase has at least one token and a cut hypothesis has the budget's length), so a caller tells it by its length.

Seen on an MI355X: test 2 — every hypothesis closes on <eot> except with timestamps in beam 5, where 7 close and 2 are cut at
the budget of 12 (timestamp pairs between the tokens use it up); test 5 — largest difference 2.11e-07; test 7 — the four
calls took 3 decode runs."""
import numpy as np
import pytest

import constrain_refs as cr
from conftest import bench_audio, make_model
from test_gpu_alternatives import MODES, NEW, _batches, _behind_a_blocker, _group_model, _kw, _prompt, _same, _suppress

pytestmark = pytest.mark.gpu

A, B, C = 20, 37, 55
# nine phrases with shared prefixes, one of them a prefix of two others, lengths 1 .. 5
PH9 = [[A], [A, B], [A, B, C], [A, C], [B], [B, A, C, 21], [C, B], [C, B, A], [21, 22, 23, 24, 25]]


@pytest.fixture(scope="module")
def setup():
    from faster_whisper_amd.backend import StorageView
    cfg, w, model = make_model("micro", seed=11, max_batch=4, max_beam=5)
    ids = {t for p in PH9 for t in p}
    assert not ids & (set(_suppress(cfg)) | set(cfg.suppress_begin)) and max(ids) < cfg.eot
    chunks = [bench_audio(480000, seed=1), bench_audio(200000, seed=2), bench_audio(480000, seed=3)[::-1].copy()]
    enc = model.encode(StorageView.from_array(model.log_mel(chunks)))
    return cfg, model, enc


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _guarantee(cfg, res, phrases, budget, proper=False):
    """every hypothesis of every result; returns (closed on <eot>, cut at the budget, unfilled slots)"""
    closed = cut = empty = 0
    for r in res:
        for ids, score in zip(r.sequences_ids, r.scores):
            if not ids:                                   # an unfilled slot (module docstring)
                assert score == 0.0
                empty += 1
                continue
            assert np.isfinite(score) and len(ids) <= budget
            kind = cr.in_list(phrases, ids, cfg.timestamp_begin)
            if len(ids) < budget:
                assert kind == "phrase", (ids, kind)
                closed += 1
            else:
                assert kind is not None and (kind == "prefix" or not proper), (ids, kind)
                cut += 1
    return closed, cut, empty


@pytest.mark.parametrize("mode", sorted(MODES))
def test_none_and_empty_list_change_nothing(setup, mode):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    kw = _kw(cfg, mode)
    base = model.generate(enc, [prompt] * 3, return_alternatives=4, **kw)
    empty = model.constraint_list([])
    assert len(empty) == 0
    for c in (None, empty):
        _same(model.generate(enc, [prompt] * 3, return_alternatives=4, constraint=c, **kw), base, alternatives=True)
    plain = model.generate(enc, [prompt] * 3, **kw)
    for c in (None, empty):
        res = model.generate(enc, [prompt] * 3, constraint=c, **kw)
        assert [(r.sequences_ids, r.scores, r.no_speech_prob) for r in res] == \
               [(r.sequences_ids, r.scores, r.no_speech_prob) for r in plain]
    # an empty list goes with rules a real list is refused for
    res = model.generate(enc, [prompt] * 3, constraint=empty, **dict(kw, no_repeat_ngram_size=2))
    assert [r.sequences_ids for r in res] == [r.sequences_ids for r in model.generate(enc, [prompt] * 3,
                                                                                       **dict(kw, no_repeat_ngram_size=2))]
    sc = model.score(enc, [prompt] * 3, [[A, B]] * 3, rules=True, suppress_tokens=kw["suppress_tokens"])
    sc_e = model.score(enc, [prompt] * 3, [[A, B]] * 3, rules=True, constraint=empty, suppress_tokens=kw["suppress_tokens"])
    assert [s.token_logprobs for s in sc] == [s.token_logprobs for s in sc_e]


@pytest.mark.parametrize("mode,timestamps", [("greedy", False), ("beam5", False), ("sampling", False), ("greedy", True),
                                             ("beam5", True)])
def test_the_guarantee(setup, mode, timestamps):
    cfg, model, enc = setup
    prompt = _prompt(cfg, timestamps)
    lst = model.constraint_list(PH9)
    res = model.generate(enc, [prompt] * 3, constraint=lst, **_kw(cfg, mode, timestamps=timestamps))
    closed, cut, empty = _guarantee(cfg, res, PH9, NEW)
    print(f"[{mode}, timestamps={timestamps}] {closed} closed on <eot>, {cut} cut at the budget, {empty} unfilled")
    nh = MODES[mode].get("num_hypotheses", 1)
    assert all(len(r.sequences_ids) == nh for r in res)
    assert empty == 0 and closed + cut == 3 * nh          # nine phrases: three hypotheses finish in every mode
    if not timestamps:
        assert cut == 0                                   # (the budget is 12, the longest phrase 5)
        if mode == "beam5":
            assert all(len({tuple(ids) for ids in r.sequences_ids}) == 3 for r in res)
    else:
        assert all(ids[0] >= cfg.timestamp_begin for r in res for ids in r.sequences_ids)   # (the rules still run)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_budget_shorter_than_every_phrase_cuts_at_a_proper_prefix(setup, mode):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    phrases = [p for p in PH9 if len(p) >= 3]
    res = model.generate(enc, [prompt] * 3, constraint=model.constraint_list(phrases), **_kw(cfg, mode, new=2))
    closed, cut, empty = _guarantee(cfg, res, phrases, 2, proper=True)
    assert closed == 0 and cut >= 3


@pytest.mark.parametrize("mode", ["greedy", "sampling", "beam5"])
def test_a_single_phrase_is_certain(setup, mode):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    lst = model.constraint_list([[A, B, C]])
    kw = dict(_kw(cfg, mode), **({"num_hypotheses": 1} if mode == "beam5" else {}))
    res = model.generate(enc, [prompt] * 3, return_token_logprobs=True, constraint=lst, **kw)
    for r in res:
        assert len(r.sequences_ids) == kw.get("num_hypotheses", 1)
        for ids, lps, end in zip(r.sequences_ids, r.token_logprobs, r.end_logprobs):
            assert ids == [A, B, C]
            assert _bits(lps).tolist() == [0, 0, 0] and _bits(end) == 0          # exactly +0.0
    if mode != "beam5":
        return
    # asked for three, one can finish: slot 0 is the phrase, the others are unfilled (module docstring)
    res = model.generate(enc, [prompt] * 3, return_alternatives=2, constraint=lst, **_kw(cfg, "beam5"))
    for r in res:
        assert r.sequences_ids == [[A, B, C], [], []] and r.scores == [0.0, 0.0, 0.0]
        assert r.token_logprobs == [[0.0] * 3, [], []] and r.end_logprobs == [0.0] * 3
        assert r.token_alternatives[1:] == [[], []] and r.end_alternatives[1:] == [None, None]
        assert r.end_alternatives[0] == [(cfg.eot, 0.0), (0, -np.inf)]
    assert _guarantee(cfg, res, [[A, B, C]], NEW) == (3, 0, 6)


def test_alternatives_of_a_two_way_step(setup):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    res = model.generate(enc, [prompt] * 3, return_alternatives=4, constraint=model.constraint_list([[A], [A, B]]),
                         **_kw(cfg, "greedy"))
    for r in res:
        ids = r.sequences_ids[0]
        assert ids in ([A], [A, B])
        assert r.token_alternatives[0][0] == [(A, 0.0), (0, -np.inf), (0, -np.inf), (0, -np.inf)]
        alts = r.token_alternatives[0][1] if len(ids) == 2 else r.end_alternatives[0]
        assert {alts[0][0], alts[1][0]} == {cfg.eot, B} and alts[0][1] >= alts[1][1] > -np.inf
        assert alts[2:] == [(0, -np.inf), (0, -np.inf)]
        total = float(np.exp(np.float64(alts[0][1])) + np.exp(np.float64(alts[1][1])))
        assert abs(total - 1.0) <= 1e-6, total


def test_numbers_against_the_raw_distribution(setup):
    """greedy, <|notimestamps|>, suppress_blank off, no suppress list, penalty 1: at every step the constrained log-prob of
    the chosen id (and of the closing <eot>) is raw[v] - logsumexp(raw[allowed]) in float64, raw from score(rules=False) on
    the prefix, within 1e-4: raw log-probs are below 32 in magnitude, where an fp32 ulp is 3.8e-6, and both sides carry a few
    roundings; a masking error moves the value by the log of a mass ratio.  Largest difference seen on an MI355X: 2.11e-07
    (printed on every run)."""
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    kw = dict(_kw(cfg, "greedy"), suppress_blank=False, suppress_tokens=[])
    res = model.generate(enc, [prompt] * 3, return_token_logprobs=True, constraint=model.constraint_list(PH9), **kw)
    # the queries of chunk b: (step, id, the sequence to score, where its raw value is)
    queries = [[] for _ in res]
    for b, r in enumerate(res):
        ids = r.sequences_ids[0]
        assert cr.in_list(PH9, ids, cfg.timestamp_begin) == "phrase"
        for t in range(len(ids) + 1):
            allowed, eot_ok = cr.allowed_of_row(PH9, ids[:t], cfg.eot, cfg.timestamp_begin)
            for v in sorted(allowed):
                queries[b].append((t, v, ids[:t] + [v]))
            if eot_ok:
                queries[b].append((t, cfg.eot, ids[:t]))
    raw = [dict() for _ in res]
    H = 5                                                 # candidates go in groups of max_beam
    for g0 in range(0, max(len(q) for q in queries), H):
        groups = [q[g0:g0 + H] or [(None, None, [])] for q in queries]
        sc = model.score(enc, [prompt] * 3, [[seq for _, _, seq in g] for g in groups], rules=False)
        for b, (g, s) in enumerate(zip(groups, sc)):
            for h, (t, v, seq) in enumerate(g):
                if t is not None:
                    raw[b][(t, v)] = s.end_logprobs[h] if v == cfg.eot else s.token_logprobs[h][t]
    worst = 0.0
    for b, r in enumerate(res):
        ids = r.sequences_ids[0]
        for t in range(len(ids) + 1):
            vals = np.asarray([x for (tt, _), x in raw[b].items() if tt == t], dtype=np.float64)
            assert len(vals) >= 1 and np.all(np.abs(vals) < 32)
            lse = vals.max() + np.log(np.sum(np.exp(vals - vals.max())))
            v, got = (ids[t], r.token_logprobs[0][t]) if t < len(ids) else (cfg.eot, r.end_logprobs[0])
            diff = abs(float(got) - float(raw[b][(t, v)] - lse))
            worst = max(worst, diff)
            assert diff <= 1e-4, (b, t, v, got, raw[b][(t, v)] - lse)
    print(f"largest |constrained - (raw - logsumexp(raw[allowed]))| = {worst:.3g}")


@pytest.mark.parametrize("timestamps", [False, True])
def test_score_reproduces_a_constrained_greedy_call(setup, timestamps):
    cfg, model, enc = setup
    prompt = _prompt(cfg, timestamps)
    kw = dict(_kw(cfg, "greedy", timestamps=timestamps), repetition_penalty=1.2)
    rules = dict(suppress_tokens=kw["suppress_tokens"], repetition_penalty=1.2)
    lst = model.constraint_list(PH9)
    res = model.generate(enc, [prompt] * 3, return_alternatives=2, constraint=lst, **kw)
    sc = model.score(enc, [prompt] * 3, [r.sequences_ids[0] for r in res], rules=True, constraint=lst, **rules)
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
            assert s.best_ids[0][len(ids)] == r.end_alternatives[0][0][0]
            assert _bits(s.best_logprobs[0][len(ids)]) == _bits(r.end_alternatives[0][0][1])
    assert closed == 3 or timestamps
    plain = model.score(enc, [prompt] * 3, [r.sequences_ids[0] for r in res], rules=True, **rules)
    assert [s.token_logprobs for s in plain] != [s.token_logprobs for s in sc]       # (the list did something)


def test_a_target_that_leaves_the_list_scores_minus_infinity_from_there(setup):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    lst = model.constraint_list(PH9)
    targets = [[[A, B, 21, C], [B, A, C, 21], [22], [A, B, C, C, C]]] * 3        # leave at 2, never, at 0, at 3
    sc = model.score(enc, [prompt] * 3, targets, rules=True, constraint=lst, suppress_tokens=_suppress(cfg))
    for s in sc:
        for seq, lps, end, q in zip(s.sequences_ids, s.token_logprobs, s.end_logprobs, (2, None, 0, 3)):
            lps = np.asarray(lps + [end], dtype=np.float32)
            if q is None:
                assert np.all(np.isfinite(lps))
            else:
                assert np.all(np.isfinite(lps[:q])) and np.all(lps[q:] == -np.inf), (seq, lps)


def test_score_with_both_lists_over_position_blocks(setup):
    """Two chunks x two candidates with targets of 0, 1, 5 and 9 ids behind a prompt of 22 ids: 31 positions, so more than
    one block whatever the block size (at most 16), the later blocks start behind position 0, and the rows of positions in
    front of the last prompt token — and of the shorter targets' tails — have no target.  Both pre-pass kernels run on every
    block.  The reference is the same call with one position per pass (fw_test_knob 4, as tests/test_gpu_score.py compares
    plain scoring): there every launch is the single-row form that tests/test_gpu_boost_kernel.py and
    tests/test_gpu_constrain_kernel.py hold against the host walks bit for bit.  (The engine returns no logits rows, so the
    host walks cannot be applied to the rows of this call directly.)"""
    from faster_whisper_amd import _lib
    from faster_whisper_amd.backend import StorageView
    cfg, model, _ = setup
    lib = _lib.load()
    enc = model.encode(StorageView.from_array(model.log_mel([bench_audio(480000, seed=1), bench_audio(200000, seed=2)])))
    prompt = [cfg.sot_prev] + [10 + (7 * i) % 200 for i in range(17)] + _prompt(cfg)
    long9 = [B, A, C, 21, A, B, C, A, B]                  # a phrase, then five ids more: it leaves the list at 4
    targets = [[[], [A]], [[21, 22, 23, 24, 25], long9]]
    assert [len(t) for ts in targets for t in ts] == [0, 1, 5, 9] and len(prompt) + 9 > 16
    kw = dict(rules=True, suppress_tokens=_suppress(cfg), repetition_penalty=1.2)
    lists = dict(constraint=model.constraint_list(PH9), boost=model.boost_list([[A, B], [21, 22, 23]], [1.5, -0.75]))

    def bits(sc):
        return [[_bits(x).tolist() for x in (s.token_logprobs[h], s.end_logprobs[h], s.best_ids[h], s.best_logprobs[h])]
                for s in sc for h in range(2)]
    res = {}
    try:
        for on in (0, 1):
            _lib.check(lib.fw_test_knob(4, on))
            res[on] = model.score(enc, [prompt] * 2, targets, **kw, **lists)
    finally:
        _lib.check(lib.fw_test_knob(4, 1))
    assert bits(res[0]) == bits(res[1])
    # both lists did something, and the constraint's pattern is the one the list implies
    only_c = model.score(enc, [prompt] * 2, targets, constraint=lists["constraint"], **kw)
    only_b = model.score(enc, [prompt] * 2, targets, boost=lists["boost"], **kw)
    assert bits(only_c) != bits(res[1]) and bits(only_b) != bits(res[1])
    lps = [np.asarray(s.token_logprobs[h] + [s.end_logprobs[h]], dtype=np.float32) for s in res[1] for h in range(2)]
    assert lps[0][0] == -np.inf                           # no phrase is empty: <eot> at once is not allowed
    assert np.all(np.isfinite(lps[1])) and np.all(np.isfinite(lps[2]))
    assert np.all(np.isfinite(lps[3][:4])) and np.all(lps[3][4:] == -np.inf)


def test_equal_lists_share_a_run_and_others_do_not():
    cfg, model = _group_model()
    short = _prompt(cfg)
    longer = [cfg.sot_prev] + [10 + (7 * i) % 200 for i in range(17)] + short
    prompts = [short, longer, short, short]
    base = dict(beam_size=5, num_hypotheses=3, max_length=len(longer) + 10, length_penalty=0.0, return_scores=True,
                return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2], return_alternatives=3)
    # built separately, in another order and with a phrase named twice: the same set, so the same table
    one, twin = model.constraint_list(PH9), model.constraint_list([list(p) for p in reversed(PH9)] + [[A, B]])
    other = model.constraint_list(PH9[:-1])
    kws = [dict(base, constraint=one), dict(base, constraint=twin), dict(base, constraint=other), dict(base)]
    batches = _batches((3, 2, 3, 2))
    solo = [model.generate(model.encode_pcm(b), [p] * len(b), **kw) for b, p, kw in zip(batches, prompts, kws)]
    for s, kw, p in zip(solo[:3], kws, prompts):
        closed, cut, empty = _guarantee(cfg, s, PH9, base["max_length"] - len(p))
        assert closed == 3 * len(s) and cut == 0 and empty == 0
    assert [r.sequences_ids for r in solo[3]] != [r.sequences_ids for r in solo[0]][:2]
    out, runs = _behind_a_blocker(model, cfg, batches, prompts, kws)
    print(f"4 calls (list, equal list behind a longer prompt, another list, none) -> {runs} decode run(s)")
    assert runs == 3
    for o, s in zip(out, solo):
        _same(o, s, alternatives=True)


def test_errors(setup):
    from faster_whisper_amd.backend import ConstraintList
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    kw = _kw(cfg, "greedy")
    sup = kw["suppress_tokens"]

    def mirror(phrases, list_vocab=cfg.n_vocab, **over):
        o = dict(suppress=sup, suppress_blank=True, ngram=0, min_new=0)
        o.update(over)
        return cr.call_error(phrases, list_vocab, cfg.n_vocab, cfg.eot, o["suppress"], o["suppress_blank"],
                             cfg.suppress_begin, o["ngram"], o["min_new"])

    blank = cfg.suppress_begin[0]
    assert 7 in sup and 7 < cfg.eot and blank < cfg.eot and blank not in sup
    cases = [([[A]], dict(list_vocab=cfg.n_vocab + 1), {}),                               # another vocabulary
             ([[A, cfg.eot]], {}, {}),                                                    # an id >= eot
             ([[A, cfg.timestamp_begin + 3]], {}, {}),
             ([[A, 7]], {}, {}),                                                          # an id in the suppress list
             ([[blank, A]], {}, {}),                                                      # suppress_blank and a first id
             ([[A, B]], dict(ngram=2), dict(no_repeat_ngram_size=2)),
             ([[A, B]], dict(min_new=1), dict(min_new_tokens=1))]
    for phrases, m_over, g_over in cases:
        assert mirror(phrases, **m_over) is not None
        lst = ConstraintList(m_over.get("list_vocab", cfg.n_vocab), phrases)
        with pytest.raises(ValueError):
            model.generate(enc, [prompt] * 3, constraint=lst, **dict(kw, **g_over))
    # the same list is fine where the rule that forbade it is off
    assert mirror([[blank, A]], suppress_blank=False) is None
    res = model.generate(enc, [prompt] * 3, constraint=model.constraint_list([[blank, A]]), **dict(kw, suppress_blank=False))
    assert all(r.sequences_ids == [[blank, A]] for r in res)
    # scoring: the same checks against the rules' fields (min_new_tokens is not one), and rules=False
    for phrases, m_over, g_over in cases[:6]:
        lst = ConstraintList(m_over.get("list_vocab", cfg.n_vocab), phrases)
        with pytest.raises(ValueError):
            model.score(enc, [prompt] * 3, [[A]] * 3, rules=True, constraint=lst, suppress_tokens=sup, **g_over)
    with pytest.raises(ValueError):
        model.score(enc, [prompt] * 3, [[A]] * 3, rules=False, constraint=model.constraint_list([[A]]))
    with pytest.raises(TypeError):
        model.generate(enc, [prompt] * 3, constraint=[[A]], **kw)
    with pytest.raises(ValueError):
        model.constraint_list([[cfg.n_vocab]])
    with pytest.raises(ValueError):
        model.constraint_list([[]])


def test_with_a_boost(setup):
    cfg, model, enc = setup
    prompt = _prompt(cfg)
    lst = model.constraint_list(PH9)
    unlisted = 30
    assert unlisted not in {t for p in PH9 for t in p}
    for mode in ("greedy", "beam5"):
        kw = _kw(cfg, mode)
        base = model.generate(enc, [prompt] * 3, return_alternatives=3, constraint=lst, **kw)
        res = model.generate(enc, [prompt] * 3, return_alternatives=3, constraint=lst,
                             boost=model.boost_list([[unlisted], [unlisted, unlisted]], [1e4, 1e4]), **kw)
        _same(res, base, alternatives=True)               # the boosted id is removed before the rules see it
        closed, cut, empty = _guarantee(cfg, res, PH9, NEW)
        assert closed == 3 * MODES[mode].get("num_hypotheses", 1) and cut == 0 and empty == 0
    # a boost on ONE listed phrase among the nine makes it the greedy result (a phrase the unboosted call does not give)
    plain = model.generate(enc, [prompt] * 3, constraint=lst, **_kw(cfg, "greedy"))
    target = next(p for p in ([C, B, A], [21, 22, 23, 24, 25]) if p != plain[0].sequences_ids[0])
    res = model.generate(enc, [prompt] * 3, constraint=lst, boost=model.boost_list([target], [1e4]), **_kw(cfg, "greedy"))
    assert all(r.sequences_ids == [target] for r in res)
