"""Constrained decoding on the host (no GPU).

  - fw_constraint_create: every FW_EINVAL, the empty list, and what the compiled table is a function of — the SET of
    phrases: equal arguments give byte-equal tables, and so do another order of the phrases and repeated phrases (the
    table holds the phrases sorted by their ids, each once); a different set gives different bytes;
  - fw_test_constrain_rows_host (the compiled table walked in plain C++, sharing its match function with the kernel)
    against the numpy restatement of tests/constrain_refs.py, the whole logits bit for bit;
  - transcribe(allowed_phrases=...) on the scripted-backend pattern of tests/test_boost_host.py: both entry points and both
    transcribe_many build ONE list per call — every phrase encoded as " " + phrase.strip() — and hand every generate call
    that same object; without the keyword nothing is built and nothing is passed; a bare string is a ValueError; and it
    composes with boost_phrases."""
import numpy as np
import pytest

import constrain_refs as cr
from faster_whisper_amd import _lib, get_config
from faster_whisper_amd.transcribe import BatchedInferencePipeline
from oracle import micro_tokenizer
from oracle.scripted_backend import ScriptedBackend
from test_host_golden import make_model

V, EOT, TSB = 500, 400, 412


# ---- fw_constraint_create ----
def _refused(n_vocab, phrases):
    rc, h = cr.create_rc(n_vocab, phrases)
    if rc == 0:
        _lib.load().fw_constraint_free(h)
    assert (rc != 0) == (cr.create_error(n_vocab, phrases) is not None), (rc, cr.create_error(n_vocab, phrases))
    assert rc in (0, -1)
    return rc != 0


def test_create_refuses_what_the_contract_lists():
    assert _refused(0, [[1]])                                            # n_vocab < 1
    assert _refused(V, [[1]] * (cr.MAX_PHRASES + 1))                     # too many phrases
    assert _refused(V, [[1], []])                                        # a phrase of no token
    assert _refused(V, [[1] * (cr.MAX_LEN + 1)])                         # a phrase of 33
    assert _refused(V, [[1] * cr.MAX_LEN] * (cr.MAX_TOKENS // cr.MAX_LEN) + [[2]])   # 4097 tokens in all
    assert _refused(V, [[1, V]])                                         # an id outside the vocabulary
    assert _refused(V, [[-1]])
    lib = _lib.load()
    import ctypes as C
    h = C.c_void_p()
    flat, offs = cr.ragged([[1, 2], [3]])
    assert lib.fw_constraint_create(V, None, _lib.as_i32p(offs), 2, C.byref(h)) == -1      # null tokens with phrases
    assert lib.fw_constraint_create(V, _lib.as_i32p(flat), None, 2, C.byref(h)) == -1
    assert lib.fw_constraint_create(V, _lib.as_i32p(flat), _lib.as_i32p(offs), 2, None) == -1
    bad = offs.copy()
    bad[0] = 1
    assert lib.fw_constraint_create(V, _lib.as_i32p(flat), _lib.as_i32p(bad), 2, C.byref(h)) == -1   # offsets[0] != 0
    bad = np.asarray([0, 3, 2], dtype=np.int32)
    assert lib.fw_constraint_create(V, _lib.as_i32p(flat), _lib.as_i32p(bad), 2, C.byref(h)) == -1   # offsets decrease
    # the limits themselves are valid: 1024 phrases, a phrase of 32, 4096 tokens, duplicates, a prefix of another phrase
    assert not _refused(V, [[j % V] for j in range(cr.MAX_PHRASES)])
    assert not _refused(V, [[1] * cr.MAX_LEN] * (cr.MAX_TOKENS // cr.MAX_LEN))
    assert not _refused(V, [[1, 2], [1, 2], [1], [1, 2, 3]])


def test_empty_list_is_valid_and_touches_nothing():
    import ctypes as C
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.fw_constraint_create(V, None, None, 0, C.byref(h)) == 0 and h
    lib.fw_constraint_free(h)
    empty = cr.Constraint(V, [])
    lg = (np.random.default_rng(0).standard_normal((3, V)) * 4).astype(np.float32)
    # an empty list has no phrase: walked as a table it allows nothing (no text id, no <eot>) — the engine never walks it,
    # fw_generate_constrain and fw_score_constrain turn it into "no constraint" (tests/test_gpu_constrain.py)
    got = cr.rows_host(lg, [[], [1], [2, 3]], empty, EOT, TSB, True)
    assert np.array_equal(cr.bits(got), cr.bits(cr.constrain_rows(lg, [], [[], [1], [2, 3]], EOT, TSB, True)))
    assert empty.table()[0] == 0


def test_the_table_is_a_function_of_the_set_of_phrases():
    phrases = [[7, 8, 9], [7], [300, 2], [7, 8], [1] * 32]
    a, b = cr.Constraint(V, phrases), cr.Constraint(V, [list(p) for p in phrases])
    assert a.table().tobytes() == b.table().tobytes()                    # equal arguments: equal bytes
    # defined here: the table holds the phrases sorted, each once — order and repeats do not change its bytes
    shuffled = cr.Constraint(V, [phrases[i] for i in (3, 0, 4, 2, 1)])
    repeated = cr.Constraint(V, phrases + [phrases[2], phrases[0]])
    assert shuffled.table().tobytes() == a.table().tobytes() == repeated.table().tobytes()
    assert cr.Constraint(V, phrases[:-1]).table().tobytes() != a.table().tobytes()       # another set
    assert cr.Constraint(V + 1, phrases).table().tobytes() != a.table().tobytes()        # another vocabulary
    t = a.table()
    assert t[0] == len(phrases) and t[1] == sum(len(p) for p in phrases)


# ---- the host walk against the reference ----
def _logits(rows, seed, n_vocab=V):
    lg = (np.random.default_rng(seed).standard_normal((rows, n_vocab)) * 4).astype(np.float32)
    lg[0, 3] = -np.inf
    lg[-1, 5] = np.float32(3e38)
    return lg


def _check_host(phrases, hists, seed, n_vocab=V, eot=EOT, tsb=TSB):
    lg = _logits(len(hists), seed, n_vocab)
    c = cr.Constraint(n_vocab, phrases)
    for with_ts in (False, True):
        want = cr.constrain_rows(lg, phrases, hists, eot, tsb, with_ts)
        got = cr.rows_host(lg, hists, c, eot, tsb, with_ts)
        assert np.array_equal(cr.bits(got), cr.bits(want)), np.argwhere(cr.bits(got) != cr.bits(want))[:8]
    return want


def test_host_walk_duplicates_prefixes_and_lengths():
    long = list(range(100, 132))
    phrases = [[7], [7, 8], [7, 8], [7, 8, 9], [7, 9], long, [40], [40]]
    ts = TSB + 5
    hists = [[], [7], [7, 8], [7, 8, 9], [7, 8, 9, 1], [8], long[:31], long, long + [1], long + [long[0]] * 2,
             [ts, 7, ts, ts, 8], [ts], [40], [7, ts + 1, 9, ts + 2], [ts] * 50 + long[:5]]
    want = _check_host(phrases, hists, 1)
    assert sorted(np.flatnonzero(want[0, :TSB] != -np.inf)) == [7, 40, 100]          # the roots (3 is -inf on input)
    assert EOT in np.flatnonzero(want[1, :TSB] != -np.inf) and 8 in np.flatnonzero(want[1, :TSB] != -np.inf)
    assert np.all(want[4, :TSB] == -np.inf) and np.all(want[8, :TSB] == -np.inf)     # left the list: nothing, no <eot>
    assert list(np.flatnonzero(want[7, :TSB] != -np.inf)) == [EOT]                   # the 32-token phrase, complete


def test_host_walk_random_lists_and_a_wide_root():
    rng = np.random.default_rng(5)
    for seed in range(4):
        n_ph = int(rng.integers(1, 60))
        phrases = [[int(t) for t in rng.integers(0, 12, size=int(rng.integers(1, 6)))] for _ in range(n_ph)]
        phrases += [list(p) for p in phrases[:3]] + [phrases[0][:1]]
        hists = []
        for _ in range(12):
            p = phrases[int(rng.integers(len(phrases)))]
            h = p[:int(rng.integers(0, len(p) + 1))] + ([int(rng.integers(0, 12))] if rng.random() < 0.3 else [])
            hists.append([x for t in h for x in ([TSB + int(rng.integers(0, 50))] if rng.random() < 0.2 else []) + [t]])
        _check_host(phrases, hists, 10 + seed)
    # a root with more than 256 distinct first ids, and second tokens behind some of them
    firsts = [int(t) for t in rng.choice(EOT, size=300, replace=False)]
    phrases = [[f] for f in firsts[:150]] + [[f, (f + 1) % EOT] for f in firsts[150:]]
    want = _check_host(phrases, [[], [firsts[0]], [firsts[200]], [firsts[299], 0]], 20)
    assert np.count_nonzero(want[0, :TSB] != -np.inf) >= 299
    # the full table: 128 phrases of 32 tokens = 4096 tokens, the three real vocabulary sizes' geometry
    phrases = [[int(t) for t in rng.integers(0, 50000, size=32)] for _ in range(128)]
    _check_host(phrases, [[], phrases[5][:31], phrases[127], phrases[9][:3] + [1]], 21, n_vocab=51866, eot=50257, tsb=50365)


def test_hook_refuses_wrong_geometry():
    c = cr.Constraint(V, [[1]])
    lg = _logits(1, 2)
    for eot, tsb in ((TSB, TSB), (-1, TSB), (EOT, V + 1)):
        with pytest.raises(ValueError):
            cr.rows_host(lg, [[]], c, eot, tsb, True)
    with pytest.raises(ValueError):
        cr.rows_host(_logits(1, 2, V + 1), [[]], c, EOT, TSB, True)      # a list for another vocabulary
    with pytest.raises(ValueError):
        cr.rows_host(lg, [[V]], c, EOT, TSB, True)                       # a history id outside the vocabulary


def test_call_validation_mirror():
    """the mirror of fw_generate_constrain's checks (tests/test_gpu_constrain.py runs it against the engine)"""
    base = dict(list_vocab=V, n_vocab=V, eot=EOT, suppress=[1, 2], suppress_blank=True, suppress_begin=(5, EOT), ngram=0,
                min_new=0)
    assert cr.call_error([[20, 5]], **base) is None
    assert cr.call_error([[20]], **dict(base, list_vocab=V + 1)) == "vocabulary"
    assert cr.call_error([[20, EOT]], **base) == "id >= eot"
    assert cr.call_error([[20, 2]], **base) == "suppressed id"
    assert cr.call_error([[5, 20]], **base) == "suppress_blank"
    assert cr.call_error([[5, 20]], **dict(base, suppress_blank=False)) is None
    assert cr.call_error([[20]], **dict(base, ngram=2)) == "no_repeat_ngram_size"
    assert cr.call_error([[20]], **dict(base, min_new=1)) == "min_new_tokens"
    assert cr.call_error([], **dict(base, ngram=2, min_new=1)) is None


# ---- transcribe(allowed_phrases=...) on a scripted backend ----
_UNSET = object()
PHRASES = ["  the quick ", "brown fox"]
STRENGTH = 2.5


class FakeList:
    def __init__(self, phrases, boosts=None):
        self.phrases, self.boosts = [list(p) for p in phrases], boosts


class ConstraintBackend(ScriptedBackend):
    """the scripted backend plus what constrained decoding (and the boost it composes with) needs of a backend:
    constraint_list / boost_list, and generate's `constraint` / `boost` keywords — strict: it is recorded whether each
    keyword was passed at all"""

    def __init__(self, cfg, hf_tok):
        super().__init__(cfg, hf_tok)
        self.built, self.built_boost = [], []
        self.seen, self.seen_boost = [], []

    def constraint_list(self, phrases):
        self.built.append(FakeList(phrases))
        return self.built[-1]

    def boost_list(self, phrases, boosts):
        self.built_boost.append(FakeList(phrases, list(boosts)))
        return self.built_boost[-1]

    def generate(self, enc, prompts, *, constraint=_UNSET, boost=_UNSET, **kw):
        self.seen.append(constraint)
        self.seen_boost.append(boost)
        return super().generate(enc, prompts, **kw)


@pytest.fixture(scope="module")
def hf_tok():
    return micro_tokenizer.build()


def _model(hf_tok):
    m = make_model(get_config("micro"), hf_tok)
    m.model = ConstraintBackend(get_config("micro"), hf_tok)
    return m


def _audio(seconds, seed=3):
    rng = np.random.default_rng(seed)
    return (0.1 * rng.standard_normal(int(seconds * 16000))).astype(np.float32)


def _expect(hf_tok):
    return [hf_tok.encode(" " + p.strip(), add_special_tokens=False).ids for p in PHRASES]


def _check_one_list(backend, hf_tok, min_calls):
    assert len(backend.built) == 1
    lst = backend.built[0]
    assert lst.phrases == _expect(hf_tok) and all(len(p) >= 1 for p in lst.phrases)
    assert len(backend.seen) >= min_calls and all(c is lst for c in backend.seen)
    assert backend.built_boost == [] and all(b is _UNSET for b in backend.seen_boost)


SEQ = dict(language="en", compression_ratio_threshold=None, log_prob_threshold=None, no_speech_threshold=None,
           condition_on_previous_text=False)
ALLOWED = dict(allowed_phrases=PHRASES)
CLIPS = [{"start": 0.0, "end": 10.0}]


def test_sequential_transcribe_hands_every_window_and_attempt_the_same_list(hf_tok):
    m = _model(hf_tok)
    segs, info = m.transcribe(_audio(65), temperature=0.0, **SEQ, **ALLOWED)
    list(segs)
    _check_one_list(m.model, hf_tok, 3)                      # three windows
    assert not hasattr(info.transcription_options, "allowed_phrases")
    m = _model(hf_tok)                                       # the ladder: every rung of every window is decoded
    segs, _ = m.transcribe(_audio(8), language="en", temperature=(0.0, 0.4, 0.8), compression_ratio_threshold=0.0,
                           no_speech_threshold=None, condition_on_previous_text=False, **ALLOWED)
    list(segs)
    _check_one_list(m.model, hf_tok, 3)


def test_batched_transcribe_hands_every_batch_the_same_list(hf_tok):
    m = _model(hf_tok)
    clips = [{"start": 0.0, "end": 10.0}, {"start": 10.0, "end": 18.0}, {"start": 18.0, "end": 25.0}]
    segs, _ = BatchedInferencePipeline(m).transcribe(_audio(26), language="en", clip_timestamps=clips, batch_size=2, **ALLOWED)
    list(segs)
    _check_one_list(m.model, hf_tok, 2)                      # two batches


def test_transcribe_many_builds_one_list_for_all_recordings(hf_tok):
    m = _model(hf_tok)
    out = BatchedInferencePipeline(m).transcribe_many([_audio(12), _audio(11, 4), _audio(11, 5)], language="en",
                                                      clip_timestamps=CLIPS, batch_size=2, **ALLOWED)
    assert len(out) == 3
    _check_one_list(m.model, hf_tok, 2)
    m = _model(hf_tok)
    out = m.transcribe_many([_audio(4), _audio(35, 4)], temperature=0.0, **SEQ, **ALLOWED)
    assert len(out) == 2
    _check_one_list(m.model, hf_tok, 3)                      # one window + two windows


def test_without_the_keyword_nothing_is_built_or_passed(hf_tok):
    runs = []
    m = _model(hf_tok)
    list(m.transcribe(_audio(8), temperature=0.0, **SEQ)[0])
    runs.append(m)
    m = _model(hf_tok)
    list(BatchedInferencePipeline(m).transcribe(_audio(12), language="en", clip_timestamps=CLIPS)[0])
    runs.append(m)
    m = _model(hf_tok)
    BatchedInferencePipeline(m).transcribe_many([_audio(12)], language="en", clip_timestamps=CLIPS)
    runs.append(m)
    m = _model(hf_tok)
    m.transcribe_many([_audio(4)], temperature=0.0, **SEQ)
    runs.append(m)
    m = _model(hf_tok)                                       # an empty list is nothing
    list(m.transcribe(_audio(8), temperature=0.0, allowed_phrases=[], **SEQ)[0])
    runs.append(m)
    for m in runs:
        assert m.model.built == [] and m.model.seen and all(c is _UNSET for c in m.model.seen)


def test_the_list_does_not_change_what_else_is_passed(hf_tok):
    a, b = _model(hf_tok), _model(hf_tok)
    list(a.transcribe(_audio(8), temperature=0.0, **SEQ)[0])
    list(b.transcribe(_audio(8), temperature=0.0, **SEQ, **ALLOWED)[0])
    assert a.model.calls == b.model.calls


def test_a_bare_string_and_non_strings_raise(hf_tok):
    m = _model(hf_tok)
    for bad in ("the quick", b"the quick", ["the quick", 3]):
        with pytest.raises(ValueError):
            m.transcribe(_audio(4), allowed_phrases=bad, **SEQ)
        with pytest.raises(ValueError):
            BatchedInferencePipeline(m).transcribe(_audio(4), language="en", clip_timestamps=CLIPS, allowed_phrases=bad)
        with pytest.raises(ValueError):
            m.transcribe_many([_audio(4)], allowed_phrases=bad, **SEQ)
        with pytest.raises(ValueError):
            BatchedInferencePipeline(m).transcribe_many([_audio(4)], language="en", clip_timestamps=CLIPS, allowed_phrases=bad)
    assert m.model.built == [] and m.model.seen == []


def test_it_composes_with_boost_phrases(hf_tok):
    """both keywords: one list of each kind per call, every generate call gets both objects"""
    boost = dict(boost_phrases=["brown fox"], phrase_boost=STRENGTH)

    def check(backend, min_calls):
        assert len(backend.built) == 1 and len(backend.built_boost) == 1
        assert backend.built[0].phrases == _expect(hf_tok)
        assert backend.built_boost[0].phrases == [_expect(hf_tok)[1]] and backend.built_boost[0].boosts == [STRENGTH]
        assert len(backend.seen) >= min_calls
        assert all(c is backend.built[0] for c in backend.seen) and all(b is backend.built_boost[0] for b in backend.seen_boost)

    m = _model(hf_tok)
    list(m.transcribe(_audio(65), temperature=0.0, **SEQ, **ALLOWED, **boost)[0])
    check(m.model, 3)
    m = _model(hf_tok)
    list(BatchedInferencePipeline(m).transcribe(_audio(12), language="en", clip_timestamps=CLIPS, **ALLOWED, **boost)[0])
    check(m.model, 1)
    m = _model(hf_tok)
    BatchedInferencePipeline(m).transcribe_many([_audio(12), _audio(11, 4)], language="en", clip_timestamps=CLIPS,
                                                batch_size=1, **ALLOWED, **boost)
    check(m.model, 2)
    m = _model(hf_tok)
    m.transcribe_many([_audio(4), _audio(35, 4)], temperature=0.0, **SEQ, **ALLOWED, **boost)
    check(m.model, 3)
