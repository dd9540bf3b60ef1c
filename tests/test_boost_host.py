"""transcribe(boost_phrases=..., phrase_boost=...) on the host (no GPU), on the scripted-backend pattern of
tests/test_alternatives_host.py: a backend whose boost_list records what it is asked to build and whose generate records the
`boost` keyword of every call.  Both entry points and both transcribe_many must build ONE list per call — every phrase
encoded as " " + phrase.strip(), every strength phrase_boost — and hand every generate call that same object; without the
two keywords nothing is built and nothing is passed; phrases without a strength are a ValueError."""
import numpy as np
import pytest

from faster_whisper_amd import get_config
from faster_whisper_amd.transcribe import BatchedInferencePipeline
from oracle import micro_tokenizer
from oracle.scripted_backend import ScriptedBackend
from test_host_golden import make_model

_UNSET = object()
PHRASES = ["  the quick ", "brown fox"]
STRENGTH = 2.5


class FakeBoostList:
    def __init__(self, phrases, boosts):
        self.phrases, self.boosts = [list(p) for p in phrases], list(boosts)


class BoostBackend(ScriptedBackend):
    """the scripted backend plus the two things phrase boosting needs of a backend: boost_list, and generate's `boost`
    keyword — strict: it is recorded whether the keyword was passed at all"""

    def __init__(self, cfg, hf_tok):
        super().__init__(cfg, hf_tok)
        self.built = []            # every list boost_list built
        self.seen = []             # per generate call: the `boost` it got, or _UNSET

    def boost_list(self, phrases, boosts):
        self.built.append(FakeBoostList(phrases, boosts))
        return self.built[-1]

    def generate(self, enc, prompts, *, boost=_UNSET, **kw):
        self.seen.append(boost)
        return super().generate(enc, prompts, **kw)


@pytest.fixture(scope="module")
def hf_tok():
    return micro_tokenizer.build()


def _model(hf_tok):
    m = make_model(get_config("micro"), hf_tok)
    m.model = BoostBackend(get_config("micro"), hf_tok)
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
    assert lst.boosts == [STRENGTH] * len(PHRASES)
    assert len(backend.seen) >= min_calls and all(b is lst for b in backend.seen)


SEQ = dict(language="en", compression_ratio_threshold=None, log_prob_threshold=None, no_speech_threshold=None,
           condition_on_previous_text=False)
BOOST = dict(boost_phrases=PHRASES, phrase_boost=STRENGTH)


def test_sequential_transcribe_hands_every_window_and_attempt_the_same_list(hf_tok):
    m = _model(hf_tok)
    segs, info = m.transcribe(_audio(65), temperature=0.0, **SEQ, **BOOST)
    list(segs)
    _check_one_list(m.model, hf_tok, 3)                      # three windows
    assert not hasattr(info.transcription_options, "boost_phrases")
    # the temperature ladder: thresholds that every attempt fails, so every rung of every window is decoded
    m = _model(hf_tok)
    segs, _ = m.transcribe(_audio(8), language="en", temperature=(0.0, 0.4, 0.8), compression_ratio_threshold=0.0,
                           no_speech_threshold=None, condition_on_previous_text=False, **BOOST)
    list(segs)
    _check_one_list(m.model, hf_tok, 3)


def test_batched_transcribe_hands_every_batch_the_same_list(hf_tok):
    m = _model(hf_tok)
    clips = [{"start": 0.0, "end": 10.0}, {"start": 10.0, "end": 18.0}, {"start": 18.0, "end": 25.0}]
    segs, _ = BatchedInferencePipeline(m).transcribe(_audio(26), language="en", clip_timestamps=clips, batch_size=2, **BOOST)
    list(segs)
    _check_one_list(m.model, hf_tok, 2)                      # two batches


def test_transcribe_many_builds_one_list_for_all_recordings(hf_tok):
    clips = [{"start": 0.0, "end": 10.0}]
    m = _model(hf_tok)
    out = BatchedInferencePipeline(m).transcribe_many([_audio(12), _audio(11, 4), _audio(11, 5)], language="en",
                                                      clip_timestamps=clips, batch_size=2, **BOOST)
    assert len(out) == 3
    _check_one_list(m.model, hf_tok, 2)
    m = _model(hf_tok)
    out = m.transcribe_many([_audio(4), _audio(35, 4)], temperature=0.0, **SEQ, **BOOST)
    assert len(out) == 2
    _check_one_list(m.model, hf_tok, 3)                      # one window + two windows


def test_without_the_keywords_nothing_is_built_or_passed(hf_tok):
    clips = [{"start": 0.0, "end": 10.0}]
    runs = []
    m = _model(hf_tok)
    list(m.transcribe(_audio(8), temperature=0.0, **SEQ)[0])
    runs.append(m)
    m = _model(hf_tok)
    list(BatchedInferencePipeline(m).transcribe(_audio(12), language="en", clip_timestamps=clips)[0])
    runs.append(m)
    m = _model(hf_tok)
    BatchedInferencePipeline(m).transcribe_many([_audio(12)], language="en", clip_timestamps=clips)
    runs.append(m)
    m = _model(hf_tok)
    m.transcribe_many([_audio(4)], temperature=0.0, **SEQ)
    runs.append(m)
    m = _model(hf_tok)                                       # no phrases: a strength alone, or an empty list, is nothing
    list(m.transcribe(_audio(8), temperature=0.0, phrase_boost=1.0, **SEQ)[0])
    list(m.transcribe(_audio(8), temperature=0.0, boost_phrases=[], phrase_boost=1.0, **SEQ)[0])
    runs.append(m)
    for m in runs:
        assert m.model.built == [] and m.model.seen and all(b is _UNSET for b in m.model.seen)


def test_the_boost_does_not_change_what_else_is_passed(hf_tok):
    """the generate calls of a boosted transcribe are those of the plain one, the keyword apart"""
    a, b = _model(hf_tok), _model(hf_tok)
    list(a.transcribe(_audio(8), temperature=0.0, **SEQ)[0])
    list(b.transcribe(_audio(8), temperature=0.0, **SEQ, **BOOST)[0])
    assert a.model.calls == b.model.calls


def test_phrases_without_a_strength_raise(hf_tok):
    clips = [{"start": 0.0, "end": 10.0}]
    m = _model(hf_tok)
    with pytest.raises(ValueError):
        m.transcribe(_audio(4), boost_phrases=PHRASES, **SEQ)
    with pytest.raises(ValueError):
        BatchedInferencePipeline(m).transcribe(_audio(4), language="en", clip_timestamps=clips, boost_phrases=PHRASES)
    with pytest.raises(ValueError):
        m.transcribe_many([_audio(4)], boost_phrases=PHRASES, **SEQ)
    with pytest.raises(ValueError):
        BatchedInferencePipeline(m).transcribe_many([_audio(4)], language="en", clip_timestamps=clips, boost_phrases=PHRASES)
    with pytest.raises(ValueError):                          # one string is not a list of phrases
        m.transcribe(_audio(4), boost_phrases="the quick", phrase_boost=1.0, **SEQ)
    assert m.model.built == [] and m.model.seen == []
