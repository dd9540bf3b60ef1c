"""The decode extras (token_logprobs, token_alternatives, boost_phrases / phrase_boost, allowed_phrases, sampling_top_k,
sampling_top_p) from the four entry points down to model.generate, without a GPU, on the scripted-backend pattern of
tests/test_constrain_host.py.  The four entry points: WhisperModel.transcribe / transcribe_many and
BatchedInferencePipeline.transcribe / transcribe_many.

  - a call that uses no extra passes no extra keyword anywhere: not at an internal boundary (generate_segments,
    generate_with_fallback, _batched_segments_generator, _batches_in_flight, _decode_batch, generate_segment_batched), not
    at model.generate;
  - a call that uses all six hands every internal boundary ONE DecodeExtras — the same object everywhere, for every
    recording — and every generate call exactly the keywords that are set: return_alternatives (never return_token_logprobs
    beside it), the two lists, each built once, and top_k / top_p on the sampled rungs of the fallback ladder only;
  - every argument the three checks refuse is a ValueError from every entry point, before anything is built or decoded."""
import numpy as np
import pytest

from faster_whisper_amd import get_config
from faster_whisper_amd.transcribe import BatchedInferencePipeline, DecodeExtras
from oracle import micro_tokenizer
from oracle.scripted_backend import ScriptedBackend
from test_host_golden import make_model

_UNSET = object()
GENERATE_KEYWORDS = ("return_token_logprobs", "return_alternatives", "boost", "constraint", "top_k", "top_p")
EXTRA_NAMES = {"token_logprobs", "token_alternatives", "boost", "constraint", "sampling_top_k", "sampling_top_p", "extras"}
MODEL_BOUNDARIES = ("generate_segments", "generate_with_fallback")
PIPELINE_BOUNDARIES = ("_batched_segments_generator", "_batches_in_flight", "_decode_batch", "generate_segment_batched")
N_ALT = 2
STRENGTH = 2.5


class FakeList:
    def __init__(self, phrases, boosts=None):
        self.phrases, self.boosts = [list(p) for p in phrases], boosts


class ExtrasBackend(ScriptedBackend):
    """the scripted backend plus the list builders and generate's six extra keywords — strict: per generate call it records
    the sampling temperature (None for a beam call) and which of the six were passed at all, with their values"""

    def __init__(self, cfg, hf_tok):
        super().__init__(cfg, hf_tok)
        self.built_boost, self.built_constraint, self.seen = [], [], []

    def boost_list(self, phrases, boosts):
        self.built_boost.append(FakeList(phrases, list(boosts)))
        return self.built_boost[-1]

    def constraint_list(self, phrases):
        self.built_constraint.append(FakeList(phrases))
        return self.built_constraint[-1]

    def generate(self, enc, prompts, *, return_token_logprobs=_UNSET, return_alternatives=_UNSET, boost=_UNSET,
                 constraint=_UNSET, top_k=_UNSET, top_p=_UNSET, **kw):
        passed = dict(zip(GENERATE_KEYWORDS, (return_token_logprobs, return_alternatives, boost, constraint, top_k, top_p)))
        sampled = kw.get("sampling_topk", 1) == 0
        self.seen.append((kw.get("sampling_temperature") if sampled else None,
                          {k: v for k, v in passed.items() if v is not _UNSET}))
        out = super().generate(enc, prompts, **kw)
        if return_alternatives is not _UNSET or return_token_logprobs is not _UNSET:
            n_alt = 0 if return_alternatives is _UNSET else return_alternatives
            for r in out:
                r.token_logprobs = [[-0.5] * len(ids) for ids in r.sequences_ids]
                r.end_logprobs = [-0.25] * len(r.sequences_ids)
                if n_alt:
                    r.token_alternatives = [[[(t, -0.5)] * n_alt for t in ids] for ids in r.sequences_ids]
                    r.end_alternatives = [[(self.config.eot, -0.25)] * n_alt] * len(r.sequences_ids)
        return out


@pytest.fixture(scope="module")
def hf_tok():
    return micro_tokenizer.build()


def _audio(seconds, seed=3):
    rng = np.random.default_rng(seed)
    return (0.1 * rng.standard_normal(int(seconds * 16000))).astype(np.float32)


def _record(obj, names, log):
    """every call of obj.<name> is logged as (name, positional arguments, keywords) and then made"""
    for name in names:
        inner = getattr(obj, name)

        def outer(*args, _inner=inner, _name=name, **kw):
            log.append((_name, args, kw))
            return _inner(*args, **kw)
        setattr(obj, name, outer)


# thresholds that every attempt fails: every rung of every window is decoded
LADDER = dict(language="en", temperature=(0.0, 0.4, 0.8), compression_ratio_threshold=0.0, no_speech_threshold=None,
              condition_on_previous_text=False)
BATCHED = dict(language="en", clip_timestamps=[{"start": 0.0, "end": 10.0}, {"start": 10.0, "end": 18.0}], batch_size=1)
ALL_SIX = dict(token_logprobs=True, token_alternatives=N_ALT, boost_phrases=["brown fox"], phrase_boost=STRENGTH,
               allowed_phrases=["  the quick ", "brown fox"], sampling_top_k=40, sampling_top_p=0.9)


def _run(entry, hf_tok, **extra):
    """one call of an entry point on a fresh model -> (backend, the boundary log, the boundaries the entry goes through)"""
    m = make_model(get_config("micro"), hf_tok)
    m.model = ExtrasBackend(get_config("micro"), hf_tok)
    pipe = BatchedInferencePipeline(m)
    log = []
    _record(m, MODEL_BOUNDARIES, log)
    _record(pipe, PIPELINE_BOUNDARIES, log)
    if entry == "transcribe":
        list(m.transcribe(_audio(8), **LADDER, **extra)[0])
    elif entry == "transcribe_many":
        assert len(m.transcribe_many([_audio(4), _audio(5, 4)], **LADDER, **extra)) == 2
    elif entry == "batched":
        list(pipe.transcribe(_audio(19), **BATCHED, **extra)[0])
    else:
        assert len(pipe.transcribe_many([_audio(19), _audio(19, 4)], **BATCHED, **extra)) == 2
    crossed = {name for name, _, _ in log}
    if entry in ("transcribe", "transcribe_many"):
        assert crossed == set(MODEL_BOUNDARIES)
    else:   # (the many-recordings entry pools its batches itself: it does not go through the per-recording generator)
        assert crossed == set(PIPELINE_BOUNDARIES) - ({"_batched_segments_generator"} if entry == "batched_many" else set())
    return m.model, log


ENTRIES = ("transcribe", "transcribe_many", "batched", "batched_many")


@pytest.mark.parametrize("entry", ENTRIES)
def test_without_extras_no_boundary_and_no_generate_call_sees_a_keyword(hf_tok, entry):
    backend, log = _run(entry, hf_tok)
    assert log and backend.seen
    for name, args, kw in log:
        assert not EXTRA_NAMES & set(kw), (name, sorted(kw))
        assert not any(isinstance(a, DecodeExtras) for a in args), name
    assert all(passed == {} for _, passed in backend.seen)
    assert backend.built_boost == [] and backend.built_constraint == []


@pytest.mark.parametrize("entry", ENTRIES)
def test_with_all_six_every_boundary_gets_one_carrier_and_generate_exactly_what_is_set(hf_tok, entry):
    backend, log = _run(entry, hf_tok, **ALL_SIX)
    # each list built once, from " " + phrase.strip()
    enc = lambda phrases: [hf_tok.encode(" " + p.strip(), add_special_tokens=False).ids for p in phrases]
    assert len(backend.built_boost) == 1 and len(backend.built_constraint) == 1
    boost, constraint = backend.built_boost[0], backend.built_constraint[0]
    assert boost.phrases == enc(ALL_SIX["boost_phrases"]) and boost.boosts == [STRENGTH]
    assert constraint.phrases == enc(ALL_SIX["allowed_phrases"])
    # ONE carrier, the same object at every boundary, and nothing else that names an extra
    carriers = []
    for name, args, kw in log:
        assert EXTRA_NAMES & set(kw) == {"extras"}, (name, sorted(kw))
        assert not any(isinstance(a, DecodeExtras) for a in args), name
        carriers.append(kw["extras"])
    assert all(c is carriers[0] for c in carriers)
    assert carriers[0] == DecodeExtras(token_logprobs=True, token_alternatives=N_ALT, boost=boost, constraint=constraint,
                                       sampling_top_k=40, sampling_top_p=0.9)
    # every generate call: the alternatives keyword alone stands for both value keywords, both lists, and the sampling limits
    # on the sampled rungs only (the batched entries decode every chunk once, without sampling)
    always = dict(return_alternatives=N_ALT, boost=boost, constraint=constraint)
    for temperature, passed in backend.seen:
        assert passed == (always if temperature is None else dict(always, top_k=40, top_p=0.9)), (temperature, passed)
        assert passed["boost"] is boost and passed["constraint"] is constraint
    rungs = sorted((t for t, _ in backend.seen), key=str)
    if entry == "transcribe":
        assert rungs == sorted([None, 0.4, 0.8], key=str)
    elif entry == "transcribe_many":
        assert rungs == sorted([None, 0.4, 0.8] * 2, key=str)
    else:
        assert rungs == [None] * (2 if entry == "batched" else 4)


# one example per branch of the three argument checks
BAD = [dict(boost_phrases="brown fox", phrase_boost=STRENGTH),      # a bare string
       dict(boost_phrases=["brown fox", 3], phrase_boost=STRENGTH),   # not all strings
       dict(boost_phrases=["brown fox"]),                             # phrases without a strength
       dict(allowed_phrases=b"brown fox"),                            # a bare byte string
       dict(allowed_phrases=["brown fox", None]),                     # not all strings
       dict(sampling_top_k=-1), dict(sampling_top_k=True), dict(sampling_top_k=2.5),
       dict(sampling_top_p=0.0), dict(sampling_top_p="0.9")]


@pytest.mark.parametrize("bad", BAD)
def test_a_refused_argument_is_a_value_error_from_every_entry_point(hf_tok, bad):
    for entry in ENTRIES:
        m = make_model(get_config("micro"), hf_tok)
        m.model = ExtrasBackend(get_config("micro"), hf_tok)
        pipe = BatchedInferencePipeline(m)
        with pytest.raises(ValueError):
            if entry == "transcribe":
                m.transcribe(_audio(4), **LADDER, **bad)
            elif entry == "transcribe_many":
                m.transcribe_many([_audio(4)], **LADDER, **bad)
            elif entry == "batched":
                pipe.transcribe(_audio(4), **BATCHED, **bad)
            else:
                pipe.transcribe_many([_audio(4)], **BATCHED, **bad)
        assert m.model.seen == [] and m.model.built_boost == [] and m.model.built_constraint == []
