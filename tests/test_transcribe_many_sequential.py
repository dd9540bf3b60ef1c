"""WhisperModel.transcribe_many on the host: the sequential (seek-loop) path over many recordings in one call, the N
transcribe() generators run to completion on a pool of at most `num_workers` threads.  Every recording must come back, in
input order, as exactly what transcribe() alone returns for it — every field of every Segment and of the TranscriptionInfo.
Driven by the scripted backend of the host goldens (oracle/scripted_backend.py: every output is a pure function of the
chunk, the prompt and the temperature, so equality holds whatever runs beside it).  No GPU."""
import dataclasses
import threading

import numpy as np
import pytest

from faster_whisper_amd import get_config
from oracle import host_scenarios as hs
from oracle import micro_tokenizer
from test_host_golden import _close, _plain, make_model

# (seed, seconds, silences): one window, three windows, two windows, one window
SPECS = [(31, 14.0, ()), (32, 70.0, ((21.0, 24.0),)), (33, 45.0, ()), (34, 9.0, ())]


@pytest.fixture(scope="module")
def hf_tok():
    return micro_tokenizer.build()


@pytest.fixture(scope="module")
def audios():
    return [hs.synth_audio(*s) for s in SPECS]


def _model(hf_tok, workers):
    model = make_model(get_config("micro"), hf_tok)
    model.model.inter_threads = workers
    # the scripted backend keeps the level of the last encode on itself between two statements: one encode at a time
    lock, encode = threading.Lock(), model.model.encode

    def locked_encode(*a, **kw):
        with lock:
            return encode(*a, **kw)

    model.model.encode = locked_encode
    return model


def _per(value, i):
    """entry i of a per-recording list; a plain value (a list of token ids is one) as it is"""
    return value[i] if isinstance(value, list) and not all(isinstance(t, int) for t in value) else value


def _serial(hf_tok, audios, language=None, initial_prompt=None, **kw):
    out, logs = [], []
    for i, audio in enumerate(audios):
        model = _model(hf_tok, 1)
        segs, info = model.transcribe(audio, language=_per(language, i), initial_prompt=_per(initial_prompt, i), **kw)
        out.append((list(segs), info))
        logs.append(model.model.calls)
    return out, logs


def _assert_equal(got, want):
    assert len(got) == len(want)
    for i, ((gs, gi), (ws, wi)) in enumerate(zip(got, want)):
        assert isinstance(gs, list)
        _close([_plain(s) for s in gs], [_plain(s) for s in ws], f"rec[{i}].segments")
        assert dataclasses.asdict(gi).keys() == dataclasses.asdict(wi).keys()
        _close(_plain(gi), _plain(wi), f"rec[{i}].info")


def _generate_prompts(log):
    return [p for kind, d in log if kind == "generate" for p in d["prompts"]]


@pytest.mark.parametrize("workers", [1, 3])
def test_results_equal_serial_calls_in_input_order(hf_tok, audios, workers):
    kw = dict(language="en", condition_on_previous_text=True)
    want, logs = _serial(hf_tok, audios, **kw)
    assert len({len(s) for s, _ in want}) > 1 and all(len(s) >= 1 for s, _ in want)   # recordings that differ
    model = _model(hf_tok, workers)
    got = model.transcribe_many(audios, **kw)
    _assert_equal(got, want)
    assert [info.duration for _, info in got] == [s[1] for s in SPECS]                # input order
    # the backend saw every generate call of the serial runs, no more and no fewer (previous text included: the prompts)
    seen = sorted(map(tuple, _generate_prompts(model.model.calls)))
    assert seen == sorted(tuple(p) for log in logs for p in _generate_prompts(log))
    assert len({len(p) for p in seen}) > 1                                            # prompts of different lengths


def test_language_and_initial_prompt_per_recording(hf_tok, audios):
    languages = ["de", "en", None, "es"]
    prompts = [None, "hello there", [7, 8, 9], None]
    kw = dict(temperature=0.0)
    want, logs = _serial(hf_tok, audios, language=languages, initial_prompt=prompts, **kw)
    model = _model(hf_tok, 2)
    got = model.transcribe_many(audios, language=languages, initial_prompt=prompts, **kw)
    _assert_equal(got, want)
    assert [info.language for _, info in got][:2] == ["de", "en"] and got[3][1].language == "es"
    cfg = get_config("micro")
    firsts = [_generate_prompts(log)[0] for log in logs]
    assert firsts[0][0] == cfg.sot and firsts[3][0] == cfg.sot                        # no initial prompt: <sot> first
    assert firsts[1][0] == cfg.sot_prev and firsts[2][:4] == [cfg.sot_prev, 7, 8, 9]  # routed to their recordings
    seen = set(map(tuple, _generate_prompts(model.model.calls)))
    assert all(tuple(f) in seen for f in firsts)
    # one value for all recordings
    want1, _ = _serial(hf_tok, audios[:2], language="en", initial_prompt=[7, 8, 9], **kw)
    _assert_equal(_model(hf_tok, 2).transcribe_many(audios[:2], language="en", initial_prompt=[7, 8, 9], **kw), want1)


def test_argument_errors_and_empty_input(hf_tok, audios):
    model = _model(hf_tok, 2)
    assert model.transcribe_many([]) == []
    with pytest.raises(ValueError, match="language has 2 entries for 4"):
        model.transcribe_many(audios, language=["en", "de"])
    with pytest.raises(ValueError, match="initial_prompt has 3 entries for 4"):
        model.transcribe_many(audios, initial_prompt=["a", None, "b"])
    with pytest.raises(TypeError):
        model.transcribe_many(audios[:1], no_such_keyword=1)


@pytest.mark.parametrize("workers", [1, 3])
def test_an_exception_in_one_recording_surfaces(hf_tok, audios, workers):
    model = _model(hf_tok, workers)
    generate = model.model.generate
    marker = [7, 8, 9]

    def failing_generate(enc, prompts, **kw):
        if any(list(p[1:4]) == marker for p in prompts):
            raise RuntimeError("decode failed for the marked recording")
        return generate(enc, prompts, **kw)

    model.model.generate = failing_generate
    with pytest.raises(RuntimeError, match="marked recording"):
        model.transcribe_many(audios, language="en", initial_prompt=[None, None, marker, None])
    # the model is still usable, and the other recordings are what they always were
    model.model.generate = generate
    want, _ = _serial(hf_tok, audios[:2], language="en")
    _assert_equal(model.transcribe_many(audios[:2], language="en"), want)
