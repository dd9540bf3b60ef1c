"""BatchedInferencePipeline.transcribe_many on the host: many recordings in one call, their chunks pooled into batches
across recording boundaries, must return for every recording exactly what `transcribe` on a fresh pipeline returns for
it — every field of every Segment / Word and of the TranscriptionInfo — while the backend sees full batches.  Driven by
the scripted backend of the host goldens (oracle/scripted_backend.py: every output is a pure function of the chunk, so
equality holds whatever shares a batch).  No GPU."""
import dataclasses
from math import ceil

import numpy as np
import pytest

from faster_whisper_amd import get_config
from faster_whisper_amd import vad as fvad
from faster_whisper_amd.transcribe import BatchedInferencePipeline
from oracle import host_scenarios as hs
from oracle import micro_tokenizer
from test_host_golden import _close, _plain, make_model

# three recordings of one chunk, one of three, one of two, one of pure silence (None)
SPECS = [(21, 12.0, ()), (22, 20.0, ()), (23, 8.0, ()), (24, 75.0, ((20.0, 23.0), (48.0, 51.0))),
         (25, 50.0, ((24.0, 27.0),)), None]
CHUNKS = [1, 1, 1, 3, 2, 0]


@pytest.fixture(scope="module")
def hf_tok():
    return micro_tokenizer.build()


@pytest.fixture(scope="module")
def recordings():
    audios = [np.zeros(160000, np.float32) if s is None else hs.synth_audio(*s) for s in SPECS]
    probs = [hs.speech_probs(np.pad(a, (0, 512 - a.shape[0] % 512))) for a in audios]
    return audios, probs


def _per(value, i):
    """entry i of a per-recording list; a plain value (a list of clip dicts is one) as it is"""
    return value[i] if isinstance(value, list) and not isinstance(value[0], dict) else value


def _single_calls(hf_tok, audios, probs, language=None, clip_timestamps=None, workers=1, **kw):
    """transcribe() per recording on a fresh model + pipeline -> (results, the backend call log of every recording)"""
    out, logs = [], []
    for i, audio in enumerate(audios):
        model = make_model(get_config("micro"), hf_tok)
        model.model.inter_threads = workers
        segs, info = BatchedInferencePipeline(model).transcribe(
            audio, language=_per(language, i), clip_timestamps=_per(clip_timestamps, i),
            vad_speech_probs=probs[i], **kw)
        out.append((list(segs), info))
        logs.append(model.model.calls)
    return out, logs


def _many(hf_tok, audios, workers=1, **kw):
    model = make_model(get_config("micro"), hf_tok)
    model.model.inter_threads = workers
    return BatchedInferencePipeline(model).transcribe_many(audios, **kw), model.model.calls


def _assert_equal(got, want):
    assert len(got) == len(want)
    for i, ((gs, gi), (ws, wi)) in enumerate(zip(got, want)):
        assert isinstance(gs, list)
        _close([_plain(s) for s in gs], [_plain(s) for s in ws], f"rec[{i}].segments")
        assert dataclasses.asdict(gi).keys() == dataclasses.asdict(wi).keys()
        _close(_plain(gi), _plain(wi), f"rec[{i}].info")


def _chunks_of(log):
    return [fp for kind, d in log if kind == "encode" for fp in d]


@pytest.mark.parametrize("extra", [dict(word_timestamps=True), dict(without_timestamps=False)],
                         ids=["word_timestamps", "with_timestamps"])
def test_six_recordings_equal_the_per_recording_calls_and_are_pooled(hf_tok, recordings, extra):
    audios, probs = recordings
    kw = dict(language="en", batch_size=4, **extra)
    want, logs = _single_calls(hf_tok, audios, probs, **kw)
    assert [len(_chunks_of(log)) for log in logs] == CHUNKS
    assert any(len(s) > 1 for s, _ in want) and want[5][0] == [] and want[5][1].duration_after_vad == 0
    got, calls = _many(hf_tok, audios, vad_speech_probs=probs, **kw)
    _assert_equal(got, want)
    assert [s.id for s in got[3][0]] == list(range(1, len(got[3][0]) + 1))       # ids start at 1 per recording
    # pooling: the chunks of all recordings in recording order, a batch every 4 chunks, across recording boundaries
    pooled = [fp for log in logs for fp in _chunks_of(log)]
    assert len(pooled) == 8
    encodes = [d for kind, d in calls if kind == "encode"]
    assert encodes == [pooled[:4], pooled[4:]]               # recordings 0, 1, 2 + the head of 3 | the rest of 3 + 4
    n_generate = [kind for kind, _ in calls].count("generate")
    assert n_generate == ceil(8 / 4) == 2 < sum(1 for log in logs for kind, _ in log if kind == "generate")
    if extra.get("word_timestamps"):
        assert [len(d["n"]) for kind, d in calls if kind == "align"] == [4, 4]
        assert all(s.words for s, _ in got[:5] for s in s)


def test_batches_in_flight_keep_the_result(hf_tok, recordings):
    """worker replicas: the pooled batches are decoded concurrently, every recording's result stays the serial one"""
    audios, probs = recordings
    kw = dict(language="en", batch_size=1, word_timestamps=True)
    want, _ = _single_calls(hf_tok, audios, probs, **kw)
    got, calls = _many(hf_tok, audios, workers=3, vad_speech_probs=probs, **kw)
    _assert_equal(got, want)
    assert [kind for kind, _ in calls].count("generate") == 8


def test_language_per_recording_never_mixes_languages_in_a_batch(hf_tok, recordings):
    audios, probs = recordings
    languages = ["de", "en", "de", "en", "de", "en"]
    kw = dict(batch_size=4, word_timestamps=True)
    want, logs = _single_calls(hf_tok, audios, probs, language=languages, **kw)
    got, calls = _many(hf_tok, audios, language=languages, vad_speech_probs=probs, **kw)
    _assert_equal(got, want)
    assert [i.language for _, i in got] == languages
    generates = [d for kind, d in calls if kind == "generate"]
    for d in generates:
        assert len({tuple(p) for p in d["prompts"]}) == 1                         # one prompt = one language per batch
    assert len({tuple(d["prompts"][0]) for d in generates}) == 2
    # per language the pool is in recording order: de = recordings 0, 2, 4 (1 + 1 + 2 chunks), en = 1, 3 (1 + 3)
    fps = [_chunks_of(log) for log in logs]
    assert [d for kind, d in calls if kind == "encode"] == [fps[0] + fps[2] + fps[4], fps[1] + fps[3]]


def test_language_detection_is_batched_and_falls_back_per_recording(hf_tok, recordings):
    audios, probs = recordings
    kw = dict(batch_size=4, language_detection_segments=2, language_detection_threshold=0.7)
    want, logs = _single_calls(hf_tok, audios, probs, language=None, **kw)
    n_detect = [[kind for kind, _ in log].count("detect_language") for log in logs]
    # the scripted model is sure of recording 2 and of the silence at once; 3 and 4 have a second segment to look at
    # (3 becomes sure there, 4 ends in the majority vote); 0 and 1 have no second segment
    assert n_detect == [1, 1, 1, 2, 2, 1]
    assert want[2][1].language_probability > 0.7 > want[4][1].language_probability
    got, calls = _many(hf_tok, audios, language=None, vad_speech_probs=probs, **kw)
    _assert_equal(got, want)
    assert all(i.all_language_probs for _, i in got)
    # the first segments of all six recordings (the silent one too: it still gets a language) in batches of 4
    first = [next(d for kind, d in log if kind == "detect_language") for log in logs]
    detects = [d for kind, d in calls if kind == "detect_language"]
    assert detects[0] == [f[0] for f in first[:4]]
    # recording 3 fell under the threshold in that batch: its second segment follows alone, then the next batch
    assert len(detects[1]) == 1 and len(detects) == 4 and detects[2] == [f[0] for f in first[4:]]
    assert calls[0][0] == "encode" and calls[0][1] == detects[0] and calls[1][0] == "detect_language"
    assert sum(len(d) for d in detects) == sum(n_detect)


def test_clip_timestamps_and_speech_probs_per_recording(hf_tok, recordings):
    audios, probs = recordings
    clips = [None, [dict(start=1.0, end=9.5), dict(start=9.5, end=19.0)], None,
             [dict(start=0.0, end=29.0), dict(start=30.0, end=55.0), dict(start=55.0, end=74.0)], None, None]
    # recordings 0 and 2 swap their probability tracks' role: 2 is given a track that calls its second half silence
    p = list(probs)
    p[2] = probs[2].copy()
    p[2][len(p[2]) // 2:] = 0.01
    kw = dict(language="en", batch_size=4, word_timestamps=True)
    want, logs = _single_calls(hf_tok, audios, p, clip_timestamps=clips, **kw)
    assert want[2][1].duration_after_vad < 0.75 * want[2][1].duration              # the given track was used
    got, calls = _many(hf_tok, audios, clip_timestamps=clips, vad_speech_probs=p, **kw)
    _assert_equal(got, want)
    assert got[1][1].transcription_options.clip_timestamps == clips[1] and got[1][1].vad_options is None
    assert got[0][1].vad_options == fvad.VadOptions(max_speech_duration_s=30, min_silence_duration_ms=160)
    assert [len(_chunks_of(log)) for log in logs] == [1, 2, 1, 3, 2, 0]


def test_one_value_applies_to_every_recording(hf_tok, recordings):
    audios, probs = recordings
    audios = audios[:3]
    clips = [dict(start=0.5, end=4.0), dict(start=4.0, end=7.5)]
    kw = dict(language="zh", clip_timestamps=clips, batch_size=4, without_timestamps=False)
    want, _ = _single_calls(hf_tok, audios, [None] * 3, **kw)
    got, calls = _many(hf_tok, audios, **kw)
    _assert_equal(got, want)
    assert [i.language for _, i in got] == ["zh"] * 3 and [len(d) for kind, d in calls if kind == "encode"] == [4, 2]
    # one probability track for all: three copies of one recording
    same = [audios[0]] * 3
    want, _ = _single_calls(hf_tok, same, [probs[0]] * 3, language="en")
    got, _ = _many(hf_tok, same, language="en", vad_speech_probs=probs[0])
    _assert_equal(got, want)
    with pytest.raises(ValueError):
        _many(hf_tok, audios, language=["en", "de"], vad_speech_probs=probs[:3])


def test_the_vad_runs_once_for_all_recordings(hf_tok, recordings):
    """no probabilities given: ONE forward_many of the model serves every recording that needs the VAD"""
    audios, probs = recordings
    seen = []

    class Model:
        def forward_many(self, padded):
            seen.append([len(a) for a in padded])
            return [hs.speech_probs(a) for a in padded]

    clips = [None, [dict(start=1.0, end=9.5)], None, None, None, None]
    kw = dict(language="en", batch_size=4)
    want, _ = _single_calls(hf_tok, audios, probs, clip_timestamps=clips, **kw)
    got, _ = _many(hf_tok, audios, clip_timestamps=clips, vad_model=Model(), **kw)
    _assert_equal(got, want)
    assert seen == [[len(a) + 512 - len(a) % 512 for i, a in enumerate(audios) if i != 1]]
    got, _ = _many(hf_tok, audios, clip_timestamps=clips, vad_model=hs.speech_probs, **kw)      # a plain callable
    _assert_equal(got, want)


def test_shard_is_refused_and_no_recordings_give_no_results(hf_tok, recordings):
    audios, probs = recordings
    with pytest.raises(ValueError):
        _many(hf_tok, audios, shard=True, vad_speech_probs=probs)
    got, calls = _many(hf_tok, [])
    assert got == [] and calls == []
    with pytest.raises(TypeError):
        _many(hf_tok, audios, no_such_keyword=1)


def test_get_speech_timestamps_many_equals_the_per_recording_calls():
    tracks = hs.vad_prob_tracks()
    audios = [np.zeros(n, np.float32) for n, _ in tracks.values()]
    given = [p for _, p in tracks.values()]
    for opts in hs.VAD_CASES.values():
        o = fvad.VadOptions(**opts)
        got = fvad.get_speech_timestamps_many(audios, o, speech_probs=given)
        assert got == [fvad.get_speech_timestamps(a, o, speech_probs=p) for a, p in zip(audios, given)]
    assert any(len(g) > 1 for g in got)
    # a mix: the model runs (once) for the recordings without probabilities only
    rec = [hs.synth_audio(31, 6.0, ((2.0, 4.0),)), hs.synth_audio(32, 3.0)]
    calls = []

    def model(padded):
        calls.append(len(padded))
        return hs.speech_probs(padded)
    got = fvad.get_speech_timestamps_many(rec, speech_probs=[None, hs.speech_probs(np.pad(rec[1], (0, 512 - len(rec[1]) % 512)))],
                                          vad_model=model, min_silence_duration_ms=300)
    assert calls == [96256]
    assert got == [fvad.get_speech_timestamps(a, vad_model=hs.speech_probs, min_silence_duration_ms=300) for a in rec]
    assert len(got[0]) == 2
    assert fvad.get_speech_timestamps_many([]) == []


def test_forward_many_on_the_host_equals_the_per_recording_calls():
    from test_vad_network import synthetic_weights
    model = fvad.SileroVADModel(weights=synthetic_weights(7), n_threads=2)
    rng = np.random.default_rng(5)
    recs = [(0.2 * rng.standard_normal(512 * n)).astype(np.float32) for n in (1, 2, 37, 0, 5)]
    got = model.forward_many(recs)
    assert [g.shape[0] for g in got] == [1, 2, 37, 0, 5]
    for a, g in zip(recs, got):
        if a.shape[0]:
            assert np.array_equal(g, model(a))
    assert model.forward_many([]) == []
