"""BatchedInferencePipeline.transcribe_many on the GPU: five recordings — bursts of noise between digital silence that
the native device VAD (one fw_vad_forward_audio_batch_dev call for all of them) cuts into 1, 1, 3, 0 and 2 chunks — go
through ONE call whose batches of 4 chunks span recording boundaries.  Every recording's result must be EXACTLY what its
own transcribe() call gives on the same VAD probabilities: tokens, times, avg_logprob, no_speech_prob, words with their
boundaries and probabilities.  No tolerance and no chunk left out: the engine's result for a chunk does not depend on what
shares its batch or its decode run (test_gpu_pipeline.py, test_gpu_merged_run.py assert that bit for bit)."""
import dataclasses

import numpy as np
import pytest

from test_gpu_c5 import peaked_vad_weights, recording

pytestmark = pytest.mark.gpu

# (speech s, gap s) per burst.  The batched path's VAD options (spans padded by 0.4 s, chunks of at most 30 s) merge them
# into: one chunk of two bursts | one chunk | 14 + 13, 12 + 11, 9 + 10 | nothing | 16, 15
BURSTS = [[(5.0, 2.0), (4.0, 0.5)],
          [(7.0, 0.6)],
          [(14.0, 1.0), (13.0, 1.0), (12.0, 1.2), (11.0, 0.8), (9.0, 1.0), (10.0, 0.5)],
          None,
          [(16.0, 1.0), (15.0, 1.0)]]
CHUNKS = [1, 1, 3, 0, 2]
# the batched path's default silence, and a minimum length: from its zero state the peaked network calls the first few
# windows of digital silence speech (a span of 0.16 s), which is not what the silent recording is here for
VAD = dict(min_silence_duration_ms=160, min_speech_duration_ms=250)


@pytest.fixture(scope="module")
def setup():
    from faster_whisper_amd import get_config, synthetic_weights
    from faster_whisper_amd import vad as fvad
    from faster_whisper_amd.transcribe import WhisperModel
    from oracle import micro_tokenizer
    cfg = get_config("micro")
    tok = micro_tokenizer.build()
    gpu = WhisperModel("synthetic:micro", device="cuda", compute_type="float16",
                       files={"config": cfg, "weights": synthetic_weights(cfg, seed=33),
                              "tokenizer.json": tok.to_str().encode()},
                       max_batch_size=16, max_beam_size=5)
    dev = fvad.SileroVADModel(weights=peaked_vad_weights(), device="cuda")
    recs = [np.zeros(16000 * 6, np.float32) if b is None else recording(b, seed=200 + 10 * i)
            for i, b in enumerate(BURSTS)]
    # the device probabilities of every recording, by the single-recording call: what the per-recording runs are fed
    probs = [dev(np.pad(a, (0, 512 - len(a) % 512))) for a in recs]
    # (synthetic weights: most of micro's vocabulary are timestamp ids; suppressing them leaves words to time)
    kw = dict(beam_size=5, batch_size=4, word_timestamps=True, vad_filter=True, vad_parameters=VAD, max_new_tokens=14,
              suppress_tokens=[1, 2, 3] + list(range(cfg.timestamp_begin, cfg.n_vocab)))
    return gpu, dev, recs, probs, kw


def _fields(segments):
    return [dataclasses.asdict(s) for s in segments]


def _info(info):
    return dataclasses.asdict(info)


def _run_both(setup, **more):
    from faster_whisper_amd import vad as fvad
    from faster_whisper_amd.transcribe import BatchedInferencePipeline
    gpu, dev, recs, probs, kw = setup
    kw = dict(kw, **more)
    spans = [fvad.get_speech_timestamps(a, fvad.VadOptions(max_speech_duration_s=30, **VAD), speech_probs=p)
             for a, p in zip(recs, probs)]
    chunks = [len(fvad.collect_chunks(a, sp, max_duration=30)[0]) if sp else 0 for a, sp in zip(recs, spans)]
    assert chunks == CHUNKS and len(spans[0]) == 2, (chunks, spans[0])
    before = gpu.model.decode_stats()["requests"]
    got = BatchedInferencePipeline(gpu).transcribe_many(recs, vad_model=dev, **kw)
    pooled = gpu.model.decode_stats()["requests"] - before
    want = []
    for a, p in zip(recs, probs):
        segs, info = BatchedInferencePipeline(gpu).transcribe(a, vad_speech_probs=p, **kw)
        want.append((list(segs), info))
    single = gpu.model.decode_stats()["requests"] - before - pooled
    return got, want, pooled, single


def test_transcribe_many_equals_the_per_recording_calls_exactly(setup):
    got, want, pooled, single = _run_both(setup, language="en")
    assert len(got) == 5
    for r, ((gs, gi), (ws, wi)) in enumerate(zip(got, want)):
        assert _fields(gs) == _fields(ws), r                       # every field of every Segment and Word, exactly
        assert _info(gi) == _info(wi), r
        assert len({s.seek for s in gs}) == CHUNKS[r]              # every chunk gave segments: none was left out
        assert [s.id for s in gs] == list(range(1, len(gs) + 1))
        assert all(s.words for s in gs)
    assert got[3][0] == [] and got[3][1].duration_after_vad == 0
    # restore_speech_timestamps had work to do: the second burst of recording 0 (two spans in one chunk, asserted with the
    # chunk counts) lies behind a removed silence
    assert got[0][1].duration - got[0][1].duration_after_vad > 0.5
    # 7 chunks in batches of 4 across recording boundaries: 2 generate calls, against one per non-empty recording
    assert (pooled, single) == (2, 4)


def test_language_detection_in_batches_equals_the_per_recording_calls(setup):
    """language=None: the first segments of all five recordings are detected in batches (the silent one too); language,
    probability and all_language_probs are the per-recording call's, and so is everything decoded under that language"""
    got, want, _, _ = _run_both(setup, language=None)
    for r, ((gs, gi), (ws, wi)) in enumerate(zip(got, want)):
        assert (gi.language, gi.language_probability, gi.all_language_probs) == \
               (wi.language, wi.language_probability, wi.all_language_probs), r
        assert _info(gi) == _info(wi) and _fields(gs) == _fields(ws), r
