"""transcribe_many(token_logprobs=True) on the GPU: three recordings (1, 1 and 2 chunks: the bursts of
tests/test_gpu_transcribe_many.py) in ONE call on a `micro` model with the micro tokenizer, timestamps on, so that chunks
split into sub-segments.

  * every segment is a ScoredSegment and every other field is the default call's, exactly;
  * per chunk, its sub-segments' tokens / token_logprobs are the chunk's generate() ids / log-probs index for index (the
    sub-segments are consecutive slices from index 0: together a prefix of the chunk);
  * the chunk's avg_logprob * (n + 1) is the sum of ALL its token log-probs plus the end value, within 1e-5.  The call runs
    at length_penalty 0, where the score is the cumulative log-prob itself: at length_penalty 1 the score is a float32
    quotient whose rounding alone, times n, is of the order of 1e-5 at the |cum| of about 60 these chunks reach, and the
    check would measure that division instead of the bookkeeping.  The sum is taken in float32 in order, as the engine's."""
import dataclasses

import numpy as np
import pytest

from test_gpu_c5 import peaked_vad_weights, recording
from test_gpu_transcribe_many import BURSTS, VAD

pytestmark = pytest.mark.gpu

RECS = [0, 1, 4]
CHUNKS = [1, 1, 2]


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
                       max_batch_size=4, max_beam_size=5)
    dev = fvad.SileroVADModel(weights=peaked_vad_weights(), device="cuda")
    recs = [recording(BURSTS[i], seed=200 + 10 * i) for i in RECS]
    kw = dict(language="en", beam_size=5, batch_size=4, vad_filter=True, vad_parameters=VAD, max_new_tokens=14,
              without_timestamps=False, length_penalty=0.0, suppress_tokens=[1, 2, 3])
    return cfg, gpu, dev, recs, kw


def _sum32(values):
    c = np.float32(0)
    for x in values:
        c = np.float32(c + np.float32(x))
    return float(c)


def test_transcribe_many_token_logprobs(setup, monkeypatch):
    from faster_whisper_amd.transcribe import BatchedInferencePipeline, ScoredSegment, Segment
    cfg, gpu, dev, recs, kw = setup
    plain = BatchedInferencePipeline(gpu).transcribe_many(recs, vad_model=dev, **kw)
    chunks = []                       # every chunk's generate() result, in decode order
    generate = gpu.model.generate

    def recording_generate(*a, **k):
        assert k.get("return_token_logprobs") is True
        res = generate(*a, **k)
        chunks.extend((r.sequences_ids[0], r.token_logprobs[0], r.end_logprobs[0]) for r in res)
        return res

    monkeypatch.setattr(gpu.model, "generate", recording_generate)
    scored = BatchedInferencePipeline(gpu).transcribe_many(recs, vad_model=dev, token_logprobs=True, **kw)
    assert len(chunks) == sum(CHUNKS)                 # one batch of four chunks across the recordings
    it = iter(chunks)
    n_sub = []
    for r, ((ss, si), (ps, pi)) in enumerate(zip(scored, plain)):
        assert dataclasses.asdict(si) == dataclasses.asdict(pi)
        assert len(ss) == len(ps) > 0
        for a, b in zip(ss, ps):
            assert type(a) is ScoredSegment and type(b) is Segment
            d = dataclasses.asdict(a)
            lps = d.pop("token_logprobs")
            assert d == dataclasses.asdict(b), r                           # every other field, exactly
            assert len(lps) == len(a.tokens)
        by_chunk = {}
        for s in ss:
            by_chunk.setdefault(s.seek, []).append(s)
        assert len(by_chunk) == CHUNKS[r]                                  # every chunk gave segments
        for seek, segs in sorted(by_chunk.items()):
            ids, lps, end = next(it)
            n_sub.append(len(segs))
            toks = [t for s in segs for t in s.tokens]
            got = [x for s in segs for x in s.token_logprobs]
            assert toks == ids[:len(toks)] and got == lps[:len(toks)], (r, seek)
            n = len(ids)
            assert ids[0] >= cfg.timestamp_begin and 0 < n <= 14
            total = _sum32(list(lps) + [end])
            assert abs(segs[0].avg_logprob * (n + 1) - total) <= 1e-5, (r, seek, segs[0].avg_logprob * (n + 1), total)
            assert all(s.avg_logprob == segs[0].avg_logprob for s in segs)
    print(f"sub-segments per chunk: {n_sub}")
    assert max(n_sub) > 1                             # at least one chunk was split: the slicing had work to do
