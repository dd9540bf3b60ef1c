"""transcribe(token_alternatives=3) on the GPU: the 5 s speech clip of tests/golden/ through BatchedInferencePipeline.transcribe
and through the sequential WhisperModel.transcribe, on a `micro` model with the micro tokenizer, timestamps on.

  * every segment is an AlternativesSegment; texts, tokens, token_logprobs and every other field equal those of the
    token_logprobs=True run, exactly;
  * for every token the identities of tests/test_gpu_alternatives.py hold on the segments: the list is sorted, a token that
    is in its list has its recorded log-prob there bit for bit, one that is not lies at or below the list's last entry."""
import dataclasses
import os

import numpy as np
import pytest

from alternatives_refs import check_alternatives

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def setup():
    from faster_whisper_amd import get_config, synthetic_weights
    from faster_whisper_amd.transcribe import WhisperModel
    from oracle import micro_tokenizer
    cfg = get_config("micro")
    tok = micro_tokenizer.build()
    gpu = WhisperModel("synthetic:micro", device="cuda", compute_type="float16",
                       files={"config": cfg, "weights": synthetic_weights(cfg, seed=33),
                              "tokenizer.json": tok.to_str().encode()},
                       max_batch_size=4, max_beam_size=5)
    pcm = np.load(os.path.join(GOLD, "speech_pcm.npz"))["pcm"].astype(np.float32)
    return cfg, gpu, pcm


def _check(on, ref):
    from faster_whisper_amd.transcribe import AlternativesSegment, ScoredSegment
    assert len(on) == len(ref) > 0
    n_tok = found = 0
    for a, b in zip(on, ref):
        assert type(a) is AlternativesSegment and type(b) is ScoredSegment
        d = dataclasses.asdict(a)
        alts = d.pop("token_alternatives")
        assert d == dataclasses.asdict(b)                     # text, tokens, token_logprobs and every other field
        assert len(a.token_alternatives) == len(a.tokens) and all(len(x) == 3 for x in a.token_alternatives)
        found += check_alternatives(a.tokens, a.token_logprobs, a.token_alternatives)
        n_tok += len(a.tokens)
    return n_tok, found


def test_batched_pipeline_alternatives(setup):
    from faster_whisper_amd.transcribe import BatchedInferencePipeline
    cfg, gpu, pcm = setup
    kw = dict(language="en", beam_size=5, batch_size=4, clip_timestamps=[{"start": 0.0, "end": len(pcm) / 16000.0}],
              max_new_tokens=14, without_timestamps=False, length_penalty=0.0, suppress_tokens=[1, 2, 3])
    ref = list(BatchedInferencePipeline(gpu).transcribe(pcm, token_logprobs=True, **kw)[0])
    on = list(BatchedInferencePipeline(gpu).transcribe(pcm, token_alternatives=3, **kw)[0])
    n_tok, found = _check(on, ref)
    print(f"batched: {len(on)} segment(s), {n_tok} tokens, {found} of them among their 3 alternatives")
    assert found > 0


def test_sequential_transcribe_alternatives(setup):
    cfg, gpu, pcm = setup
    kw = dict(language="en", beam_size=5, temperature=0.0, max_new_tokens=14, without_timestamps=False, length_penalty=0.0,
              suppress_tokens=[1, 2, 3], compression_ratio_threshold=None, log_prob_threshold=None, no_speech_threshold=None,
              condition_on_previous_text=False)
    ref = list(gpu.transcribe(pcm, token_logprobs=True, **kw)[0])
    on = list(gpu.transcribe(pcm, token_alternatives=3, **kw)[0])
    n_tok, found = _check(on, ref)
    print(f"sequential: {len(on)} segment(s), {n_tok} tokens, {found} of them among their 3 alternatives")
    assert found > 0
