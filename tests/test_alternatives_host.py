"""transcribe(token_alternatives=N) on the host (no GPU), on the scripted-backend pattern of
tests/test_token_logprobs_host.py: a fake backend whose generate returns scripted ids with timestamp tokens, scripted
per-token log-probs and scripted per-token alternatives.  Both entry points must yield AlternativesSegments whose
token_alternatives (and token_logprobs) are the scripted values at the indices of their tokens — cut along the sub-segments
exactly as the tokens are — with every other field the default run's; the backend sees `return_alternatives` only when it
was asked for, and never `return_token_logprobs` beside it."""
import dataclasses

import numpy as np
import pytest

from faster_whisper_amd import WhisperGenerationResult, get_config
from faster_whisper_amd.transcribe import AlternativesSegment, BatchedInferencePipeline, ScoredSegment, Segment
from oracle import micro_tokenizer
from oracle.scripted_backend import ScriptedBackend
from test_host_golden import make_model

_UNSET = object()
SEGMENT_FIELDS = ["id", "seek", "start", "end", "text", "tokens", "avg_logprob", "compression_ratio", "no_speech_prob",
                  "words", "temperature"]


class FakeBackend(ScriptedBackend):
    """generate: chunk n of the backend's life gets script n % 2 (three closed sub-segments | one closed and one ended by a
    lone timestamp), token i of chunk n the log-prob -(100 n + i + 1) / 1000 and the alternatives
    [(id, lp), (1000 n + 10 i + j, lp - j) for j = 1 .. N - 1].  The signature is strict: an unknown keyword is an error,
    and which of the two value keywords were passed at all is recorded."""

    def __init__(self, cfg, hf_tok):
        super().__init__(cfg, hf_tok)
        self.n_chunks = 0
        self.seen = []             # (return_token_logprobs passed, return_alternatives passed or its value) per call
        self.scripted = []         # (ids, log-probs, alternatives) per chunk, in call order

    def generate(self, enc, prompts, *, beam_size=5, patience=1, num_hypotheses=1, length_penalty=1,
                 repetition_penalty=1, no_repeat_ngram_size=0, max_length=448, return_scores=False,
                 return_no_speech_prob=False, max_initial_timestamp_index=50, suppress_blank=True,
                 suppress_tokens=None, sampling_topk=1, sampling_temperature=1, return_token_logprobs=_UNSET,
                 return_alternatives=_UNSET):
        self.seen.append((return_token_logprobs is not _UNSET, None if return_alternatives is _UNSET else return_alternatives))
        tb = self.config.timestamp_begin
        a = self.pool
        out = []
        for _ in prompts:
            n = self.n_chunks
            self.n_chunks += 1
            if n % 2 == 0:
                ids = [tb, a[0], a[1], tb + 50, tb + 50, a[2], a[3], a[4], tb + 100, tb + 100, a[5], a[6], tb + 150, tb + 150]
            else:
                ids = [tb, a[7], a[8], tb + 40, tb + 40, a[9], a[10], tb + 90]
            lps = [-(100 * n + i + 1) / 1000.0 for i in range(len(ids))]
            end = -(100 * n + 99) / 1000.0
            N = 0 if return_alternatives is _UNSET else int(return_alternatives)
            alts = [[(t, lp)] + [(1000 * n + 10 * i + j, lp - j) for j in range(1, N)] for i, (t, lp) in enumerate(zip(ids, lps))]
            self.scripted.append((ids, lps, alts))
            score = (sum(lps) + end) / (len(ids) ** length_penalty)
            res = WhisperGenerationResult([list(ids)], [score], 0.01)
            if return_token_logprobs is True or N:
                res.token_logprobs, res.end_logprobs = [list(lps)], [end]
            if N:
                res.token_alternatives, res.end_alternatives = [alts], [[(self.config.eot, end)] * N]
            out.append(res)
        return out


@pytest.fixture(scope="module")
def hf_tok():
    return micro_tokenizer.build()


def _model(hf_tok):
    m = make_model(get_config("micro"), hf_tok)
    m.model = FakeBackend(get_config("micro"), hf_tok)
    return m


def _audio(seconds):
    rng = np.random.default_rng(3)
    return (0.1 * rng.standard_normal(int(seconds * 16000))).astype(np.float32)


def _check(on, off, backend_on, expect_tokens, N):
    assert len(on) == len(off) > 0
    for s_on, s_off in zip(on, off):
        assert type(s_on) is AlternativesSegment and isinstance(s_on, ScoredSegment) and type(s_off) is Segment
        d_on = dataclasses.asdict(s_on)
        alts, lps = d_on.pop("token_alternatives"), d_on.pop("token_logprobs")
        assert d_on == dataclasses.asdict(s_off)
        assert len(alts) == len(lps) == len(s_on.tokens) and all(len(a) == N for a in alts)
    by_chunk = {}
    for s in on:
        by_chunk.setdefault(s.seek, []).append(s)
    assert len(by_chunk) == len(expect_tokens) == len(backend_on.scripted)
    for (seek, segs), (ids, lps, alts), n in zip(sorted(by_chunk.items()), backend_on.scripted, expect_tokens):
        toks = [t for s in segs for t in s.tokens]
        assert len(toks) == n and toks == ids[:n]
        assert [x for s in segs for x in s.token_logprobs] == lps[:n]
        assert [a for s in segs for a in s.token_alternatives] == alts[:n]
        for s in segs:                                   # aligned to the tokens: entry 0 of the script is the token itself
            assert [a[0][0] for a in s.token_alternatives] == s.tokens


def test_segment_field_lists():
    assert [f.name for f in dataclasses.fields(Segment)] == SEGMENT_FIELDS
    assert [f.name for f in dataclasses.fields(ScoredSegment)] == SEGMENT_FIELDS + ["token_logprobs"]
    assert [f.name for f in dataclasses.fields(AlternativesSegment)] == SEGMENT_FIELDS + ["token_logprobs", "token_alternatives"]
    r = WhisperGenerationResult([[1, 2]], [-0.5], 0.1)
    assert r.token_alternatives == [] and r.end_alternatives == []


@pytest.mark.parametrize("word_timestamps", [False, True])
def test_batched_pipeline_yields_alternatives_segments(hf_tok, word_timestamps):
    clips = [{"start": 0.0, "end": 10.0}, {"start": 10.0, "end": 18.0}]
    kw = dict(language="en", clip_timestamps=clips, without_timestamps=False, batch_size=2, word_timestamps=word_timestamps)
    runs = {}
    for n_alt in (0, 2):
        m = _model(hf_tok)
        extra = dict(token_alternatives=2) if n_alt else {}
        segs, info = BatchedInferencePipeline(m).transcribe(_audio(20), **kw, **extra)
        runs[n_alt] = (list(segs), m.model)
        assert "token_alternatives" not in dataclasses.asdict(info.transcription_options)
    assert runs[0][1].seen == [(False, None)] and runs[2][1].seen == [(False, 2)]
    assert [len(s.tokens) for s in runs[2][0]] == [4, 5, 4, 4, 4]        # three sub-segments, then two
    _check(runs[2][0], runs[0][0], runs[2][1], [13, 8], 2)
    assert runs[2][0][1].token_alternatives[0] == [(runs[2][0][1].tokens[0], -0.005), (41, -1.005)]
    assert runs[2][0][4].token_alternatives[-1][1] == (1071, -1.108)     # chunk 1, token 7: ends on the lone timestamp


def test_sequential_transcribe_yields_alternatives_segments(hf_tok):
    kw = dict(language="en", temperature=0.0, compression_ratio_threshold=None, log_prob_threshold=None,
              no_speech_threshold=None, condition_on_previous_text=False)
    runs = {}
    for n_alt in (0, 3):
        m = _model(hf_tok)
        extra = dict(token_alternatives=3) if n_alt else {}
        segs, _ = m.transcribe(_audio(8), **kw, **extra)
        runs[n_alt] = (list(segs), m.model)
    assert runs[0][1].seen == [(False, None)] * 2 and runs[3][1].seen == [(False, 3)] * 2
    assert [s.seek for s in runs[3][0]] == [0, 0, 0, 300, 300]
    _check(runs[3][0], runs[0][0], runs[3][1], [13, 8], 3)


def test_token_logprobs_alone_still_passes_its_own_keyword_only(hf_tok):
    m = _model(hf_tok)
    segs, _ = BatchedInferencePipeline(m).transcribe(_audio(9), language="en", clip_timestamps=[{"start": 0.0, "end": 9.0}],
                                                     without_timestamps=False, token_logprobs=True)
    assert all(type(s) is ScoredSegment for s in segs) and m.model.seen == [(True, None)]


def test_transcribe_many_passes_it_per_recording(hf_tok):
    clips = [{"start": 0.0, "end": 10.0}]
    m = _model(hf_tok)
    out = BatchedInferencePipeline(m).transcribe_many([_audio(12), _audio(11)], language="en", clip_timestamps=clips,
                                                      without_timestamps=False, batch_size=2, token_alternatives=2)
    assert m.model.seen == [(False, 2)]
    assert [[type(s) for s in segs] for segs, _ in out] == [[AlternativesSegment] * 3, [AlternativesSegment] * 2]
    assert out[1][0][0].token_alternatives[1] == [(out[1][0][0].tokens[1], -0.102), (1011, -1.102)]
    m = _model(hf_tok)
    out = BatchedInferencePipeline(m).transcribe_many([_audio(12)], language="en", clip_timestamps=clips,
                                                      without_timestamps=False)
    assert m.model.seen == [(False, None)] and all(type(s) is Segment for s in out[0][0])
    # the sequential transcribe_many: every recording's transcribe() gets the keyword
    kw = dict(language="en", temperature=0.0, compression_ratio_threshold=None, log_prob_threshold=None,
              no_speech_threshold=None, condition_on_previous_text=False)
    m = _model(hf_tok)
    out = m.transcribe_many([_audio(4), _audio(4)], token_alternatives=2, **kw)
    assert len(out) == 2 and all(type(s) is AlternativesSegment for segs, _ in out for s in segs)
    assert m.model.seen and all(s == (False, 2) for s in m.model.seen)
    m = _model(hf_tok)
    out = m.transcribe_many([_audio(4)], **kw)
    assert all(s == (False, None) for s in m.model.seen) and all(type(s) is Segment for s in out[0][0])


def test_shard_refuses_the_keyword(hf_tok):
    with pytest.raises(ValueError):
        BatchedInferencePipeline(_model(hf_tok)).transcribe(_audio(5), language="en", shard=True, token_alternatives=2)
