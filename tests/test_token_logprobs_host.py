"""transcribe(token_logprobs=True) on the host (no GPU): a fake backend whose generate returns scripted ids with timestamp
tokens and scripted per-token log-probs.  Both entry points must yield ScoredSegments whose token_logprobs are the
scripted values at the indices of their tokens, with every other field the default run's; with the keyword off the
backend never sees `return_token_logprobs` and plain Segments come out.  Plus the numpy reference of the beam update's
log-prob bookkeeping (tests/token_logprob_refs.py) checked against the identity it exists for."""
import dataclasses

import numpy as np
import pytest

from faster_whisper_amd import WhisperGenerationResult, get_config
from faster_whisper_amd.transcribe import BatchedInferencePipeline, ScoredSegment, Segment
from oracle import micro_tokenizer
from oracle.scripted_backend import ScriptedBackend
from test_host_golden import make_model

_UNSET = object()
SEGMENT_FIELDS = ["id", "seek", "start", "end", "text", "tokens", "avg_logprob", "compression_ratio", "no_speech_prob",
                  "words", "temperature"]


class FakeBackend(ScriptedBackend):
    """generate: chunk n of the backend's life gets script n % 2 —
         0: three sub-segments closed by timestamp pairs (the second timestamp of the last pair belongs to no sub-segment),
         1: one closed sub-segment and one ended by a lone timestamp —
       and token i of chunk n the log-prob -(100 n + i + 1) / 1000.  The signature is strict: an unknown keyword is an
       error, and whether return_token_logprobs was passed at all is recorded."""

    def __init__(self, cfg, hf_tok):
        super().__init__(cfg, hf_tok)
        self.n_chunks = 0
        self.seen_keyword = []
        self.scripted = []         # (ids, log-probs, end log-prob) per chunk, in call order

    def generate(self, enc, prompts, *, beam_size=5, patience=1, num_hypotheses=1, length_penalty=1,
                 repetition_penalty=1, no_repeat_ngram_size=0, max_length=448, return_scores=False,
                 return_no_speech_prob=False, max_initial_timestamp_index=50, suppress_blank=True,
                 suppress_tokens=None, sampling_topk=1, sampling_temperature=1, return_token_logprobs=_UNSET):
        self.seen_keyword.append(return_token_logprobs is not _UNSET)
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
            self.scripted.append((ids, lps, end))
            score = (sum(lps) + end) / (len(ids) ** length_penalty)
            res = WhisperGenerationResult([list(ids)], [score], 0.01)
            if return_token_logprobs is True:
                res.token_logprobs, res.end_logprobs = [list(lps)], [end]
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


def _check(on, off, backend_on, expect_tokens):
    """on / off: the segments of the run with and without the keyword; expect_tokens: per chunk (in order) the number of
    its tokens that belong to sub-segments"""
    assert len(on) == len(off) > 0
    for s_on, s_off in zip(on, off):
        assert type(s_on) is ScoredSegment and isinstance(s_on, Segment) and type(s_off) is Segment
        d_on = dataclasses.asdict(s_on)
        lps = d_on.pop("token_logprobs")
        assert d_on == dataclasses.asdict(s_off)
        assert len(lps) == len(s_on.tokens)
    # per chunk: its sub-segments' tokens / log-probs are the scripted ones, index for index
    by_chunk = {}
    for s in on:
        by_chunk.setdefault(s.seek, []).append(s)
    assert len(by_chunk) == len(expect_tokens) == len(backend_on.scripted)
    for (seek, segs), (ids, lps, _), n in zip(sorted(by_chunk.items()), backend_on.scripted, expect_tokens):
        toks = [t for s in segs for t in s.tokens]
        got = [x for s in segs for x in s.token_logprobs]
        assert len(toks) == n and toks == ids[:n] and got == lps[:n], (seek, toks, got)


def test_segment_field_list_is_unchanged():
    assert [f.name for f in dataclasses.fields(Segment)] == SEGMENT_FIELDS
    assert [f.name for f in dataclasses.fields(ScoredSegment)] == SEGMENT_FIELDS + ["token_logprobs"]
    r = WhisperGenerationResult([[1, 2]], [-0.5], 0.1)          # the three-argument constructor keeps working
    assert r.token_logprobs == [] and r.end_logprobs == []


@pytest.mark.parametrize("word_timestamps", [False, True])
def test_batched_pipeline_yields_scored_segments(hf_tok, word_timestamps):
    clips = [{"start": 0.0, "end": 10.0}, {"start": 10.0, "end": 18.0}]
    kw = dict(language="en", clip_timestamps=clips, without_timestamps=False, batch_size=2, word_timestamps=word_timestamps)
    runs = {}
    for flag in (False, True):
        m = _model(hf_tok)
        extra = dict(token_logprobs=True) if flag else {}
        segs, info = BatchedInferencePipeline(m).transcribe(_audio(20), **kw, **extra)
        runs[flag] = (list(segs), m.model)
        assert "token_logprobs" not in dataclasses.asdict(info.transcription_options)
    assert runs[False][1].seen_keyword == [False] and runs[True][1].seen_keyword == [True]
    assert [len(s.tokens) for s in runs[True][0]] == [4, 5, 4, 4, 4]     # three sub-segments, then two
    _check(runs[True][0], runs[False][0], runs[True][1], [13, 8])
    assert runs[True][0][1].token_logprobs == [-0.005, -0.006, -0.007, -0.008, -0.009]
    assert runs[True][0][4].token_logprobs == [-0.105, -0.106, -0.107, -0.108]          # ends on the lone timestamp


def test_transcribe_many_forwards_the_keyword(hf_tok):
    clips = [{"start": 0.0, "end": 10.0}]
    m = _model(hf_tok)
    out = BatchedInferencePipeline(m).transcribe_many([_audio(12), _audio(11)], language="en", clip_timestamps=clips,
                                                      without_timestamps=False, batch_size=2, token_logprobs=True)
    assert m.model.seen_keyword == [True]
    assert [[type(s) for s in segs] for segs, _ in out] == [[ScoredSegment] * 3, [ScoredSegment] * 2]
    assert out[1][0][0].token_logprobs == [-0.101, -0.102, -0.103, -0.104]
    m = _model(hf_tok)
    out = BatchedInferencePipeline(m).transcribe_many([_audio(12)], language="en", clip_timestamps=clips,
                                                      without_timestamps=False)
    assert m.model.seen_keyword == [False] and all(type(s) is Segment for s in out[0][0])


def test_sequential_transcribe_yields_scored_segments(hf_tok):
    """the seek loop: window 0 (script 0) ends at its last timestamp pair (3.0 s), window 1 (script 1) on a lone
    timestamp; the values are those of the result the fallback ladder kept (one temperature, no thresholds: one call)"""
    kw = dict(language="en", temperature=0.0, compression_ratio_threshold=None, log_prob_threshold=None,
              no_speech_threshold=None, condition_on_previous_text=False)
    runs = {}
    for flag in (False, True):
        m = _model(hf_tok)
        extra = dict(token_logprobs=True) if flag else {}
        segs, _ = m.transcribe(_audio(8), **kw, **extra)
        runs[flag] = (list(segs), m.model)
    assert runs[False][1].seen_keyword == [False, False] and runs[True][1].seen_keyword == [True, True]
    assert [s.seek for s in runs[True][0]] == [0, 0, 0, 300, 300]
    _check(runs[True][0], runs[False][0], runs[True][1], [13, 8])


def test_shard_refuses_the_keyword(hf_tok):
    with pytest.raises(ValueError):
        BatchedInferencePipeline(_model(hf_tok)).transcribe(_audio(5), language="en", shard=True, token_logprobs=True)


def test_reference_of_the_beam_update_adds_up():
    """tests/token_logprob_refs.py on a toy language model, beam search chained to the end: for every finished
    hypothesis the float32 sum of its recorded log-probs in order, then its end value, IS its cum (bit for bit) — the
    candidates are built as cum + lp, so the bookkeeping only has to follow the right parents"""
    from decode_state_refs import FIN_CAP, chain_inputs, toy_candidates, toy_table
    from token_logprob_refs import beam_update_lp_ref, lp_state
    B, K, NT, P, budget, V, eot = 2, 3, 12, 2, 9, 11, 4
    logp = toy_table(5, V, n=B)
    R = B * K
    st = lp_state(B, K, NT, 0, P, None, None, np.zeros((R, P - 1), np.uint8), np.zeros(R, np.float32), -77, -1234.5)
    n_checked = 0
    for step in range(budget):
        cv, ct = toy_candidates(logp, st, B, K, step, st["done"])
        prev = np.where(step == 0, V, st["hist2"][step & 1, :, step - 1] if step else 0)
        cl = np.full_like(cv, -np.inf)
        for r in range(R):
            ok = np.isfinite(cv[r])
            cl[r, ok] = logp[r // K, V if step == 0 else int(prev[r])][ct[r, ok]]
        out = beam_update_lp_ref(st, cv, ct, cl, K=K, P=P, step=step, budget=budget, max_fin=K, lp_pow=0.0, eot=eot)
        if out["done"].all():
            break
        hist, kvidx, cum = chain_inputs(out, B, K, P, step + 1)
        live = np.repeat(np.asarray(out["done"]) == 0, K)
        lphist = np.where(live[:, None], out["lphist2"][(step + 1) & 1, :, :step + 1], 0).astype(np.float32)
        st = lp_state(B, K, NT, step + 1, P, hist, lphist, kvidx, cum, -77, -1234.5, fin_lp=out["fin_lp"],
                      done=out["done"], n_done=int(out["n_done"][0]), n_fin=out["n_fin"],
                      fin=(out["fin_tok"], out["fin_len"], out["fin_score"], out["fin_cum"]))
    assert out["done"].all()
    ends = set()
    for c in range(B):
        assert 0 < out["n_fin"][c] <= FIN_CAP
        for f in range(out["n_fin"][c]):
            acc = np.float32(0)
            for x in out["fin_lp"][c, f, :out["fin_len"][c, f]]:
                acc = np.float32(acc + x)
            acc = np.float32(acc + out["fin_lp"][c, f, NT])
            assert acc.view(np.uint32) == np.float32(out["fin_cum"][c, f]).view(np.uint32), (c, f)
            ends.add(bool(out["fin_lp"][c, f, NT] != 0))
            n_checked += 1
    assert n_checked >= 2 * K and ends == {True, False}      # hypotheses closed by <eot> and cut at the budget
