"""Truncated sampling without a GPU: the reference helper of the GPU tests (tests/sampling_trunc_refs.py) against a brute-force
sort on tiny vocabularies, and the Python fronts (transcribe / transcribe_many / BatchedInferencePipeline.transcribe) with a
scripted backend: at the defaults no new keyword reaches generate, with limits they reach exactly the temperature > 0 rungs
of the fallback ladder, and bad values raise before anything is decoded."""
import math

import numpy as np
import pytest

import sampling_trunc_refs as st
from faster_whisper_amd import get_config
from faster_whisper_amd.transcribe import BatchedInferencePipeline
from oracle import micro_tokenizer
from oracle.scripted_backend import ScriptedBackend
from test_host_golden import make_model

_UNSET = object()


# ---- the reference against brute force ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_reference_set_equals_brute_force(seed):
    """vocabularies of 1 .. 40 ids on a grid of 8 levels (ties everywhere), some ids masked, every k and a sweep of p; cuts that
    fall within 1e-9 of a cumulative mass are left out (float64 against Python floats)"""
    rng = np.random.default_rng(seed)
    n = 0
    for V in (1, 2, 3, 7, 40):
        for _ in range(8):
            lp = (-rng.integers(0, 8, V) / 2.0).astype(np.float32)
            lp[rng.random(V) < 0.25] = -np.inf
            for T in (0.5, 1.0, 2.0):
                for k in (0, 1, 2, 3, V - 1, V, V + 1, 100000):
                    if k < 0:
                        continue
                    for p in (0.05, 0.3, 0.5, 0.77, 0.99, 1.0):
                        t = st.trunc_set(lp, k, p, 1.0 / T)
                        if t["margin"] < 1e-9:
                            continue
                        assert t["S"].tolist() == st.brute_force_set(lp, k, p, 1.0 / T), (lp, k, p, T)
                        assert t["S"].tolist() == t["S_k"][:len(t["S"])].tolist() == t["order"][:len(t["S"])].tolist()
                        n += 1
    assert n > 1000


def test_reference_order_ties_and_edges():
    lp = np.asarray([-1.0, -0.5, -np.inf, -0.5, -1.0, -0.5], np.float32)
    assert st.order_of(lp).tolist() == [1, 3, 5, 0, 4]                     # log-prob descending, id ascending
    assert st.trunc_set(lp, 2, 1.0, 1.0)["S"].tolist() == [1, 3]           # a tie at the cut goes to the lower id
    assert st.trunc_set(lp, 0, 1.0, 1.0)["S"].tolist() == [1, 3, 5, 0, 4]
    assert st.trunc_set(lp, 9, 1.0, 1.0)["S"].tolist() == [1, 3, 5, 0, 4]
    assert st.trunc_set(lp, 0, 1e-6, 1.0)["S"].tolist() == [1]             # the first id is always in
    w = np.exp(np.asarray([0, 0, 0, -0.5, -0.5]))
    for j in range(5):                                                     # p at the middle of id j's mass keeps j + 1 ids
        p = (w[:j].sum() + 0.5 * w[j]) / w.sum()
        assert len(st.trunc_set(lp, 0, p, 1.0)["S"]) == j + 1
    # temperature comes before the nucleus: the same p keeps fewer ids when the distribution is sharpened
    sizes = [len(st.trunc_set(lp, 0, 0.7, 1.0 / T)["S"]) for T in (0.25, 1.0, 4.0)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    # Z is the top-k mass: with k = 2 half of it is one id, without k half of everything is two
    assert len(st.trunc_set(lp, 2, 0.45, 1.0)["S"]) == 1 and len(st.trunc_set(lp, 0, 0.45, 1.0)["S"]) == 2
    dead = np.full(4, -np.inf, np.float32)
    assert st.trunc_set(dead, 3, 0.5, 1.0)["S"].size == 0 and st.draw(dead, [], 1.0, np.zeros(4))[0] == 0
    # the draw: arg-max inside S only, the lowest id on a tie; the noise of an id does not depend on S
    noise = np.asarray([5.0, 0.0, 0.0, 0.0, 9.0, 0.0], np.float32)
    assert st.draw(lp, [1, 3, 5, 0, 4], 1.0, noise)[0] == 4 and st.draw(lp, [1, 3], 1.0, noise)[0] == 1
    assert st.draw(lp, [1, 3, 5, 0], 1.0, noise) == (0, 4.5)


# ---- the Python fronts --------------------------------------------------------------------------------------------------
class TruncBackend(ScriptedBackend):
    """the scripted backend with generate's top_k / top_p — strict: it records whether each keyword was passed at all"""

    def __init__(self, cfg, hf_tok):
        super().__init__(cfg, hf_tok)
        self.seen = []             # per generate call: (sampling_temperature or None for a beam call, top_k, top_p)

    def generate(self, enc, prompts, *, top_k=_UNSET, top_p=_UNSET, **kw):
        sampled = kw.get("sampling_topk", 1) == 0
        self.seen.append((kw.get("sampling_temperature") if sampled else None, top_k, top_p))
        return super().generate(enc, prompts, **kw)


@pytest.fixture(scope="module")
def hf_tok():
    return micro_tokenizer.build()


def _model(hf_tok):
    m = make_model(get_config("micro"), hf_tok)
    m.model = TruncBackend(get_config("micro"), hf_tok)
    return m


def _audio(seconds, seed=3):
    rng = np.random.default_rng(seed)
    return (0.1 * rng.standard_normal(int(seconds * 16000))).astype(np.float32)


# thresholds that every attempt fails: every rung of every window is decoded
LADDER = dict(language="en", temperature=(0.0, 0.4, 0.8), compression_ratio_threshold=0.0, no_speech_threshold=None,
              condition_on_previous_text=False)
CLIPS = [{"start": 0.0, "end": 10.0}]


def test_at_the_defaults_no_keyword_reaches_generate(hf_tok):
    runs = []
    m = _model(hf_tok)
    list(m.transcribe(_audio(8), **LADDER)[0])
    assert [t for t, _, _ in m.model.seen] == [None, 0.4, 0.8]
    runs.append(m)
    m = _model(hf_tok)
    list(m.transcribe(_audio(8), sampling_top_k=0, sampling_top_p=1.0, **LADDER)[0])
    runs.append(m)
    m = _model(hf_tok)
    m.transcribe_many([_audio(4), _audio(5, 4)], **LADDER)
    runs.append(m)
    m = _model(hf_tok)
    list(BatchedInferencePipeline(m).transcribe(_audio(12), language="en", clip_timestamps=CLIPS)[0])
    runs.append(m)
    m = _model(hf_tok)
    BatchedInferencePipeline(m).transcribe_many([_audio(12)], language="en", clip_timestamps=CLIPS)
    runs.append(m)
    for m in runs:
        assert m.model.seen and all(k is _UNSET and p is _UNSET for _, k, p in m.model.seen)


def test_limits_reach_exactly_the_sampled_rungs(hf_tok):
    m = _model(hf_tok)
    list(m.transcribe(_audio(8), sampling_top_k=40, sampling_top_p=0.9, **LADDER)[0])
    assert m.model.seen == [(None, _UNSET, _UNSET), (0.4, 40, 0.9), (0.8, 40, 0.9)]
    m = _model(hf_tok)                                           # one limit alone: only that keyword
    list(m.transcribe(_audio(8), sampling_top_p=0.5, **LADDER)[0])
    assert m.model.seen == [(None, _UNSET, _UNSET), (0.4, _UNSET, 0.5), (0.8, _UNSET, 0.5)]
    m = _model(hf_tok)
    list(m.transcribe(_audio(8), sampling_top_k=3, **LADDER)[0])
    assert m.model.seen == [(None, _UNSET, _UNSET), (0.4, 3, _UNSET), (0.8, 3, _UNSET)]
    m = _model(hf_tok)                                           # every recording of transcribe_many gets them
    m.transcribe_many([_audio(4), _audio(5, 4)], sampling_top_k=7, **LADDER)
    assert sorted(m.model.seen, key=str) == sorted([(None, _UNSET, _UNSET), (0.4, 7, _UNSET), (0.8, 7, _UNSET)] * 2, key=str)
    # the batched path never samples: the limits are accepted and limit nothing
    m = _model(hf_tok)
    list(BatchedInferencePipeline(m).transcribe(_audio(12), language="en", clip_timestamps=CLIPS, sampling_top_k=5,
                                                sampling_top_p=0.9)[0])
    assert m.model.seen and all(k is _UNSET and p is _UNSET for _, k, p in m.model.seen)


def test_the_limits_do_not_change_what_else_is_passed(hf_tok):
    a, b = _model(hf_tok), _model(hf_tok)
    list(a.transcribe(_audio(8), **LADDER)[0])
    list(b.transcribe(_audio(8), sampling_top_k=40, sampling_top_p=0.9, **LADDER)[0])
    assert a.model.calls == b.model.calls


@pytest.mark.parametrize("bad", [dict(sampling_top_k=-1), dict(sampling_top_k=2.5), dict(sampling_top_k=True),
                                 dict(sampling_top_p=0.0), dict(sampling_top_p=1.5), dict(sampling_top_p=math.nan),
                                 dict(sampling_top_p=-0.1), dict(sampling_top_p="0.9")])
def test_bad_values_raise_before_any_decode(hf_tok, bad):
    m = _model(hf_tok)
    with pytest.raises(ValueError):
        m.transcribe(_audio(4), language="en", **bad)
    with pytest.raises(ValueError):
        m.transcribe_many([_audio(4)], language="en", **bad)
    with pytest.raises(ValueError):
        BatchedInferencePipeline(m).transcribe(_audio(4), language="en", clip_timestamps=CLIPS, **bad)
    with pytest.raises(ValueError):
        BatchedInferencePipeline(m).transcribe_many([_audio(4)], language="en", clip_timestamps=CLIPS, **bad)
    assert m.model.seen == []
