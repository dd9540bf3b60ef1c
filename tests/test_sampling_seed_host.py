"""transcribe(sampling_seed=) / transcribe_many(sampling_seed=) on the host: which `seed` keyword every generate() call of the
temperature fallback carries.  Driven by the scripted backend of the host goldens (oracle/scripted_backend.py), whose
generate() is wrapped here to record the keyword; the backend itself ignores it.  The ladder is (0, 0.4, 0.8) with
log_prob_threshold=0.0, which no scripted decode passes (their average log-probs are negative): every window climbs the
whole ladder unless it looks like silence.  No GPU."""
import threading

import numpy as np
import pytest

from faster_whisper_amd import get_config
from faster_whisper_amd.backend import attempt_seed, recording_seed
from oracle import host_scenarios as hs
from oracle import micro_tokenizer
from test_host_golden import make_model

# (seed, seconds, silences): one window, three windows, two windows
SPECS = [(31, 14.0, ()), (32, 70.0, ((21.0, 24.0),)), (33, 45.0, ())]
LADDER = dict(temperature=[0.0, 0.4, 0.8], log_prob_threshold=0.0, language="en", condition_on_previous_text=True)
MISSING = "no seed keyword"


@pytest.fixture(scope="module")
def hf_tok():
    return micro_tokenizer.build()


@pytest.fixture(scope="module")
def audios():
    return [hs.synth_audio(*s) for s in SPECS]


def _model(hf_tok, workers):
    """a scripted model whose generate() calls are recorded as (window fingerprint, temperature, seed keyword)"""
    model = make_model(get_config("micro"), hf_tok)
    model.model.inter_threads = workers
    lock, encode, generate = threading.Lock(), model.model.encode, model.model.generate
    seen = []

    def locked_encode(*a, **kw):      # (the scripted backend keeps the level of its last encode between two statements)
        with lock:
            return encode(*a, **kw)

    def recording_generate(enc, prompts, **kw):
        with lock:
            seen.append((tuple(enc.fp), float(kw.get("sampling_temperature", 0.0)) if kw.get("sampling_topk", 1) == 0 else 0.0,
                         kw.get("seed", MISSING)))
            return generate(enc, prompts, **kw)

    model.model.encode = locked_encode
    model.model.generate = recording_generate
    return model, seen


def _run(hf_tok, audio, **kw):
    model, seen = _model(hf_tok, 1)
    segs, _ = model.transcribe(audio, **LADDER, **kw)
    return list(segs), seen


def test_no_seed_keyword_without_sampling_seed(hf_tok, audios):
    _, seen = _run(hf_tok, audios[1])
    assert any(t > 0 for _, t, _ in seen)                       # the fallback did sample
    assert all(s == MISSING for _, _, s in seen)


def test_seeds_are_a_function_of_seed_window_and_rung(hf_tok, audios):
    segs_a, a = _run(hf_tok, audios[1], sampling_seed=9)
    segs_b, b = _run(hf_tok, audios[1], sampling_seed=9)
    assert a == b and segs_a == segs_b                          # two runs: identical seeds
    assert all((s == MISSING) == (t == 0) for _, t, s in a)     # only on the sampled attempts
    sampled = [(fp, t, s) for fp, t, s in a if t > 0]
    windows = sorted({fp for fp, _, _ in sampled})
    assert len(windows) >= 2                                    # several windows climbed the ladder
    assert len({s for _, _, s in sampled}) == len(sampled)      # every window and every rung has a seed of its own
    for fp in windows:
        rungs = {t: s for f, t, s in sampled if f == fp}
        assert 0.4 in rungs and (0.8 not in rungs or rungs[0.8] != rungs[0.4])
    assert any(0.8 in {t for f, t, _ in sampled if f == fp} for fp in windows)
    # the first window starts at frame 0: its seeds are attempt_seed(9, 0, rung) with the rung's index in the ladder
    first = a[0][0]
    assert [s for fp, t, s in a if fp == first and t > 0][:1] == [attempt_seed(9, 0, 1)]
    # another base seed: other seeds
    _, c = _run(hf_tok, audios[1], sampling_seed=10)
    assert not {s for _, t, s in c if t > 0} & {s for _, _, s in sampled}


def test_attempt_and_recording_seed_are_64_bit_mixes():
    vals = [attempt_seed(b, s, t) for b in (0, 1, 5) for s in (0, 3000, 6000) for t in (0, 1, 2)]
    vals += [recording_seed(b, i) for b in (0, 1, 5) for i in range(4)]
    assert len(set(vals)) == len(vals) and all(0 <= v < 2 ** 64 for v in vals)
    assert attempt_seed(5, 3000, 1) == attempt_seed(5, 3000, 1) and attempt_seed(2 ** 64 + 5, 0, 0) == attempt_seed(5, 0, 0)


@pytest.mark.parametrize("workers", [1, 3])
def test_transcribe_many_passes_each_recording_its_own_seeds(hf_tok, audios, workers):
    want_calls, want_segs = [], []
    for i, audio in enumerate(audios):
        segs, seen = _run(hf_tok, audio, sampling_seed=recording_seed(5, i))
        want_calls += seen
        want_segs.append(segs)
    assert any(t > 0 for _, t, _ in want_calls)
    model, seen = _model(hf_tok, workers)
    got = model.transcribe_many(audios, sampling_seed=5, **LADDER)
    assert sorted(seen, key=repr) == sorted(want_calls, key=repr)   # window by window (fingerprint), rung by rung
    assert [s for s, _ in got] == want_segs
    # one seed per recording, given explicitly
    model, seen = _model(hf_tok, workers)
    model.transcribe_many(audios, sampling_seed=[recording_seed(5, i) for i in range(3)], **LADDER)
    assert sorted(seen, key=repr) == sorted(want_calls, key=repr)
    # no seed: no keyword
    model, seen = _model(hf_tok, workers)
    model.transcribe_many(audios, **LADDER)
    assert all(s == MISSING for _, _, s in seen)


def test_a_seed_sequence_of_the_wrong_length_is_refused(hf_tok, audios):
    model, _ = _model(hf_tok, 2)
    with pytest.raises(ValueError, match="sampling_seed has 2 entries for 3"):
        model.transcribe_many(audios, sampling_seed=[1, 2], **LADDER)
