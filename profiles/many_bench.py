"""Many short recordings: a loop of transcribe(), a thread pool of transcribe() calls, and ONE transcribe_many call.

Workload: N synthetic recordings of 8 - 28 s (two noise bursts with a short digital silence between and after them),
ndarrays in host memory; large-v3 geometry, synthetic weights, fp16, beam 5, `--workers` worker replicas as in bench.py;
the VAD runs on the device with the peaked Silero weights of tests/test_gpu_c5.py.  Three ways, alternating in one process:
    (a) loop        for audio in recordings: transcribe(audio)
    (b) pool        `--workers` host threads, each calling transcribe() on the next recording — the best a user can do
                    without transcribe_many; repeated `--pool-reps` times for its run-to-run spread
    (c) many        transcribe_many(recordings)
plus the VAD front alone: N per-recording device calls (SileroVADModel.__call__) against one batched call (forward_many).
Before any figure is printed, (c) is compared with (a) segment for segment (every field) and must be equal.
A fourth way, for the SEQUENTIAL path (`--sequential N`, longer recordings of `--seq-seconds` LO HI, no VAD):
    (d) seq_pool    `--workers` host threads, each calling WhisperModel.transcribe(condition_on_previous_text=True) on the
                    next recording: every later window's prompt carries its own amount of previous text
        seq_many    WhisperModel.transcribe_many(recordings, condition_on_previous_text=True), compared with seq_pool
                    recording for recording before its figure counts
    each with the decode group's counters over that way (decode runs, chunks, largest run): calls of different prompt lengths
    share decode runs, so both should show fewer, larger runs than a build in which they cannot.  `--sequential-only`
    skips (a) - (c) and the VAD front.  max_length stays 448 for every window (max_new_tokens would tie it to the prompt
    length, and calls that differ in max_length never share a run); nothing is suppressed and every recording has an
    initial prompt of its own length, so prompt lengths differ between recordings and from window to window.  (largest_run is the group's running maximum: the second way's figure is the maximum over both.)
Prints one JSON line (and writes it to --out).  Needs a GPU; there is no fallback.

    python profiles/many_bench.py --out profiles/many_bench.json
"""
import argparse
import dataclasses
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def recordings(n, seed):
    """n recordings of 8 - 28 s: burst, 0.6 s of silence, burst, 0.4 s of silence (one VAD chunk of two spans each)"""
    from test_gpu_c5 import recording
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        total = float(rng.uniform(8.0, 28.0))
        first = float(rng.uniform(0.3, 0.7)) * (total - 1.0)
        out.append(recording([(first, 0.6), (total - 1.0 - first, 0.4)], seed=seed + 2 * i))
    return out


def long_recordings(n, seed, lo, hi):
    """n recordings of lo - hi s: bursts of 9 - 24 s with half a second of digital silence after each"""
    from test_gpu_c5 import recording
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        total, spans = float(rng.uniform(lo, hi)), []
        while total > 0:
            sp = min(total, float(rng.uniform(9.0, 24.0)))
            spans.append((sp, 0.5))
            total -= sp + 0.5
        out.append(recording(spans, seed=seed + 50 * i))
    return out


def sequential_modes(args, backend, wm, cfg):
    """(d): thread pool of WhisperModel.transcribe against WhisperModel.transcribe_many, condition_on_previous_text=True"""
    recs = long_recordings(args.sequential, args.seed + 7, *args.seq_seconds)
    audio_s = sum(len(a) for a in recs) / 16000.0
    # nothing suppressed: a window's text ends where the (synthetic) model says <|endoftext|>, so the previous text differs
    # in length from window to window; and every recording starts from an initial prompt of its own length (0 - 120 tokens)
    kw = dict(language="en", beam_size=args.beam, temperature=0.0, condition_on_previous_text=True,
              without_timestamps=True, suppress_tokens=[])
    rng = np.random.default_rng(args.seed + 11)
    initial = [[int(t) for t in rng.integers(1000, 20000, size=int(n))] or None
               for n in rng.integers(0, 121, size=len(recs))]

    def seq_pool(k):
        def one(i):
            s, info = wm.transcribe(recs[i], initial_prompt=initial[i], **kw)
            return list(s), info
        with ThreadPoolExecutor(max_workers=args.workers) as ex:
            return list(ex.map(one, range(k)))

    def seq_many(k):
        return wm.transcribe_many(recs[:k], initial_prompt=initial[:k], **kw)

    ways = [seq_pool] + ([seq_many] if hasattr(wm, "transcribe_many") else [])
    for fn in ways:                              # warm-up: code objects, workspaces, thread replicas
        fn(min(len(recs), max(2, args.workers // 4)))
    out, results = {"recordings": len(recs), "audio_s": round(audio_s, 1)}, {}
    for fn in ways:
        backend.synchronize()
        st0 = backend.decode_stats()
        t = time.perf_counter()
        results[fn.__name__] = fn(len(recs))
        dt = time.perf_counter() - t
        st = backend.decode_stats()
        print(f"[many_bench] {fn.__name__}: {dt:.3f} s", file=sys.stderr, flush=True)
        out[fn.__name__] = {"wall_s": round(dt, 3), "rate": round(audio_s / dt, 1),
                            "decode_stats": {"runs": st["runs"] - st0["runs"], "calls": st["requests"] - st0["requests"],
                                             "chunks": st["chunks"] - st0["chunks"], "largest_run": st["max_run_chunks"]}}
    if "seq_many" in results:
        for r, ((gs, gi), (ws, wi)) in enumerate(zip(results["seq_many"], results["seq_pool"])):
            assert [dataclasses.asdict(s) for s in gs] == [dataclasses.asdict(s) for s in ws], f"recording {r}: segments differ"
            assert dataclasses.asdict(gi) == dataclasses.asdict(wi), f"recording {r}: info differs"
        out["seq_many_equals_seq_pool"] = True
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", "--recordings", type=int, default=256)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--workers", type=int, default=32)
    ap.add_argument("--new-tokens", type=int, default=100)
    ap.add_argument("--pool-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4000)
    ap.add_argument("--sequential", type=int, default=0, help="(d): recordings for the sequential ways (0: skip them)")
    ap.add_argument("--seq-seconds", type=float, nargs=2, default=(60.0, 120.0), metavar=("LO", "HI"))
    ap.add_argument("--sequential-only", action="store_true", help="only (d): no loop / pool / many, no VAD front")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import bench
    from faster_whisper_amd import Whisper, _lib, get_config, synthetic_weights
    from faster_whisper_amd import vad as fvad
    from faster_whisper_amd.transcribe import BatchedInferencePipeline
    from test_gpu_c5 import peaked_vad_weights
    if _lib.load().fw_device_count() <= 0:
        raise SystemExit("many_bench.py: no HIP device (this measurement has no CPU form)")

    cfg = get_config(args.model)
    t0 = time.perf_counter()
    backend = Whisper(f"synthetic:{args.model}", files={"config": cfg, "weights": synthetic_weights(cfg, seed=1234)},
                      device="cuda", compute_type="float16", max_batch_size=args.batch, max_beam_size=args.beam,
                      inter_threads=args.workers)
    load_s = time.perf_counter() - t0
    print(f"[many_bench] model loaded in {load_s:.1f} s", file=sys.stderr, flush=True)
    wm = bench.host_model(backend, cfg)
    if args.sequential_only:
        out = {"what": "long recordings, sequential path: thread pool of WhisperModel.transcribe / WhisperModel.transcribe_many",
               "unit": "audio-seconds per wall-second", "model": args.model, "compute_type": "float16", "beam": args.beam,
               "workers": args.workers, "model_load_s": round(load_s, 1),
               "sequential": sequential_modes(args, backend, wm, cfg)}
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return out
    dev = fvad.SileroVADModel(weights=peaked_vad_weights(), device="cuda")
    fvad._VAD_MODEL = dev                       # what transcribe(vad_filter=True) runs per call
    recs = recordings(args.recordings, args.seed)
    audio_s = sum(len(a) for a in recs) / 16000.0
    # decode length fixed as in bench.py: <|endoftext|> suppressed up to max_new_tokens
    kw = dict(language="en", beam_size=args.beam, batch_size=args.batch, vad_filter=True, max_new_tokens=args.new_tokens,
              suppress_tokens=[cfg.eot], without_timestamps=True)

    def loop():
        return [(list(s), i) for s, i in (BatchedInferencePipeline(wm).transcribe(a, **kw) for a in recs)]

    def pool():
        def one(a):
            s, i = BatchedInferencePipeline(wm).transcribe(a, **kw)
            return list(s), i
        with ThreadPoolExecutor(max_workers=args.workers) as ex:
            return list(ex.map(one, recs))

    def many():
        return BatchedInferencePipeline(wm).transcribe_many(recs, vad_model=dev, **kw)

    def timed(fn):
        backend.synchronize()
        t = time.perf_counter()
        out = fn()                               # (every way ends with its last Segment on the host)
        dt = time.perf_counter() - t
        print(f"[many_bench] {fn.__name__}: {dt:.3f} s", file=sys.stderr, flush=True)
        return dt, out

    # warm-up: every way once on a slice that fills the workers (code objects, workspaces, thread replicas)
    warm = recs[:min(len(recs), 2 * args.workers)]
    full, recs = recs, warm
    for fn in (loop, pool, many):
        fn()
    recs = full

    # (a) (b) (c) (b) (b): the ways alternate, (b) is repeated for its spread
    t_loop, r_loop = timed(loop)
    t_pool = [timed(pool)[0]]
    t_many, r_many = timed(many)
    t_pool += [timed(pool)[0] for _ in range(args.pool_reps - 1)]
    t_many2, _ = timed(many)

    # (c) == (a), segment for segment, before any figure
    assert len(r_many) == len(r_loop) == len(recs)
    n_seg = 0
    for r, ((gs, gi), (ws, wi)) in enumerate(zip(r_many, r_loop)):
        assert [dataclasses.asdict(s) for s in gs] == [dataclasses.asdict(s) for s in ws], f"recording {r}: segments differ"
        assert dataclasses.asdict(gi) == dataclasses.asdict(wi), f"recording {r}: info differs"
        n_seg += len(gs)
    assert n_seg >= len(recs), "every recording has speech"

    # the VAD front alone
    padded = [np.pad(a, (0, 512 - len(a) % 512)) for a in recs]

    def vad_single():
        return [dev(a) for a in padded]

    def vad_batch():
        return dev.forward_many(padded)

    vad_single(), vad_batch()
    vs = [timed(vad_single) for _ in range(3)]
    vb = [timed(vad_batch) for _ in range(3)]
    assert all(np.array_equal(x, y) for x, y in zip(vs[0][1], vb[0][1])), "batched VAD differs from the single calls"

    # where (c)'s time goes: the same call fed the probabilities (no VAD inside)
    t_many_given, _ = timed(lambda: BatchedInferencePipeline(wm).transcribe_many(recs, vad_speech_probs=vb[0][1], **kw))

    rate = lambda t: round(audio_s / t, 1)      # noqa: E731
    pool_rates = [rate(t) for t in t_pool]
    spread = max(pool_rates) - min(pool_rates)
    out = {
        "what": "many short recordings: loop of transcribe() / thread pool of transcribe() / transcribe_many",
        "unit": "audio-seconds per wall-second", "model": args.model, "compute_type": "float16", "beam": args.beam,
        "batch": args.batch, "workers": args.workers, "new_tokens": args.new_tokens, "recordings": len(recs),
        "audio_s": round(audio_s, 1), "segments": n_seg, "model_load_s": round(load_s, 1),
        "loop": {"wall_s": round(t_loop, 3), "rate": rate(t_loop)},
        "pool": {"wall_s": [round(t, 3) for t in t_pool], "rate": pool_rates, "spread": round(spread, 1)},
        "many": {"wall_s": [round(t_many, 3), round(t_many2, 3)], "rate": [rate(t_many), rate(t_many2)]},
        "many_given_vad_probs": {"wall_s": round(t_many_given, 3), "rate": rate(t_many_given)},
        "many_equals_loop": True,
        "many_above_pool_by_more_than_its_spread": bool(min(rate(t_many), rate(t_many2)) - max(pool_rates) > spread),
        "vad_front_ms": {"per_recording_calls": [round(1e3 * t, 2) for t, _ in vs],
                         "one_batched_call": [round(1e3 * t, 2) for t, _ in vb],
                         "windows": int(sum(len(a) for a in padded) // 512), "equal": True},
        "decode_stats": backend.decode_stats(),
    }
    if args.sequential > 0:
        out["sequential"] = sequential_modes(args, backend, wm, cfg)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
