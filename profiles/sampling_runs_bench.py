"""What do sampled fallback attempts cost, alone and sharing a decode run — on this build and on another one (the parent
commit's), alternating on one machine in one visit?

Geometry: large-v3, synthetic weights, 8 worker replicas (+ one for the blocker), one decode lane.  Per worker one
fallback-shaped generate() call: 1 chunk, beam_size=1, sampling_topk=0, num_hypotheses = best_of = 5, max_length = prompt +
100, min_new_tokens = 100 (every hypothesis runs its whole budget), a seed and a temperature of its own.

Per build, in a fresh process per repeat (the library is chosen at import: FWAMD_LIB):
  (a) the 8 calls one after another (three times, new seeds every time): wall time of the 8;
  (b) the 8 calls from 8 threads, queued behind a blocker run that holds the lane: wall time from the blocker's end to the
      last result, decode runs it took, the largest run;
  (c) step graphs captured during the first (a) (a build without the counter reports null: by its code — the graph key held
      seed and temperature — it captured one per call).

    python profiles/sampling_runs_bench.py --other /path/to/parent/libfwamd.so [--repeats 3]

writes profiles/sampling_runs_bench.json (and prints it).  Not part of bench.py, not run by the suite."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKERS = 8
BEST_OF = 5
NEW_TOKENS = 100


def child(model_name):
    from faster_whisper_amd import Whisper, get_config
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import bench_audio
    cfg = get_config(model_name)
    model = Whisper(f"synthetic:{model_name}", device="cuda", max_batch_size=1, max_beam_size=5, inter_threads=WORKERS + 1)
    model.set_decode_lanes(1)
    prompt = list(cfg.sot_sequence) + [cfg.no_timestamps]
    sup = [cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, cfg.translate, cfg.transcribe]
    base = dict(beam_size=1, num_hypotheses=BEST_OF, sampling_topk=0, max_length=len(prompt) + NEW_TOKENS,
                min_new_tokens=NEW_TOKENS, suppress_tokens=sup, return_scores=True, return_no_speech_prob=True)
    seeds = iter(range(1000, 100000))

    def kw(i):
        return dict(base, sampling_temperature=0.2 + 0.1 * i, seed=next(seeds))

    # one encoder output per worker replica (a host thread keeps the replica it was first given)
    encs = [None] * WORKERS
    go, results = threading.Event(), [None] * WORKERS
    encoded = threading.Barrier(WORKERS + 1)
    t_done = [0.0] * WORKERS

    def work(i):
        encs[i] = model.encode_pcm([bench_audio(480000, seed=300 + i)])
        encoded.wait()
        go.wait()
        results[i] = model.generate(encs[i], [prompt], **kw(i))
        t_done[i] = time.perf_counter()

    ts = [threading.Thread(target=work, args=(i,)) for i in range(WORKERS)]
    for t in ts:
        t.start()
    encoded.wait()
    blocker_enc = model.encode_pcm([bench_audio(480000, seed=299)])
    model.generate(encs[0], [prompt], **kw(0))                     # warm: workspace, pool, the first graph
    model.synchronize()
    rec = {"a_ms": [], "a_captures": None}
    for rep in range(3):
        c0 = model.graph_captures() if hasattr(model, "graph_captures") else -1
        t0 = time.perf_counter()
        for i in range(WORKERS):
            out = model.generate(encs[i], [prompt], **kw(i))
            assert all(len(ids) == NEW_TOKENS for ids in out[0].sequences_ids)
        rec["a_ms"].append(round(1e3 * (time.perf_counter() - t0), 2))
        if rep == 0 and c0 >= 0:
            rec["a_captures"] = model.graph_captures() - c0
    # (b): behind a blocker (beam 2: no sampling call shares its run)
    st0 = model.decode_stats()
    t_blocker = [0.0]

    def block():
        model.generate(blocker_enc, [prompt], beam_size=2, max_length=len(prompt) + 60, min_new_tokens=60, suppress_tokens=sup)
        t_blocker[0] = time.perf_counter()

    tb = threading.Thread(target=block)
    tb.start()
    while model.decode_stats()["runs"] == st0["runs"]:
        pass
    go.set()
    for t in ts + [tb]:
        t.join()
    st = model.decode_stats()
    assert all(len(ids) == NEW_TOKENS for r in results for ids in r[0].sequences_ids)
    rec["b_ms"] = round(1e3 * (max(t_done) - t_blocker[0]), 2)
    rec["b_runs"] = int(st["runs"] - st0["runs"] - 1)
    rec["b_max_run_chunks"] = int(st["max_run_chunks"])
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="libfwamd.so of the build to compare with (the parent commit's)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_runs_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.model)
    builds = [("parent", a.other)] if a.other else []
    builds.append(("this", None))
    runs = []
    for rep in range(a.repeats):
        for name, lib in builds:                      # alternating
            env = dict(os.environ)
            env.pop("FWAMD_LIB", None)
            if lib:
                env["FWAMD_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--model", a.model], env=env,
                               capture_output=True, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{name} build, repeat {rep}: exit status {p.returncode}")
            rec = dict(build=name, repeat=rep, **json.loads(line[0][7:]))
            print(json.dumps(rec), flush=True)
            runs.append(rec)
    summary = {}
    for name, _ in builds:
        mine = [r for r in runs if r["build"] == name]
        a_all = [x for r in mine for x in r["a_ms"]]
        summary[name] = {"a_ms_median": statistics.median(a_all), "a_ms_min": min(a_all), "a_ms_max": max(a_all),
                         "b_ms_median": statistics.median(r["b_ms"] for r in mine),
                         "b_ms_all": [r["b_ms"] for r in mine], "b_runs": [r["b_runs"] for r in mine],
                         "a_captures": [r["a_captures"] for r in mine]}
    if "parent" in summary:
        s, p = summary["this"], summary["parent"]
        summary["a_this_over_parent"] = round(s["a_ms_median"] / p["a_ms_median"], 4)
        summary["parent_a_spread_rel"] = round((p["a_ms_max"] - p["a_ms_min"]) / p["a_ms_median"], 4)
        summary["b_this_over_parent"] = round(s["b_ms_median"] / p["b_ms_median"], 4)
        summary["b_this_over_a_this"] = round(s["b_ms_median"] / s["a_ms_median"], 4)
    doc = {"model": a.model, "workers": WORKERS, "best_of": BEST_OF, "new_tokens": NEW_TOKENS, "lanes": 1,
           "runs": runs, "summary": summary}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
