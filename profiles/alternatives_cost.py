"""What generate(return_alternatives=N) costs per call (profiles/NOTES.md, "alternatives"): one encoder output of 16 chunks on
the large-v3 geometry (synthetic weights, bench.py's audio, prompt, suppress list and min_new_tokens = the new-token
count, so that every call decodes exactly that many steps), then generate() timed for beam 5, greedy and sampling (5
hypotheses) with N in {0, 5, 8}.  The settings ALTERNATE inside one process — every round runs all nine once, in order —
and the table gives the median per setting, its ratio to the same mode's N = 0 and the spread (max - min) / median of the
repeated N = 0 runs beside it.

usage: python profiles/alternatives_cost.py [--model large-v3] [--new-tokens 100] [--rounds 7] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--new-tokens", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from faster_whisper_amd import get_config
    cfg = get_config(args.model)
    bargs = argparse.Namespace(model=args.model, batch=args.batch, beam=5, workers=1, compute_type="float16",
                               merge_fill=None, merge_wait_ms=None)
    model, _ = bench.build_backend(bargs, cfg, 0, 1, 0)
    enc = model.encode_pcm(bench.synth_chunks(args.batch, 1000))
    prompt = list(cfg.sot_sequence) + [cfg.no_timestamps]
    n = args.new_tokens
    sup = [cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, cfg.translate, cfg.transcribe]
    base = dict(patience=1.0, length_penalty=1.0, max_length=len(prompt) + n, return_scores=True,
                return_no_speech_prob=True, suppress_blank=True, suppress_tokens=sup, min_new_tokens=n)
    modes = {
        "beam5": dict(beam_size=5),
        "greedy": dict(beam_size=1),
        "sampling5": dict(beam_size=1, num_hypotheses=5, sampling_topk=0, sampling_temperature=0.8, seed=99),
    }
    settings = [(m, a) for m in modes for a in (0, 5, 8)]

    def call(mode, n_alt):
        t0 = time.perf_counter()
        res = model.generate(enc, [prompt] * args.batch, **base, **modes[mode],
                             **(dict(return_alternatives=n_alt) if n_alt else {}))
        dt = time.perf_counter() - t0
        assert all(len(r.sequences_ids[0]) == n for r in res)
        return dt * 1e3

    # warm-up: workspaces and one step graph per setting; the N = 0 settings first, so that what the others add to the
    # device memory in use is the alternatives' buffers (alt_tok / alt_lp, fin_path, the gather's output) alone
    import torch
    for s in sorted(settings, key=lambda s: s[1] > 0):
        if s == next(x for x in settings if x[1] > 0):
            free0 = torch.cuda.mem_get_info()[0]
        call(*s)
        call(*s)
    model.synchronize()
    print(f"device memory taken by the first runs with alternatives: {(free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20:.1f} MiB")
    times = {s: [] for s in settings}
    for _ in range(args.rounds):
        for s in settings:
            times[s].append(call(*s))
    rows = []
    print(f"{args.model}, {args.batch} chunks x {n} new tokens, {args.rounds} alternating rounds; ms per generate() call")
    print("| mode | N | median ms | ms / step | vs N = 0 | spread of N = 0 |")
    print("|---|---|---|---|---|---|")
    for mode in modes:
        t0 = np.asarray(times[(mode, 0)])
        spread = float((t0.max() - t0.min()) / np.median(t0))
        for n_alt in (0, 5, 8):
            t = np.asarray(times[(mode, n_alt)])
            med = float(np.median(t))
            ratio = med / float(np.median(t0))
            rows.append(dict(mode=mode, n_alt=n_alt, median_ms=med, ms_per_step=med / n, ratio=ratio, n0_spread=spread,
                             all_ms=[round(float(x), 3) for x in t]))
            print(f"| {mode} | {n_alt} | {med:.2f} | {med / n:.3f} | {100 * (ratio - 1):+.2f} % | {100 * spread:.2f} % |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(model=args.model, batch=args.batch, new_tokens=n, rounds=args.rounds, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
