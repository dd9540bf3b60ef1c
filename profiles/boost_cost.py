"""What generate(boost=list) costs per call ("Phrase boosting"): one encoder output of 16 chunks on the large-v3
geometry (synthetic weights, bench.py's audio, prompt, suppress list and min_new_tokens = the new-token count, so that
every call decodes exactly that many steps), then generate() timed for beam 5 and greedy without a list, with a list of 16
phrases and with a full list (1024 phrases of 4 tokens).  The settings ALTERNATE inside one process — every round runs all
of them once, in order — and the table gives the median per setting, its ratio to the same mode without a list and the
spread (max - min) / median of the repeated runs without a list beside it.

FWAMD_LIB=<the parent commit's libfwamd.so> runs the settings without a list on that library (it has no fw_generate_boost;
the settings with a list are then left out): the same run without a list on the parent's code.

usage: python profiles/boost_cost.py [--model large-v3] [--new-tokens 100] [--rounds 7] [--out FILE.json]"""
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
    from faster_whisper_amd import _lib, get_config
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
    modes = {"beam5": dict(beam_size=5), "greedy": dict(beam_size=1)}
    lists = {"none": None}
    if hasattr(_lib.load(), "fw_generate_boost"):
        rng = np.random.default_rng(0)
        text = np.arange(1000, 40000)

        def phrases(count, length):
            return [[int(t) for t in rng.choice(text, size=length)] for _ in range(count)]
        lists["16 x 3"] = model.boost_list(phrases(16, 3), [2.0] * 16)
        lists["1024 x 4"] = model.boost_list(phrases(1024, 4), [2.0] * 1024)
    settings = [(m, name) for m in modes for name in lists]

    def call(mode, name):
        t0 = time.perf_counter()
        res = model.generate(enc, [prompt] * args.batch, **base, **modes[mode],
                             **(dict(boost=lists[name]) if lists[name] is not None else {}))
        dt = time.perf_counter() - t0
        assert all(len(r.sequences_ids[0]) == n for r in res)
        return dt * 1e3

    for s in settings:        # warm-up: workspaces and one step graph per setting
        call(*s)
        call(*s)
    model.synchronize()
    times = {s: [] for s in settings}
    for _ in range(args.rounds):
        for s in settings:
            times[s].append(call(*s))
    rows = []
    print(f"{args.model}, {args.batch} chunks x {n} new tokens, {args.rounds} alternating rounds; ms per generate() call; "
          f"library {_lib.LIB_PATH}")
    print("| mode | list | median ms | ms / step | vs none | spread of none |")
    print("|---|---|---|---|---|---|")
    for mode in modes:
        t0 = np.asarray(times[(mode, "none")])
        spread = float((t0.max() - t0.min()) / np.median(t0))
        for name in lists:
            t = np.asarray(times[(mode, name)])
            med = float(np.median(t))
            ratio = med / float(np.median(t0))
            rows.append(dict(mode=mode, list=name, median_ms=med, ms_per_step=med / n, ratio=ratio, none_spread=spread,
                             all_ms=[round(float(x), 3) for x in t]))
            print(f"| {mode} | {name} | {med:.2f} | {med / n:.3f} | {100 * (ratio - 1):+.2f} % | {100 * spread:.2f} % |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(model=args.model, batch=args.batch, new_tokens=n, rounds=args.rounds, library=_lib.LIB_PATH,
                           rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
