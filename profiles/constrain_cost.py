"""What generate(constraint=list) costs per decode step ("Constrained decoding"): one encoder output of 16 chunks
on the large-v3 geometry (synthetic weights, bench.py's audio, prompt and suppress list), beam 5 = 80 logits rows, then
generate() without a list, with a list of 16 phrases and with a full list (128 phrases = 4096 tokens).  Every phrase has
32 tokens — the longest a phrase may be — and the budget is 32 new tokens, so a constrained call decodes exactly 32 steps
(no phrase is complete before, <eot> is not allowed); the call without a list decodes the same 32 steps through
min_new_tokens = 32, which a constrained call may not set.  A call of 100 steps does not exist under a list: a phrase ends
after 32 tokens.  Two measurements:

  default     wall time of generate() with step graphs, the settings ALTERNATING inside one process (every round runs all
              of them once, in order): median per setting, the difference to "none" per step in us, and the spread
              (max - min) / median of the runs without a list;
  --family    time per launch of the PF_DEC_SAMPLE family (`dec_sample`: boost, constraint, rules kernel, beam update and
              step advance of one step; HIP-event timing through fw_prof_*), steps launched eagerly (FWAMD_NO_GRAPH=1):
              best of five per setting.

FWAMD_LIB=<the parent commit's libfwamd.so> runs the setting without a list on that library (it has no
fw_generate_constrain; the settings with a list are then left out): the same run on the parent's code.

usage: python profiles/constrain_cost.py [--family] [--model large-v3] [--rounds 7] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STEPS = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--family", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.family:
        os.environ["FWAMD_NO_GRAPH"] = "1"
    import bench
    from faster_whisper_amd import _lib, get_config
    cfg = get_config(args.model)
    bargs = argparse.Namespace(model=args.model, batch=args.batch, beam=5, workers=1, compute_type="float16",
                               merge_fill=None, merge_wait_ms=None)
    model, _ = bench.build_backend(bargs, cfg, 0, 1, 0)
    enc = model.encode_pcm(bench.synth_chunks(args.batch, 1000))
    prompt = list(cfg.sot_sequence) + [cfg.no_timestamps]
    sup = [cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, cfg.translate, cfg.transcribe]
    base = dict(beam_size=5, patience=1.0, length_penalty=1.0, max_length=len(prompt) + STEPS, return_scores=True,
                return_no_speech_prob=True, suppress_blank=True, suppress_tokens=sup)
    lists = {"none": None}
    if hasattr(_lib.load(), "fw_generate_constrain"):
        rng = np.random.default_rng(0)
        text = np.setdiff1d(np.arange(1000, 40000), np.asarray(sup + list(cfg.suppress_begin)))

        def phrases(count):
            return [[int(t) for t in rng.choice(text, size=STEPS)] for _ in range(count)]
        lists["16 x 32"] = model.constraint_list(phrases(16))
        lists["128 x 32"] = model.constraint_list(phrases(128))
    settings = list(lists)

    def call(name):
        kw = dict(min_new_tokens=STEPS) if lists[name] is None else dict(constraint=lists[name])
        t0 = time.perf_counter()
        res = model.generate(enc, [prompt] * args.batch, **base, **kw)
        dt = time.perf_counter() - t0
        assert all(len(r.sequences_ids[0]) == STEPS for r in res)
        return dt * 1e3

    for s in settings:        # warm-up: workspaces and one step graph per setting
        call(s)
        call(s)
    model.synchronize()
    rows = []
    head = f"{args.model}, {args.batch} chunks x beam 5 x {STEPS} steps; library {_lib.LIB_PATH}"
    if args.family:
        print(head + "; us per launch of the dec_sample family, eager steps, best of 5")
        best = {}
        for s in settings:
            for _ in range(5):
                model.profile(True)
                call(s)
                r = model.profile_report()
                model.profile(False)
                (key, v), = {k: v for k, v in r.items() if "sample" in k.lower()}.items()
                us = 1000.0 * v["ms"] / max(1, v["launches"])
                best[s] = min(best.get(s, us), us)
        print("| list | us per step (dec_sample) | added |")
        print("|---|---|---|")
        for s in settings:
            rows.append(dict(list=s, family_us=best[s], added_us=best[s] - best["none"]))
            print(f"| {s} | {best[s]:.1f} | {best[s] - best['none']:+.1f} |")
    else:
        times = {s: [] for s in settings}
        for _ in range(args.rounds):
            for s in settings:
                times[s].append(call(s))
        print(head + f"; {args.rounds} alternating rounds, ms per generate() call")
        print("| list | median ms | us / step | added us / step | spread of none |")
        print("|---|---|---|---|---|")
        t0 = np.asarray(times["none"])
        spread = float((t0.max() - t0.min()) / np.median(t0))
        for s in settings:
            med = float(np.median(times[s]))
            added = 1e3 * (med - float(np.median(t0))) / STEPS
            rows.append(dict(list=s, median_ms=med, us_per_step=1e3 * med / STEPS, added_us_per_step=added, none_spread=spread,
                             all_ms=[round(float(x), 3) for x in times[s]]))
            print(f"| {s} | {med:.2f} | {1e3 * med / STEPS:.1f} | {added:+.1f} | {100 * spread:.2f} % |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(model=args.model, batch=args.batch, steps=STEPS, family=args.family, library=_lib.LIB_PATH,
                           rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
