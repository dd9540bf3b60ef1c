"""What one launch of dec_automaton_kernel costs ("Automaton-constrained decoding"), through the timing of
fw_test_automaton_rows: the step form at large-v3's vocabulary (51 866 ids) and text context, 80 rows (16 chunks x beam 5)
and 640 rows (a full lane of 128 chunks), for

  list      the phrase-list automaton: 127 phrases x 32 tokens (16 140 table words), and
  limits    an automaton at both limits (4096 states, 8192 edges),

at text histories of m ids, each with the table walked where it lies (L2) and staged in LDS first.  The kernel only sees
the vocabulary size, the rows and the text context, so the micro model serves as the device handle.

usage: python profiles/automaton_cost.py [--iters 2000] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, EOT, TSB = 51866, 50257, 50365


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from faster_whisper_amd import Whisper, _lib, get_config, synthetic_weights
    from faster_whisper_amd.grammar import Grammar
    cfg = get_config("micro")
    model = Whisper("synthetic:automaton-cost", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    handle, lib = model._replicas[0].handle, _lib.load()
    rng = np.random.default_rng(0)
    phrases = [[int(t) for t in rng.integers(1000, 40000, size=32)] for _ in range(127)]
    S = 4096
    limits = ([2 * s for s in range(S + 1)], [t for s in range(S) for t in (s % 40, 40 + s % 5)],
              [t for s in range(S) for t in ((s + 1) % S, (7 * s + 3) % S)], [int(s % 3 == 0) for s in range(S)])

    def limits_walk(n):
        s, out = 0, []
        for pick in rng.integers(0, 2, size=n):
            out.append(limits[1][2 * s + pick])
            s = limits[2][2 * s + pick]
        return out
    settings = {"list": (Grammar.phrases(phrases).csr(), lambda n: phrases[int(rng.integers(0, 127))][:n], (0, 4, 16, 31)),
                "limits": (limits, limits_walk, (0, 4, 16, 64, 447))}
    rows_out = []
    print(f"us per launch of dec_automaton_kernel<false>, V = {V}, mean of {args.iters} launches after 3")
    print("| automaton | table words | rows | m | L2 walk | LDS staged |")
    print("|---|---|---|---|---|---|")
    for name, (csr, walk, lengths) in settings.items():
        arrays = [np.ascontiguousarray(a, dtype=np.int32) for a in csr]
        h = C.c_void_p()
        _lib.check(lib.fw_automaton_create(V, len(csr[3]), *(_lib.as_i32p(a) for a in arrays), C.byref(h)))
        words = C.c_int32()
        _lib.check(lib.fw_test_automaton_table(h, None, 0, C.byref(words)))
        for rows in (80, 640):
            lg = rng.standard_normal((rows, V)).astype(np.float32)
            for m in lengths:
                hist = np.ascontiguousarray([walk(m) for _ in range(rows)], dtype=np.int32).reshape(rows, m)
                offs = np.arange(rows + 1, dtype=np.int32) * m
                flat = hist.reshape(-1) if m else np.zeros(1, dtype=np.int32)
                us = {}
                for staging in (1, 2):
                    out, t = lg.copy(), C.c_float()
                    _lib.check(lib.fw_test_automaton_rows(handle, _lib.ptr(out), rows, V, EOT, TSB, 0, _lib.ptr(flat),
                                                          _lib.ptr(offs), 5, None, 0, h, staging, args.iters, C.byref(t)))
                    us[staging] = t.value
                rows_out.append(dict(automaton=name, table_words=words.value, rows=rows, m=m, l2_us=us[1], lds_us=us[2]))
                print(f"| {name} | {words.value} | {rows} | {m} | {us[1]:.1f} | {us[2]:.1f} |", flush=True)
        lib.fw_automaton_free(h)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(V=V, iters=args.iters, rows=rows_out), f, indent=1)


if __name__ == "__main__":
    main()
