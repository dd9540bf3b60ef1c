"""What one launch of dec_boost_trie_kernel costs, beside dec_boost_kernel where that takes the list ("Phrase
boosting"), through the timing of fw_test_boost_cost: the step form at large-v3's vocabulary (51 866 ids), 80 rows (16 chunks
x beam 5) and 640 rows (a full lane of 128 chunks), histories of 0 and 31 ids, for
  - 16 phrases of 3 ids,
  - fw_boost_create's full list, 1 024 phrases of 4 ids,
  - a list at fw_boost_create_large's limits, 65 536 phrases of 8 ids with random first ids (some 32 000 distinct ones),
  - the same size with first ids from every 2nd and every 4th text id (some 18 800 and 9 700 distinct ones) and with 64
    distinct first ids: the root's fan-out apart, the same list.
Every history of 31 ids ends in all but the last id of a phrase, so one walk goes to the phrase's full depth.  The kernels
only see the vocabulary size, the rows and the text context, so the micro model serves as the device handle.

usage: python profiles/boost_trie_cost.py [--iters 2000] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V = 51866


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from faster_whisper_amd import Whisper, _lib, get_config, synthetic_weights
    cfg = get_config("micro")
    model = Whisper("synthetic:boost-trie-cost", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    handle, lib = model._replicas[0].handle, _lib.load()
    rng = np.random.default_rng(0)
    text = np.arange(1000, 40000)

    def phrases(count, length, first=text):
        p = rng.choice(text, size=(count, length)).astype(np.int32)
        p[:, 0] = rng.choice(first, size=count)
        return p

    lists = {"16 x 3": phrases(16, 3), "1024 x 4": phrases(1024, 4), "65536 x 8": phrases(65536, 8),
             "65536 x 8, every 2nd first id": phrases(65536, 8, text[::2]),
             "65536 x 8, every 4th first id": phrases(65536, 8, text[::4]),
             "65536 x 8, 64 first ids": phrases(65536, 8, text[:64])}

    def create(p, form):   # form: "old" | "trie"
        offs = (np.arange(len(p) + 1) * p.shape[1]).astype(np.int32)
        b, h = np.full(len(p), 2.0, dtype=np.float32), C.c_void_p()
        flat = np.ascontiguousarray(p.reshape(-1))
        if form == "old":
            rc = lib.fw_boost_create(V, _lib.as_i32p(flat), _lib.as_i32p(offs), len(p), _lib.as_f32p(b), C.byref(h))
        else:
            rc = lib.fw_boost_create_large(V, _lib.as_i32p(flat), _lib.as_i32p(offs), len(p), _lib.as_f32p(b), C.byref(h))
        return h if rc == 0 else None

    def table_words(h):
        n = C.c_int32()
        _lib.check(lib.fw_test_boost_table(h, None, 0, C.byref(n)))
        return n.value

    out_rows = []
    print(f"us per launch, step form, V = {V}, mean of {args.iters} launches after 3")
    print("| list | root edges | table words | rows | history | dec_boost_kernel | dec_boost_trie_kernel |")
    print("|---|---|---|---|---|---|---|")
    for name, p in lists.items():
        hs = {f: create(p, f) for f in ("old", "trie")}
        words = table_words(hs["trie"])
        for rows in (80, 640):
            lg = rng.standard_normal((rows, V)).astype(np.float32)
            for m in (0, 31):
                hist = rng.choice(text, size=(rows, m)).astype(np.int32)
                if m:
                    k = p.shape[1] - 1
                    hist[:, m - k:] = p[rng.integers(0, len(p), size=rows), :k]
                offs = np.arange(rows + 1, dtype=np.int32) * m
                flat = np.ascontiguousarray(hist.reshape(-1)) if m else np.zeros(1, dtype=np.int32)
                us = {}
                for f in ("old", "trie"):
                    if hs[f] is None:
                        continue
                    buf, t = lg.copy(), C.c_float()
                    _lib.check(lib.fw_test_boost_cost(handle, _lib.ptr(buf), rows, _lib.ptr(flat), _lib.ptr(offs), 5, hs[f],
                                                      args.iters, C.byref(t)))
                    us[f] = t.value
                out_rows.append(dict(list=name, root_edges=int(np.unique(p[:, 0]).size), table_words=words, rows=rows, m=m,
                                     us_old=us.get("old"), us_trie=us["trie"]))
                old = f"{us['old']:.1f}" if "old" in us else "—"
                print(f"| {name} | {np.unique(p[:, 0]).size} | {words} | {rows} | {m} | {old} | {us['trie']:.1f} |", flush=True)
        for h in hs.values():
            if h is not None:
                lib.fw_boost_free(h)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(V=V, iters=args.iters, rows=out_rows), f, indent=1)


if __name__ == "__main__":
    main()
