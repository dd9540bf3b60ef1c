"""What one launch of dec_boost_graph_kernel costs ("Phrase boosting"), through the timing of
fw_test_boost_graph_cost: the step form at large-v3's vocabulary (51 866 ids, <eot> 50 257, timestamps from 50 365), 80 rows
(16 chunks x beam 5) and 640 rows (a full lane of 128 chunks), on the lists of profiles/boost_trie_cost.py — 16 phrases of 3
ids, 1 024 of 4, 65 536 of 8 with random first ids (some 32 000 distinct ones) and with 64 distinct first ids — and three
kinds of rows:
  - no history, and 31 ids that no phrase holds: the state is the root, G(s) == 0, the sparse pass over the root alone.
    Comparator: dec_boost_trie_kernel on the same list and rows (fw_test_boost_cost), which has the same sparse work;
  - 31 ids that end in all but the last id of a phrase: every row sits mid-phrase, G(s) != 0, the dense take-back pass
    runs.  Comparator: dec_ngram_kernel with a unigram model (fw_test_ngram_rows), which reads and writes the same
    rows x (<eot> + 1) floats.
The kernels only see the vocabulary geometry, the rows and the text context, so the micro model serves as the device handle.

usage: python profiles/boost_graph_cost.py [--iters 2000] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, EOT, TS = 51866, 50257, 50365


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from faster_whisper_amd import Whisper, _lib, get_config, synthetic_weights
    cfg = get_config("micro")
    model = Whisper("synthetic:boost-graph-cost", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    handle, lib = model._replicas[0].handle, _lib.load()
    rng = np.random.default_rng(0)
    text = np.arange(1000, 40000)

    def phrases(count, length, first=text):
        p = rng.choice(text, size=(count, length)).astype(np.int32)
        p[:, 0] = rng.choice(first, size=count)
        return p

    lists = {"16 x 3": phrases(16, 3), "1024 x 4": phrases(1024, 4), "65536 x 8": phrases(65536, 8),
             "65536 x 8, 64 first ids": phrases(65536, 8, text[:64])}

    def create(p, symbol):
        offs = (np.arange(len(p) + 1) * p.shape[1]).astype(np.int32)
        b, h = np.full(len(p), 2.0, dtype=np.float32), C.c_void_p()
        flat = np.ascontiguousarray(p.reshape(-1))
        _lib.check(getattr(lib, symbol)(V, _lib.as_i32p(flat), _lib.as_i32p(offs), len(p), _lib.as_f32p(b), C.byref(h)))
        return h

    lm, counts = C.c_void_p(), np.zeros(1, dtype=np.int32)   # a unigram model: the dense pass and nothing else
    _lib.check(lib.fw_ngram_create(V, 1, _lib.as_i32p(counts), None, None, None, -10.0, 0.5, 0.0, EOT, C.byref(lm)))

    out_rows = []
    print(f"us per launch, step form, V = {V}, mean of {args.iters} launches after 3")
    print("| list | root edges | table words | rows | rows' history | dec_boost_graph_kernel | dec_boost_trie_kernel | dec_ngram_kernel |")
    print("|---|---|---|---|---|---|---|---|")
    for name, p in lists.items():
        graph, trie = create(p, "fw_boost_create_revocable"), create(p, "fw_boost_create_large")
        n = C.c_int32()
        _lib.check(lib.fw_test_boost_table(graph, None, 0, C.byref(n)))
        for rows in (80, 640):
            lg = rng.standard_normal((rows, V)).astype(np.float32)
            for kind, m in (("none", 0), ("31 off the list", 31), ("31 mid-phrase", 31)):
                hist = rng.choice(np.arange(100, 900), size=(rows, m)).astype(np.int32)
                if kind == "31 mid-phrase":
                    k = p.shape[1] - 1
                    hist[:, m - k:] = p[rng.integers(0, len(p), size=rows), :k]
                offs = np.arange(rows + 1, dtype=np.int32) * m
                flat = np.ascontiguousarray(hist.reshape(-1)) if m else np.zeros(1, dtype=np.int32)
                us = {}
                for what in ("graph", "trie", "ngram"):
                    buf, t = lg.copy(), C.c_float()
                    head = (handle, _lib.ptr(buf), rows)
                    tail = (_lib.ptr(flat), _lib.ptr(offs), 5)
                    if what == "graph":
                        rc = lib.fw_test_boost_graph_cost(*head, V, EOT, TS, *tail, graph, args.iters, C.byref(t))
                    elif what == "trie":
                        rc = lib.fw_test_boost_cost(*head, *tail, trie, args.iters, C.byref(t))
                    else:
                        rc = lib.fw_test_ngram_rows(*head, V, EOT, TS, *tail, None, 0, lm, args.iters, C.byref(t))
                    _lib.check(rc)
                    us[what] = t.value
                out_rows.append(dict(list=name, root_edges=int(np.unique(p[:, 0]).size), table_words=n.value, rows=rows,
                                     history=kind, **{"us_" + k: v for k, v in us.items()}))
                print(f"| {name} | {np.unique(p[:, 0]).size} | {n.value} | {rows} | {kind} | {us['graph']:.1f} | {us['trie']:.1f} | "
                      f"{us['ngram']:.1f} |", flush=True)
        lib.fw_boost_free(graph)
        lib.fw_boost_free(trie)
    lib.fw_ngram_free(lm)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(V=V, iters=args.iters, rows=out_rows), f, indent=1)


if __name__ == "__main__":
    main()
