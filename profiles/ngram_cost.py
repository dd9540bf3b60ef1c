"""What one launch of dec_ngram_kernel costs ("Language-model fusion"), through the timing of
fw_test_ngram_rows: the step form at large-v3's vocabulary (51 866 ids), 80 rows (16 chunks x beam 5) and 640 rows (a full
lane of 128 chunks), for a trigram model near FW_NGRAM_MAX_GRAMS — every text id a unigram, 2^19 bigrams and 2^19 - 8
trigrams that extend them — at histories of 0 and 32 ids.  Every history of 32 ends in the context of a trigram, so the walk
goes to its full depth and two sparse levels run.  The kernel only sees the vocabulary size, the rows and the text
context, so the micro model serves as the device handle.

usage: python profiles/ngram_cost.py [--iters 2000] [--out FILE.json]"""
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
    cfg = get_config("micro")
    model = Whisper("synthetic:ngram-cost", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    handle, lib = model._replicas[0].handle, _lib.load()
    rng = np.random.default_rng(0)
    n2, n3 = 1 << 19, (1 << 19) - 8
    # bigrams (w1, w2): 2^19 distinct pairs, a Zipf-like w1 so that some contexts have thousands of successors
    w1 = np.minimum((rng.pareto(1.0, size=4 * n2) * 50).astype(np.int64), EOT - 1)
    pairs = np.unique(w1 * EOT + rng.integers(0, EOT, size=4 * n2))[:n2]
    bi = np.stack([pairs // EOT, pairs % EOT], axis=1)
    tri3 = np.unique(rng.integers(0, n2, size=2 * n3) * EOT + rng.integers(0, EOT, size=2 * n3))[:n3]
    tri = np.concatenate([bi[tri3 // EOT], (tri3 % EOT)[:, None]], axis=1)
    assert len(bi) == n2 and len(tri) == n3
    uni = np.arange(EOT + 1)
    counts = np.asarray([len(uni), n2, n3], dtype=np.int32)
    ids = np.concatenate([uni, bi.reshape(-1), tri.reshape(-1)]).astype(np.int32)
    n = len(uni) + n2 + n3
    lp = -rng.uniform(0.1, 12.0, size=n).astype(np.float32)
    bo = -rng.uniform(0.1, 2.0, size=n).astype(np.float32)
    h = C.c_void_p()
    _lib.check(lib.fw_ngram_create(V, 3, _lib.as_i32p(counts), _lib.as_i32p(ids), _lib.as_f32p(lp), _lib.as_f32p(bo), -15.0, 0.5,
                                   0.1, EOT, C.byref(h)))
    words = C.c_int32()
    _lib.check(lib.fw_test_ngram_table(h, None, 0, C.byref(words)))
    rows_out = []
    print(f"us per launch of dec_ngram_kernel<false>, V = {V}, {n2 + n3} n-grams of order 2 and 3, {words.value} table words, "
          f"mean of {args.iters} launches after 3")
    print("| rows | history | us |")
    print("|---|---|---|")
    for rows in (80, 640):
        lg = rng.standard_normal((rows, V)).astype(np.float32)
        for m in (0, 32):
            hist = rng.integers(0, EOT, size=(rows, m)).astype(np.int32)
            if m:
                hist[:, -2:] = tri[rng.integers(0, n3, size=rows), :2]
            offs = np.arange(rows + 1, dtype=np.int32) * m
            flat = np.ascontiguousarray(hist.reshape(-1)) if m else np.zeros(1, dtype=np.int32)
            out, t = lg.copy(), C.c_float()
            _lib.check(lib.fw_test_ngram_rows(handle, _lib.ptr(out), rows, V, EOT, TSB, _lib.ptr(flat), _lib.ptr(offs), 5, None,
                                              0, h, args.iters, C.byref(t)))
            rows_out.append(dict(rows=rows, m=m, us=t.value))
            print(f"| {rows} | {m} | {t.value:.1f} |", flush=True)
    lib.fw_ngram_free(h)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(V=V, iters=args.iters, table_words=words.value, rows=rows_out), f, indent=1)


if __name__ == "__main__":
    main()
