"""Rate conversion of file audio, host against device: ten minutes of noise + a 440 Hz tone at 44 100 Hz and at 48 000 Hz ->
16 kHz.  Per rate, the median of 5 runs after one warm-up of
  host    wall time of audio.resample (numpy, as many BLAS threads as the environment allows)
  device  wall time of audio.resample_device: host arrays in and out, allocations and both copies included
  kernel  GPU time of the kernel alone over the resident recording (fw_bench_resample: HIP events around 5 launches)
and one JSON line.  Fails without a GPU.
    python profiles/resample_bench.py [--seconds 600] [--out profiles/resample_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from faster_whisper_amd import _lib, audio  # noqa: E402


def sig(n, rate, seed, gain=1.0):
    rng = np.random.default_rng(seed); t = np.arange(n, dtype=np.float64) / rate
    return (gain * (0.2 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440.0 * t))).astype(np.float32)


def median_wall(f, runs=5):
    f()                                             # warm-up: code objects, page faults of the output
    times = []
    for _ in range(runs):
        t = time.perf_counter()
        f()
        times.append(time.perf_counter() - t)       # (both functions return host arrays: the device call has synchronised)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    if lib.fw_device_count() <= args.device:
        raise SystemExit("resample_bench: no HIP device (nothing is measured on the CPU alone)")
    rows = []
    for rate in (44100, 48000):
        n = int(args.seconds * rate)
        x = sig(n, rate, seed=rate)
        host = median_wall(lambda: audio.resample(x, rate, 16000))
        dev = median_wall(lambda: audio.resample_device(x, rate, 16000, args.device, quantize_s16=True))
        ms = C.c_float()
        _lib.check(lib.fw_bench_resample(args.device, _lib.ptr(x), n, rate, 16000, 32, 9.0, 1, 5, C.byref(ms)))
        same = bool(np.array_equal(audio.resample_device(x, rate, 16000, args.device, quantize_s16=True),
                                   audio._to_s16_float(audio.resample(x, rate, 16000))))
        n_out = -(-n * 16000 // rate)
        taps = 32 * max(rate, 16000) // 16000 + 1   # multiply-adds per output, within one
        row = {"rate_in": rate, "seconds": args.seconds, "samples_in": n, "samples_out": n_out,
               "host_s": host[0], "host_min_max_s": host[1:], "device_s": dev[0], "device_min_max_s": dev[1:],
               "kernel_ms": ms.value, "host_over_device": host[0] / dev[0],
               "host_x_realtime": args.seconds / host[0], "device_x_realtime": args.seconds / dev[0],
               "bytes_up": 4 * n, "bytes_down": 4 * n_out, "kernel_gflops_fp64": 2.0 * taps * n_out / ms.value / 1e6,
               "s16_equal_to_host": same, "threads": os.environ.get("OMP_NUM_THREADS")}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    slower = [r["rate_in"] for r in rows if r["device_s"] >= r["host_s"]]
    if slower:
        raise SystemExit(f"resample_bench: the device call is not faster than the host function at {slower}")


if __name__ == "__main__":
    main()
