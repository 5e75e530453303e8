"""Batched camera-IMU extrinsic rotation calibration (include/vio_exrot.h) on the GPU: one JSON line.

For B = 1, 16, 64, 256 windows (directly built windows of tests/exrot_reference.py: F = 11, 8 degrees of rotation per frame, 400 points,
about 60 correspondences per pair, 0.1 px of pixel noise, drawn with 8 seeds), the median over --reps calls of:
  pairs_ms_per_call / _per_window        vio_exrot_relative_rotations_batch, the whole call (Python packing included)
  calibrate_ms_per_call / _per_window    vio_exrot_calibrate_batch on stage 1's rotations
  exrot_ms_per_call / _per_window        vio_exrot_batch, both stages in one call
  pairs_kernel_ms, solve_kernel_ms       the kernels' HIP-event times inside vio_exrot_batch
and python_restatement_ms_per_window: tests/exrot_reference.py's exrot() on one window, a Python figure (numpy), not a CPU baseline.
The reference has no timing of this step to hold these against.

    python tools/bench_exrot_batch.py [--reps 5] [--batches 1,16,64,256] [--once B]

--once B makes a single vio_exrot_batch call of B windows after one warm-up call (for a profiler run).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    import __graft_entry__ as g
    vio = g.load_package()
    vio.load_hip()
    import exrot_reference as xr
    base = [xr.make_window(s, 8, noise=0.1 / 460.0)[0] for s in range(1, 9)]
    h = vio.load_exrot().create()
    if a.once:
        items = [base[i % 8] for i in range(a.once)]
        h.exrot_batch(items[:1])
        res = h.exrot_batch(items)
        print(json.dumps(dict(tool="bench_exrot_batch", once=a.once, ok_windows=sum(r["status"] == 0 for r in res), **h.timing())))
        return
    out = {"tool": "bench_exrot_batch", "reps": a.reps, "rows": []}
    for B in [int(v) for v in a.batches.split(",")]:
        items = [base[i % 8] for i in range(B)]
        rec = {k: [] for k in ("pairs", "cal", "both", "pairs_k", "solve_k")}
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            pairs = h.relative_rotations_batch(items)
            t1 = time.perf_counter()
            h.calibrate_batch(items, [p["Rc"] for p in pairs])
            t2 = time.perf_counter()
            res = h.exrot_batch(items)
            t3 = time.perf_counter()
            tm = h.timing()
            if rep == 0:
                continue                # warm-up
            rec["pairs"].append((t1 - t0) * 1e3)
            rec["cal"].append((t2 - t1) * 1e3)
            rec["both"].append((t3 - t2) * 1e3)
            rec["pairs_k"].append(tm["pairs_ms"])
            rec["solve_k"].append(tm["solve_ms"])
        med = {k: float(np.median(v)) for k, v in rec.items()}
        out["rows"].append(dict(B=B, ok_windows=sum(r["status"] == 0 for r in res), pairs_ms_per_call=med["pairs"],
                                pairs_ms_per_window=med["pairs"] / B, calibrate_ms_per_call=med["cal"],
                                calibrate_ms_per_window=med["cal"] / B, exrot_ms_per_call=med["both"], exrot_ms_per_window=med["both"] / B,
                                pairs_kernel_ms=med["pairs_k"], solve_kernel_ms=med["solve_k"]))
    ts = []
    for it in base[:3]:
        t0 = time.perf_counter()
        xr.exrot(it)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["python_restatement_ms_per_window"] = float(np.median(ts))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
