"""Batched structure-from-motion (include/vio_sfm.h) on the GPU: one JSON line.

For B = 1, 16, 64, 256 windows (the first MH_05 window: F = 11, 40 landmarks per frame, tracks of 10 frames, 0.1 px of pixel noise,
drawn with 8 seeds), the median over --reps calls of:
  relpose_ms_per_call / _per_window      vio_sfm_relative_pose_batch, the whole call (Python packing included)
  construct_ms_per_call / _per_window    vio_sfm_construct_batch on stage 1's results
  sfm_ms_per_call / _per_window          vio_sfm_batch, both stages in one call
  relpose_kernel_ms, construct_kernel_ms the kernels' HIP-event times inside vio_sfm_batch
and python_restatement_ms_per_window: tests/sfm_reference.py's sfm() on one window, a Python figure (numpy), not a CPU baseline.

    python tools/bench_sfm_batch.py [--reps 5] [--batches 1,16,64,256] [--once B]

--once B makes a single vio_sfm_batch call of B windows after one warm-up call (for a profiler run).
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
    from vio_amd import stream as vs
    import sfm_reference as sr
    mh = dict(np.load(os.path.join(ROOT, "tests", "golden", "mh05_imu_stretch.npz")))
    base = [sr.window_item(vs.RealImuStream(mh, n_frames=12, landmarks_per_frame=40, track_len=10, seed=s, pixel_noise=0.1 / 460.0),
                           list(range(11)))[0] for s in range(8)]
    h = vio.load_sfm().create()
    if a.once:
        items = [base[i % 8] for i in range(a.once)]
        h.sfm_batch(items[:1])
        res = h.sfm_batch(items)
        print(json.dumps(dict(tool="bench_sfm_batch", once=a.once, ok_windows=sum(r["status"] == 0 for r in res), **h.timing())))
        return
    out = {"tool": "bench_sfm_batch", "reps": a.reps, "rows": []}
    for B in [int(v) for v in a.batches.split(",")]:
        items = [base[i % 8] for i in range(B)]
        rec = {k: [] for k in ("rel", "con", "sfm", "rel_k", "con_k")}
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            rel = h.relative_pose_batch(items)
            t1 = time.perf_counter()
            h.construct_batch(items, rel)
            t2 = time.perf_counter()
            res = h.sfm_batch(items)
            t3 = time.perf_counter()
            tm = h.timing()
            if rep == 0:
                continue                # warm-up
            rec["rel"].append((t1 - t0) * 1e3)
            rec["con"].append((t2 - t1) * 1e3)
            rec["sfm"].append((t3 - t2) * 1e3)
            rec["rel_k"].append(tm["relpose_ms"])
            rec["con_k"].append(tm["construct_ms"])
        med = {k: float(np.median(v)) for k, v in rec.items()}
        out["rows"].append(dict(B=B, ok_windows=sum(r["status"] == 0 for r in res), relpose_ms_per_call=med["rel"],
                                relpose_ms_per_window=med["rel"] / B, construct_ms_per_call=med["con"],
                                construct_ms_per_window=med["con"] / B, sfm_ms_per_call=med["sfm"], sfm_ms_per_window=med["sfm"] / B,
                                relpose_kernel_ms=med["rel_k"], construct_kernel_ms=med["con_k"]))
    ts = []
    for it in base[:3]:
        t0 = time.perf_counter()
        sr.sfm(it)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["python_restatement_ms_per_window"] = float(np.median(ts))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
