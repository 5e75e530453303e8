"""Batched non-keyframe PnP (include/vio_pnp.h) on the GPU: one JSON line.

For B = 1, 16, 64, 256 windows (the 21-frame MH_05 window of tests/pnp_reference.py: 11 keyframes, 10 non-keyframes of 60 to 570
usable points, 0.1 px of pixel noise; the points and keyframe poses are tests/sfm_reference.py's, computed once), the median over
--reps calls of:
  ms_per_call / _per_window / _per_frame     vio_pnp_frames_batch, the whole call (Python packing included)
  kernel_ms, kernel_us_per_frame             k_pnp_frames' HIP-event time inside that call (vio_pnp_timing)
  host_ms                                    host packing + upload
Nothing on the CPU side of this repository computes the same thing in compiled code, so there is no baseline and no ratio.

    python tools/bench_pnp_batch.py [--reps 5] [--batches 1,16,64,256] [--once B]

--once B makes a single call of B windows after one warm-up call (for a profiler run).
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
    import pnp_reference as pr
    item = pr.fixture("mh")["item"]
    nf = len(item["guess_key"])
    h = vio.load_pnp().create()
    if a.once:
        h.frames_batch([item])
        res = h.frames_batch([item] * a.once)
        print(json.dumps(dict(tool="bench_pnp_batch", once=a.once, ok_windows=sum(r["status"] == 0 for r in res), **h.timing())))
        return
    out = {"tool": "bench_pnp_batch", "reps": a.reps, "frames_per_window": nf, "points_per_frame": [int(v) for v in h.frames_batch([item])[0]["n_used"]],
           "rows": []}
    for B in [int(v) for v in a.batches.split(",")]:
        items = [item] * B
        rec = {k: [] for k in ("call", "kernel", "host")}
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            res = h.frames_batch(items)
            t1 = time.perf_counter()
            tm = h.timing()
            if rep == 0:
                continue                # warm-up
            rec["call"].append((t1 - t0) * 1e3)
            rec["kernel"].append(tm["kernel_ms"])
            rec["host"].append(tm["host_ms"])
        med = {k: float(np.median(v)) for k, v in rec.items()}
        out["rows"].append(dict(B=B, ok_windows=sum(r["status"] == 0 for r in res), ms_per_call=med["call"], ms_per_window=med["call"] / B,
                                ms_per_frame=med["call"] / (B * nf), kernel_ms=med["kernel"], kernel_us_per_frame=1e3 * med["kernel"] / (B * nf),
                                host_ms=med["host"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
