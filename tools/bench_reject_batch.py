"""Batched rejectWithF and undistortedPoints (libvio_reject_hip.so): B pairs of n = 150 matched points (MAX_CNT) with the default
hypothesis count, B = 1, 16, 64, 256.  Per call: host packing + upload, the kernel (k_reject_ransac or k_reject_lift, HIP events through
vio_reject_timing) and the whole call, the median of --reps calls after --warmup; the kernel time per pair and per hypothesis.

    python tools/bench_reject_batch.py [--out profiles/NAME.json]

The pairs are synthetic two-view scenes (tests/reject_reference.two_view_scene: a stream's landmarks through the EuRoC camera, 0.1 px
of noise, 20 % planted outliers), scene k of a batch drawn with seed k mod 8; undistort matches every point against the other frame's
150 points.  For the comparison DESIGN.md section 16 invites (the same fit out of per-lane scratch), run tools/bench_sfm_batch.py beside
it: its relpose_kernel_ms is k_sfm_relpose's time.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

N = 150


def median(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    import reject_reference as rr
    cam = rr.Camera(**rr.EUROC)
    rh = vio.load_reject().create()
    rh.set_camera(**rr.EUROC)
    rh.set_config()
    H = vio.reject.DEFAULT_HYPOTHESES
    scenes = [rr.two_view_scene(cam, seed=s, n=N)[:2] for s in range(8)]
    ids = np.arange(N, dtype=np.int64)
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        pairs = [dict(cur_pts=scenes[k % 8][0], forw_pts=scenes[k % 8][1], pair=k) for k in range(B)]
        und = [dict(pts=scenes[k % 8][1], ids=ids, prev_ids=ids[::-1].copy(), prev_un_pts=rr.un_points(cam, scenes[k % 8][0])[::-1].copy(), dt=0.05)
               for k in range(B)]
        tr, tu = [], []
        for r in range(args.warmup + args.reps):
            out = rh.reject_batch(pairs)
            t1 = rh.timing()
            rh.undistort_batch(und)
            t2 = rh.timing()
            if r >= args.warmup:
                tr.append(t1)
                tu.append(t2)
        mr, mu = median(tr), median(tu)
        row = dict(batch=B, n=N, hypotheses=H, reject=mr, undistort=mu, reject_kernel_us_per_pair=1e3 * mr["kernel_ms"] / B,
                   reject_kernel_us_per_hypothesis=1e3 * mr["kernel_ms"] / (B * H), undistort_kernel_us_per_item=1e3 * mu["kernel_ms"] / B,
                   inliers_per_pair=float(np.mean([o["n_inliers"] for o in out])), ok_pairs=sum(o["status"] == 0 for o in out))
        rows.append(row)
        print("B %3d  reject: upload %7.3f ms  kernel %8.3f ms  total %8.3f ms  %8.2f us/pair  %6.3f us/hypothesis   undistort: kernel %6.3f ms"
              "  total %7.3f ms   %5.1f inliers per pair, %d ok"
              % (B, mr["upload_ms"], mr["kernel_ms"], mr["total_ms"], row["reject_kernel_us_per_pair"], row["reject_kernel_us_per_hypothesis"],
                 mu["kernel_ms"], mu["total_ms"], row["inliers_per_pair"], row["ok_pairs"]))
    res = dict(bench="reject_batch", n=N, hypotheses=H, reps=args.reps, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    rh.close()


if __name__ == "__main__":
    main()
