"""Batched pyramidal Lucas-Kanade tracking (libvio_flow_hip.so): B pairs of 752 x 480 images with 150 keypoints each (MAX_CNT) in one
call, B = 1, 16, 64, forward and inverse mode.  Per call: host packing + upload, the pyramid kernels, k_flow_track (HIP events) and
the whole call, the median of --reps calls after --warmup; and the whole call per keypoint.

    python tools/bench_flow_batch.py [--back [--back-levels 2]] [--out profiles/NAME.json]

--back: every B and mode a second time with the forward-backward check on (include/vio_flow_back.h) over
--back-levels levels (0: the handle's 4), and the count of keypoints it kept.

The images are the fixture pair (tests/golden/flow_image_*.npz); pair k of a batch is the fixture shifted down by k rows (wrapped), so
that the pairs differ; the keypoints are the first 150 of tests/golden/flow_keypoints.npz.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_PTS = 150


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--back", action="store_true")
    ap.add_argument("--back-levels", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    fh = vio.load_flow().create()
    im1 = np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"]
    im2 = np.load(os.path.join(GOLDEN, "flow_image_2.npz"))["image"]
    kp = np.load(os.path.join(GOLDEN, "flow_keypoints.npz"))["keypoints"][:N_PTS]
    rows = []
    for inverse in (0, 1):
        fh.set_config(inverse=inverse)
        for B, back in [(int(b), k) for b in args.batches.split(",") for k in ((False, True) if args.back else (False,))]:
            fh.set_back(enabled=back, levels=args.back_levels)
            items = [dict(img_prev=np.roll(im1, k, axis=0), img_next=np.roll(im2, k, axis=0), prev_pts=kp) for k in range(B)]
            t = []
            for r in range(args.warmup + args.reps):
                out = fh.track_batch(items)
                if r >= args.warmup:
                    t.append(fh.timing())
            med = {k: float(np.median([x[k] for x in t])) for k in t[0]}
            tracked = int(sum(int(np.sum(o["status"] == 0)) for o in out))
            row = dict(mode="inverse" if inverse else "forward", back=back, back_levels=args.back_levels if back else None, batch=B, keypoints=B * len(kp), tracked=tracked, **med,
                       us_per_keypoint=1e3 * med["total_ms"] / (B * len(kp)))
            rows.append(row)
            print("%-7s %-5s B %3d  upload %8.3f ms  pyramid %7.3f ms  track %7.3f ms  total %8.3f ms  %7.3f us/keypoint  tracked %d / %d"
                  % (row["mode"], "back" if back else "", B, med["upload_ms"], med["pyramid_ms"], med["track_ms"], med["total_ms"], row["us_per_keypoint"],
                     tracked, B * len(kp)))
    res = dict(bench="flow_batch", image="752x480", keypoints_per_pair=len(kp), reps=args.reps, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    fh.close()


if __name__ == "__main__":
    main()
