"""Batched corner detection with setMask (libvio_detect_hip.so): B images of 752 x 480 with max_total 150 (MAX_CNT) in one call,
B = 1, 16, 64, with 0 and with 100 tracked points per image.  Per call: host packing + upload, k_detect_setmask, k_detect_response,
k_detect_candidates, k_detect_select (HIP events) and the whole call, the median of --reps calls after --warmup; the whole call per
image; the candidates per image.

    python tools/bench_detect_batch.py [--out profiles/NAME.json]

The image is the fixture (tests/golden/flow_image_1.npz); image k of a batch is the fixture shifted down by k rows (wrapped), so that the
images differ; the tracked points of an image are the first 100 corners the detector itself finds in it.
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
MAX_TOTAL, N_TRACKED = 150, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    dh = vio.load_detect().create()
    im = np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"]
    batches = [int(b) for b in args.batches.split(",")]
    images = [np.roll(im, k, axis=0) for k in range(max(batches))]
    corners = [o["new_pts"][:N_TRACKED] for o in dh.detect_batch([dict(img=a, max_total=MAX_TOTAL) for a in images])]
    rows = []
    for n_tracked in (0, N_TRACKED):
        for B in batches:
            items = [dict(img=images[k], tracked=corners[k][:n_tracked], track_cnt=np.ones(min(n_tracked, len(corners[k])), dtype=np.int32),
                          max_total=MAX_TOTAL) for k in range(B)]
            t = []
            for r in range(args.warmup + args.reps):
                out = dh.detect_batch(items)
                if r >= args.warmup:
                    t.append(dh.timing())
            med = {k: float(np.median([x[k] for x in t])) for k in t[0]}
            row = dict(tracked=n_tracked, batch=B, **med, us_per_image=1e3 * med["total_ms"] / B,
                       candidates_per_image=float(np.mean([o["n_candidates"] for o in out])), kept_per_image=float(np.mean([o["n_kept"] for o in out])),
                       new_per_image=float(np.mean([o["n_new"] for o in out])))
            rows.append(row)
            print("tracked %3d B %3d  upload %8.3f ms  setmask %6.3f ms  response %6.3f ms  candidates %6.3f ms  select %7.3f ms  total %8.3f ms"
                  "  %8.1f us/image  %6.0f candidates, %5.1f kept, %5.1f new per image"
                  % (n_tracked, B, med["upload_ms"], med["setmask_ms"], med["response_ms"], med["candidates_ms"], med["select_ms"],
                     med["total_ms"], row["us_per_image"], row["candidates_per_image"], row["kept_per_image"], row["new_per_image"]))
    res = dict(bench="detect_batch", image="752x480", max_total=MAX_TOTAL, reps=args.reps, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    dh.close()


if __name__ == "__main__":
    main()
