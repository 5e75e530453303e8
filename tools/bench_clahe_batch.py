"""Batched CLAHE equalisation (libvio_clahe_hip.so): B images of 752 x 480 with the reference's settings (clip limit 3, 8 x 8 tiles) in
one call, B = 1, 16, 64.  Per
call: host packing + upload, k_clahe_lut, k_clahe_apply (HIP events) and the whole call, the median of --reps calls after --warmup;
the whole call and the two kernels per image; the rate at which the two kernels move the 1.08 MB an image needs (read twice, written
once) beside the HBM peak.

    python tools/bench_clahe_batch.py [--out profiles/NAME.json]

The image is the fixture (tests/golden/flow_image_1.npz); image k of a batch is the fixture shifted down by k rows (wrapped), so that the
images differ.
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
HBM_PEAK_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    ch = vio.load_clahe().create()
    im = np.load(os.path.join(GOLDEN, "flow_image_1.npz"))["image"]
    batches = [int(b) for b in args.batches.split(",")]
    images = [np.roll(im, k, axis=0) for k in range(max(batches))]
    bytes_per_image = 3 * im.size                                   # read for the histograms, read for the blend, written once
    ch.set_config(clip_limit=3.0, tiles=(8, 8))
    rows = []
    for B in batches:
        outs = [np.empty_like(a) for a in images[:B]]
        t = []
        for r in range(args.warmup + args.reps):
            ch.apply_batch(images[:B], out=outs)
            if r >= args.warmup:
                t.append(ch.timing())
        med = {k: float(np.median([x[k] for x in t])) for k in t[0]}
        kernels_ms = med["lut_ms"] + med["apply_ms"]
        row = dict(batch=B, **med, us_per_image=1e3 * med["total_ms"] / B, lut_us_per_image=1e3 * med["lut_ms"] / B,
                   apply_us_per_image=1e3 * med["apply_ms"] / B, kernels_tb_per_s=B * bytes_per_image / (kernels_ms * 1e-3) / 1e12)
        rows.append(row)
        print("B %3d  upload %8.3f ms  lut %7.3f ms  apply %7.3f ms  total %8.3f ms  %8.1f us/image (lut %6.2f, apply %6.2f)"
              "  kernels %.3f TB/s of %.1f peak"
              % (B, med["upload_ms"], med["lut_ms"], med["apply_ms"], med["total_ms"], row["us_per_image"], row["lut_us_per_image"],
                 row["apply_us_per_image"], row["kernels_tb_per_s"], HBM_PEAK_TBS))
    res = dict(bench="clahe_batch", image="752x480", clip_limit=3.0, tiles=[8, 8], bytes_per_image=bytes_per_image, hbm_peak_tb_per_s=HBM_PEAK_TBS,
               reps=args.reps, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ch.close()


if __name__ == "__main__":
    main()
