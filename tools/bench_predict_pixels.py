"""frontend.predict_pixels_batch for B streams against B frontend.predict_pixels calls: the wall time of the
whole prediction of a frame, through the bindings, medians of --reps after --warmup.  Every stream is a slot of one fm.FmHandle seeded
with the 150-row track table of tests/predict_inputs.py and a slot of one camera.CameraHandle with the EuRoC PINHOLE camera.

    python tools/bench_predict_pixels.py [--batch 64] [--reps 20] [--warmup 3] [--out profiles/NAME.json]
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
import __graft_entry__ as g  # noqa: E402
import camera_reference as cr  # noqa: E402
import predict_inputs as pi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    fe, B = vio.frontend, args.batch
    fmh, ch = vio.load_fm().create(), vio.load_camera().create()
    poses, ext, _ = pi.poses(8)
    t, _ = pi.table(150, 10)
    cam = cr.Camera(**cr.EUROC)
    for s in range(B):
        fmh.tracks_set(s, *[t[k] for k in ("ids", "start", "depth", "flag", "off", "pts")])
        ch.set_camera(slot=s, **cr.EUROC)
    items = [dict(frame_count=10, poses=poses, ext=ext, fm_slot=s, camera_slot=s) for s in range(B)]
    size = dict(width=cam.width, height=cam.height)
    wall = dict(batch=[], loop=[])
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        got = fe.predict_pixels_batch(fmh, ch, items, **size)
        t1 = time.perf_counter()
        ref = [fe.predict_pixels(fmh, ch, 10, poses, ext, fm_slot=s, camera_slot=s, **size) for s in range(B)]
        t2 = time.perf_counter()
        if k >= args.warmup:
            wall["batch"].append(1e3 * (t1 - t0))
            wall["loop"].append(1e3 * (t2 - t1))
    same = all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(got, ref))
    res = dict(bench="predict_pixels", batch=B, reps=args.reps, warmup=args.warmup, rows_per_stream=float(np.mean([len(a[0]) for a in got])), same=bool(same),
               batch_ms=float(np.median(wall["batch"])), batch_ms_min=float(np.min(wall["batch"])), batch_ms_max=float(np.max(wall["batch"])),
               loop_ms=float(np.median(wall["loop"])), loop_ms_min=float(np.min(wall["loop"])), loop_ms_max=float(np.max(wall["loop"])))
    fmh.close()
    ch.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
