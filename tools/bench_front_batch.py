"""A frame of the whole front end (readImage and updateID) for B image streams of 752 x 480 frames, max_cnt 150, equalised.

  leg read   one FrameHandle.read_batch over the B slots: the join of the steps on the device, one wait     
  leg loop   B frontend.FeatureTracker(frames=FrameHandle, rejecter=RejectHandle, slot=s), each read_image + update_ids: the per-stream
             path, four calls that wait per stream and frame, the point sets through numpy in between        (sections 21 and 23)

Per leg and B = 1, 16, 64: the wall time of a frame (every call of it, the bindings included; each leg ends in a device synchronise),
the median of --reps frames after --warmup, with the least and the most; for leg read the library's own split of its last call by stage
(vio_frame_read_timing, medians) and the bytes moved per frame (the library's counters).  The two legs of a B run back to back, and
--repeats runs the whole measurement again that many times with the order of the legs alternating, for the spread.  Both legs see the
same images and times from the same empty state, and the outputs of the last frame are compared byte for byte (`same`).

    python tools/bench_front_batch.py [--batches 1,16,64] [--reps 20] [--warmup 3] [--repeats 3] [--out profiles/NAME.json]

Stream k sees the fixture pair (tests/golden/flow_image_1.npz, flow_image_2.npz) alternating, shifted down by k rows (wrapped).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_CNT, MIN_DIST, DT = 150, 30, 0.05
# VM/config/euroc_config.yaml:11-22
EUROC = dict(fx=4.616e+02, fy=4.603e+02, cx=3.630e+02, cy=2.481e+02, k1=-2.917e-01, k2=8.228e-02, p1=5.333e-05, p2=-1.578e-04, width=752, height=480)
KEYS = ("pts", "ids", "track_cnt", "un_pts", "velocity")
STAGES = ("host_ms", "push_ms", "track_ms", "reject_ms", "detect_ms", "finish_ms", "readback_ms", "total_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    cfg = dict(equalize=True, clahe=dict(clip_limit=3.0, tiles=(8, 8)), flow={}, detect=dict(min_distance=MIN_DIST))
    pair = [np.load(os.path.join(GOLDEN, "flow_image_%d.npz" % k))["image"] for k in (1, 2)]
    batches = [int(b) for b in args.batches.split(",")]
    raw = [[np.roll(im, k, axis=0) for k in range(max(batches))] for im in pair]                   # raw[parity][stream]
    frames = args.warmup + args.reps
    rows = []
    for rep in range(args.repeats):
        for B in batches:
            last = {}
            # fresh handles for every B: both legs start from the same empty state, id counters included
            fr, lo, rh = vio.load_frame().create(), vio.load_frame().create(), vio.load_reject().create()
            fr.set_config(**cfg)
            lo.set_config(**cfg)
            fr.set_camera(**EUROC)
            rh.set_camera(**EUROC)
            for leg in (("read", "loop") if rep % 2 == 0 else ("loop", "read")):
                wall, parts, moved = [], [], None
                if leg == "read":
                    bt = vio.BatchFeatureTracker(fr, range(B), max_cnt=MAX_CNT, min_dist=MIN_DIST)
                else:
                    fts = [vio.FeatureTracker(None, None, max_cnt=MAX_CNT, min_dist=MIN_DIST, rejecter=rh, frames=lo, slot=s) for s in range(B)]
                for t in range(frames):
                    imgs = raw[t & 1][:B]
                    c0 = fr.counters() if leg == "read" else None
                    t0 = time.perf_counter()
                    if leg == "read":
                        outs = bt.read_images(imgs, DT * t)
                    else:
                        outs = []
                        for s in range(B):
                            o = fts[s].read_image(imgs[s], DT * t)
                            o["ids"] = fts[s].update_ids()
                            outs.append(o)
                    dt = 1e3 * (time.perf_counter() - t0)
                    if leg == "read":
                        c1 = fr.counters()
                        moved = {k: c1[k] - c0[k] for k in c1}
                        if t >= args.warmup:
                            parts.append(fr.read_timing())
                    if t >= args.warmup:
                        wall.append(dt)
                last[leg] = outs
                row = dict(repeat=rep, batch=B, leg=leg, frame_ms=float(np.median(wall)), frame_ms_min=float(np.min(wall)),
                           frame_ms_max=float(np.max(wall)), us_per_stream=1e3 * float(np.median(wall)) / B,
                           points_per_stream=float(np.mean([len(o["pts"]) for o in outs])))
                if leg == "read":
                    row["stages_ms"] = {k: float(np.median([p[k] for p in parts])) for k in STAGES}
                    row["bytes_per_frame"] = moved
                rows.append(row)
                print("repeat %d  B %3d  leg %-4s  frame %9.3f ms (%.3f .. %.3f)  %9.1f us/stream  points %.1f  %s"
                      % (rep, B, leg, row["frame_ms"], row["frame_ms_min"], row["frame_ms_max"], row["us_per_stream"], row["points_per_stream"],
                         " ".join("%s %.3f" % (k[:-3], v) for k, v in row.get("stages_ms", {}).items())), flush=True)
            same = all(a[k].tobytes() == b[k].tobytes() for a, b in zip(last["read"], last["loop"]) for k in KEYS)
            rows.append(dict(repeat=rep, batch=B, same=bool(same)))
            print("repeat %d  B %3d  outputs of the two legs identical: %s" % (rep, B, same), flush=True)
            for h in (fr, lo, rh):
                h.close()
    res = dict(bench="front_batch", image="%dx%d" % (pair[0].shape[1], pair[0].shape[0]), max_cnt=MAX_CNT, min_dist=MIN_DIST, reps=args.reps,
               warmup=args.warmup, repeats=args.repeats, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
