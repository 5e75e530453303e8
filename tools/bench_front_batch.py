"""A frame of the whole front end (readImage and updateID) for B image streams of 752 x 480 frames, max_cnt 150, equalised.

  leg read   one FrameHandle.read_batch over the B slots: the join of the steps on the device, one wait     
  leg loop   B frontend.FeatureTracker(frames=FrameHandle, rejecter=RejectHandle, slot=s), each read_image + update_ids: the per-stream
             path, four calls that wait per stream and frame, the point sets through numpy in between        (sections 21 and 23)

Per leg and B = 1, 16, 64: the wall time of a frame (every call of it, the bindings included; each leg ends in a device synchronise),
the median of --reps frames after --warmup, with the least and the most; for leg read the library's own split of its last call by stage
(vio_frame_read_timing, medians) and the bytes moved per frame (the library's counters).  The two legs of a B run back to back, and
--repeats runs the whole measurement again that many times with the order of the legs alternating, for the spread.  Both legs see the
same images and times from the same empty state, and the outputs of the last frame are compared byte for byte (`same`).

    python tools/bench_front_batch.py [--batches 1,16,64] [--reps 20] [--warmup 3] [--repeats 3] [--slot-cameras none|pinhole|mixed]
                                      [--flow-back [--back-levels 2]] [--no-reject] [--legs read,loop] [--out profiles/NAME.json]
                                      [--predict [--min-tracked K]]

--slot-cameras (include/vio_frame_camera.h): none: the handle's camera alone, the PINHOLE kernels; pinhole: every
slot has that same camera as its own, so the same arithmetic runs through the general kernels and the camera table; mixed: slot s has
the handle's camera, a KANNALA_BRANDT, a MEI or a SCARAMUZZA camera of its own by s mod 4, and leg loop's rejecter is a
camera.CameraHandle.bind(s) with the same cameras.

--flow-back (include/vio_frame_back.h): the forward-backward check of the tracker over --back-levels levels, in both
legs; --no-reject: no rejectWithF in a published frame, in both legs.  --legs read: leg read alone (no comparison).

--predict (include/vio_frame_predict.h): from the second frame on every stream gets a prediction for each of its
points, the point's own pixel moved by half a pixel, inside the timed frame: leg read through BatchFeatureTracker.set_predictions (one
call), leg loop through FeatureTracker.set_prediction.  --min-tracked K arms the fallback in both legs: 1 never falls back here (the
second pass runs over rows that leave at once), 1024 makes every stream fall back.  Rows gain `fell_back`, the streams that did in the
last frame.

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
# the other three models at 752 x 480 (KANNALA_BRANDT and MEI: tests/camera_reference.py's)
SLOT_CAMERAS = [
    None,
    dict(model=1, width=752, height=480, k2=-0.0125, k3=0.0045, k4=-0.0031, k5=0.00052, mu=150.0, mv=150.5, u0=376.0, v0=240.5, theta_max=1.6),
    dict(model=2, width=752, height=480, xi=0.9, k1=-0.12, k2=0.03, p1=2e-4, p2=-3e-4, gamma1=830.0, gamma2=828.0, u0=371.5, v0=243.25),
    dict(model=3, width=752, height=480, poly0=-260.0, poly1=0.0, poly2=6e-4, ac=0.9995, ad=2.5e-4, ae=-1.5e-4, cx=375.25, cy=240.5),
]
KEYS = ("pts", "ids", "track_cnt", "un_pts", "velocity")
STAGES = ("host_ms", "push_ms", "track_ms", "reject_ms", "detect_ms", "finish_ms", "readback_ms", "total_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slot-cameras", choices=("none", "pinhole", "mixed"), default="none")
    ap.add_argument("--flow-back", action="store_true")
    ap.add_argument("--back-levels", type=int, default=2)
    ap.add_argument("--no-reject", action="store_true")
    ap.add_argument("--legs", default="read,loop")
    ap.add_argument("--out", default=None)
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--min-tracked", type=int, default=0)
    args = ap.parse_args()
    vio = g.load_package()
    cfg = dict(equalize=True, clahe=dict(clip_limit=3.0, tiles=(8, 8)), flow={}, detect=dict(min_distance=MIN_DIST))
    pair = [np.load(os.path.join(GOLDEN, "flow_image_%d.npz" % k))["image"] for k in (1, 2)]
    batches = [int(b) for b in args.batches.split(",")]
    raw = [[np.roll(im, k, axis=0) for k in range(max(batches))] for im in pair]                   # raw[parity][stream]
    frames = args.warmup + args.reps
    legs = tuple(args.legs.split(","))
    extra = dict(flow_back=dict(levels=args.back_levels) if args.flow_back else None, reject_with_f=not args.no_reject)
    if args.predict:
        extra["prediction"] = dict(min_tracked=args.min_tracked)
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
            own = {}
            if args.slot_cameras == "pinhole":
                own = {s: dict(model=0, **EUROC) for s in range(B)}
            elif args.slot_cameras == "mixed":
                own = {s: SLOT_CAMERAS[s % 4] for s in range(B) if s % 4}
                ch = vio.load_camera().create()
                for s in range(B):
                    ch.set_camera(slot=s, **own.get(s, dict(model=0, **EUROC)))
            for leg in (legs if rep % 2 == 0 else legs[::-1]):
                wall, parts, moved = [], [], None
                if leg == "read":
                    bt = vio.BatchFeatureTracker(fr, range(B), max_cnt=MAX_CNT, min_dist=MIN_DIST, cameras=own, **extra)
                else:
                    fts = [vio.FeatureTracker(None, None, max_cnt=MAX_CNT, min_dist=MIN_DIST, rejecter=ch.bind(s) if args.slot_cameras == "mixed" else rh,
                                              frames=lo, slot=s, **extra) for s in range(B)]
                for t in range(frames):
                    imgs = raw[t & 1][:B]
                    c0 = fr.counters() if leg == "read" else None
                    guesses = [(o["ids"], o["pts"] + np.float32(0.5)) for o in outs] if args.predict and t > 0 else None
                    t0 = time.perf_counter()
                    if leg == "read":
                        if guesses is not None:
                            bt.set_predictions(dict(enumerate(guesses)))
                        outs = bt.read_images(imgs, DT * t)
                    else:
                        outs = []
                        for s in range(B):
                            if guesses is not None:
                                fts[s].set_prediction(*guesses[s])
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
                if args.predict:
                    row["fell_back"] = int(sum(p["fell_back"] for p in (bt.pred_info if leg == "read" else [ft.pred_info for ft in fts])))
                if leg == "read":
                    row["stages_ms"] = {k: float(np.median([p[k] for p in parts])) for k in STAGES}
                    row["bytes_per_frame"] = moved
                rows.append(row)
                print("repeat %d  B %3d  leg %-4s  frame %9.3f ms (%.3f .. %.3f)  %9.1f us/stream  points %.1f  %s"
                      % (rep, B, leg, row["frame_ms"], row["frame_ms_min"], row["frame_ms_max"], row["us_per_stream"], row["points_per_stream"],
                         " ".join("%s %.3f" % (k[:-3], v) for k, v in row.get("stages_ms", {}).items())), flush=True)
            if len(last) == 2:
                same = all(a[k].tobytes() == b[k].tobytes() for a, b in zip(last["read"], last["loop"]) for k in KEYS)
                rows.append(dict(repeat=rep, batch=B, same=bool(same)))
                print("repeat %d  B %3d  outputs of the two legs identical: %s" % (rep, B, same), flush=True)
            for h in (fr, lo, rh) + ((ch,) if args.slot_cameras == "mixed" else ()):
                h.close()
    res = dict(bench="front_batch", slot_cameras=args.slot_cameras, flow_back=bool(args.flow_back), back_levels=args.back_levels if args.flow_back else None,
               reject_with_f=not args.no_reject, predict=bool(args.predict), min_tracked=args.min_tracked if args.predict else None, image="%dx%d" % (pair[0].shape[1], pair[0].shape[0]), max_cnt=MAX_CNT, min_dist=MIN_DIST, reps=args.reps,
               warmup=args.warmup, repeats=args.repeats, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
