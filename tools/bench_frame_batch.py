"""The image steps of the front end for B image streams of 752 x 480 frames, per frame: equalise, track 150 points, detect up to 150.

  leg a   the host-array path: ClaheHandle.apply_batch, FlowHandle.track_batch (the equalised pair), DetectHandle.detect_batch (the
          equalised image), each from host arrays                     (libvio_clahe_hip, libvio_flow_hip, libvio_detect_hip)
  leg b   the resident path: FrameHandle.push_batch, track_batch, detect_batch          (libvio_frame_hip)

Per leg and B = 1, 16, 64: the wall time of a frame (every call of it, the binding included), the median of --reps frames after --warmup,
the kernels' ms of that frame from HIP events, and the bytes moved each way per frame (leg b: the library's counters; leg a: counted from
what its calls are handed and hand back: four image uploads and one download per stream).  --repeats runs the whole measurement again
that many times, for the spread.  --lib-dir takes leg a's three libraries from another directory (a build of another commit): leg b is
then left out.

    python tools/bench_frame_batch.py [--legs a,b] [--repeats 5] [--lib-dir DIR] [--out profiles/NAME.json]

Stream k sees the fixture pair (tests/golden/flow_image_1.npz, flow_image_2.npz) alternating, shifted down by k rows (wrapped).  The
points tracked out of a frame are that frame's own corners (detected once, before the clock starts); the tracked points handed to the
detection are those the tracker kept.
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
N_PTS, MAX_TOTAL = 150, 150


def kept(out, shape):
    """The tracked points a front end would hand to the detection: status OK, rounded inside the image."""
    h, w = shape
    p = out["next_pts"][out["status"] == 0]
    r = np.rint(p.astype(np.float64))
    return p[(r[:, 0] >= 0) & (r[:, 0] < w) & (r[:, 1] >= 0) & (r[:, 1] < h)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--lib-dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    legs = [x for x in args.legs.split(",") if x]
    if args.lib_dir:
        legs = ["a"]
        d = os.path.abspath(args.lib_dir)
        clahe_lib, flow_lib, detect_lib = (vio.ClaheLib(os.path.join(d, "libvio_clahe_hip.so")), vio.FlowLib(os.path.join(d, "libvio_flow_hip.so")),
                                           vio.DetectLib(os.path.join(d, "libvio_detect_hip.so")))
    else:
        clahe_lib, flow_lib, detect_lib = vio.load_clahe(), vio.load_flow(), vio.load_detect()
    ch, fh, dh = clahe_lib.create(), flow_lib.create(), detect_lib.create()
    ch.set_config(clip_limit=3.0, tiles=(8, 8))
    fh.set_config()
    dh.set_config(min_distance=30)
    fr = None
    if "b" in legs:
        fr = vio.load_frame().create()
        fr.set_config(equalize=True, clahe=dict(clip_limit=3.0, tiles=(8, 8)), flow={}, detect=dict(min_distance=30))
    pair = [np.load(os.path.join(GOLDEN, "flow_image_%d.npz" % k))["image"] for k in (1, 2)]
    shape = pair[0].shape
    px = pair[0].size
    batches = [int(b) for b in args.batches.split(",")]
    Bmax = max(batches)
    raw = [[np.roll(im, k, axis=0) for k in range(Bmax)] for im in pair]                   # raw[parity][stream]
    eq0 = [ch.apply_batch(raw[p]) for p in (0, 1)]
    corners = [[o["new_pts"][:N_PTS] for o in dh.detect_batch([dict(img=e, max_total=N_PTS) for e in eq0[p]])] for p in (0, 1)]
    frames = args.warmup + args.reps
    rows = []
    for rep in range(args.repeats):
        for B in batches:
            for leg in legs:
                wall, kern, moved, parts = [], [], [], []
                prev_eq = None
                if leg == "b":
                    for s in range(B):
                        fr.reset(s)
                for t in range(frames + 1):                  # (frame 0 fills prev: it is not timed)
                    p = t & 1
                    pts = corners[1 - p]                     # the corners of the frame before
                    c0 = fr.counters() if leg == "b" else None
                    t0 = time.perf_counter()
                    if leg == "a":
                        eq = ch.apply_batch(raw[p][:B])
                        if t > 0:
                            tr = fh.track_batch([dict(img_prev=prev_eq[s], img_next=eq[s], prev_pts=pts[s]) for s in range(B)])
                            de = dh.detect_batch([dict(img=eq[s], tracked=kept(tr[s], shape), max_total=MAX_TOTAL) for s in range(B)])
                        prev_eq = eq
                    else:
                        fr.push_batch([dict(slot=s, img=raw[p][s]) for s in range(B)])
                        if t > 0:
                            tr = fr.track_batch([dict(slot=s, prev_pts=pts[s]) for s in range(B)])
                            de = fr.detect_batch([dict(slot=s, tracked=kept(tr[s], shape), max_total=MAX_TOTAL) for s in range(B)])
                    dt = 1e3 * (time.perf_counter() - t0)
                    # (the handles keep the timing of their last call: it is read outside the clock)
                    if leg == "a":
                        tm = dict(clahe=ch.timing(), flow=fh.timing(), detect=dh.timing())
                        k_ms = tm["clahe"]["lut_ms"] + tm["clahe"]["apply_ms"]
                        if t > 0:
                            k_ms += tm["flow"]["pyramid_ms"] + tm["flow"]["track_ms"] + sum(tm["detect"][k] for k in ("setmask_ms", "response_ms", "candidates_ms", "select_ms"))
                        if t > args.warmup:
                            parts.append(tm)
                    if leg == "b":
                        tm = fr.timing()
                        k_ms = tm["push_clahe_ms"] + tm["push_pyramid_ms"] + (tm["track_ms"] + tm["detect_ms"] if t > 0 else 0.0)
                        c1 = fr.counters()
                        if t > args.warmup:
                            parts.append(dict(frame=tm))
                        moved.append([c1[k] - c0[k] for k in ("image_up", "image_down", "other_up", "other_down")])
                    else:
                        moved.append([4 * B * px, B * px, 0, 0])         # (the tables and results of leg a are not counted)
                    if t > args.warmup:
                        wall.append(dt)
                        kern.append(k_ms)
                n_trk = float(np.mean([len(kept(o, shape)) for o in tr]))
                n_new = float(np.mean([o["n_new"] for o in de]))
                row = dict(repeat=rep, batch=B, leg=leg, frame_ms=float(np.median(wall)), frame_ms_min=float(np.min(wall)),
                           frame_ms_max=float(np.max(wall)), us_per_stream=1e3 * float(np.median(wall)) / B, kernels_ms=float(np.median(kern)),
                           bytes_per_frame=dict(zip(("image_up", "image_down", "other_up", "other_down"), [int(x) for x in moved[-1]])),
                           tracked_per_stream=n_trk, new_per_stream=n_new)
                # the libraries' own timing of their calls (ms, medians over the timed frames)
                row["timing"] = {lib: {k: float(np.median([x[lib][k] for x in parts])) for k in parts[0][lib]} for lib in parts[0]}
                rows.append(row)
                print("repeat %d  B %3d  leg %s  frame %9.3f ms (%.3f .. %.3f)  %9.1f us/stream  kernels %8.3f ms  image bytes up %d down %d"
                      "  tracked %.1f new %.1f" % (rep, B, leg, row["frame_ms"], row["frame_ms_min"], row["frame_ms_max"], row["us_per_stream"],
                                                   row["kernels_ms"], moved[-1][0], moved[-1][1], n_trk, n_new), flush=True)
    res = dict(bench="frame_batch", image="%dx%d" % (shape[1], shape[0]), points=N_PTS, max_total=MAX_TOTAL, reps=args.reps, warmup=args.warmup,
               repeats=args.repeats, lib_dir=args.lib_dir, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for h in (ch, fh, dh, fr):
        if h is not None:
            h.close()


if __name__ == "__main__":
    main()
