"""A frame of the FeatureManager for B streams of 150 points per image on full 11-frame windows: addFeatureCheckParallax, triangulate
and the window arrays, setDepth with removeFailures, and the slide the keyframe decision asks for.

  leg batch  fm.BatchFeatureManager over B slots of one FmHandle: four batched calls per frame, each one launch and one wait
             
  leg loop   B host mirrors vio::FeatureManager (host/feature_manager.cpp), each with its waiting vio_triangulate, looped in C++
             (tools/bench_fm_host.cpp, built here into a shared object and called in this process): the per-stream path

Per leg and B = 1, 16, 64, 256: the wall time of a frame at frame_count = 10, the median of --reps frames after the window has filled
and --warmup more, with the least and the most.  Leg loop is timed inside the C++ loop (nothing of Python in it); leg batch is timed
around the four Python calls (bindings included) and, as lib_ms, as the sum of the library's own whole-call times (vio_fm_timing),
with the stage split of each call.  The two legs of a B run back to back, and --repeats runs the whole measurement again that many
times with the order of the legs alternating, for the spread.  Both legs see the same images from the same empty state; the keyframe
decisions and the track counts of the last frame are compared (`same`).

    python tools/bench_fm_batch.py [--batches 1,16,64,256] [--reps 20] [--warmup 3] [--repeats 3] [--out profiles/NAME.json]

--remove measures erasing a tenth of the rows of B slots by feature id instead, B = 1, 16, 64 (--batches) and
150 and 2048 tracks per slot:

  leg batch  one FmHandle.remove_batch over the B slots (include/vio_fm_outlier.h): one launch and one wait
  leg host   per slot tracks_get, the erase on the host (a numpy mask over the arrays) and tracks_set: the route without the call

Every repetition seeds the slots afresh (not timed); the two legs alternate as above and must leave the same tables (`same`).

--predict measures predictPtsInNextFrame of B slots of 150 tracks, B = 1 and 64 (--batches), against a loop over
the numpy restatement (measure_predict).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

POINTS, WINDOW = 150, 10
HOST = os.path.join(ROOT, "visual-inertial-odometry_amd", "host")
CALLS = ("add", "export", "set_depth", "slide")


def build_host_leg(csrc):
    d = tempfile.mkdtemp(prefix="bench_fm_")
    so = os.path.join(d, "libbench_fm_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", os.path.join(ROOT, "tools", "bench_fm_host.cpp"),
                           os.path.join(HOST, "feature_manager.cpp"), os.path.join(HOST, "estimator_backend.cpp"), "-L" + csrc, "-lvio_hip",
                           "-Wl,-rpath," + csrc, "-o", so])
    dll = C.CDLL(so)
    dll.fmh_create.restype, dll.fmh_create.argtypes = C.c_void_p, [C.c_int32]
    dll.fmh_destroy.restype, dll.fmh_destroy.argtypes = None, [C.c_void_p]
    dll.fmh_frame.restype, dll.fmh_frame.argtypes = C.c_double, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 10
    return dll


def make_stream(seed, frames):
    """[(ids (POINTS,) int64 shuffled, pts (POINTS, 2))] per frame: tracked points, a tenth lost and replaced per frame, the step size
    changing so that both keyframe decisions occur."""
    rng = np.random.RandomState(seed)
    ids, pts, nxt = np.arange(POINTS, dtype=np.int64), rng.uniform(-0.5, 0.5, (POINTS, 2)), POINTS
    out = []
    for f in range(frames):
        order = rng.permutation(POINTS)
        out.append((ids[order].copy(), pts[order].copy()))
        pts = pts + (0.03 if (f // 3) % 2 else 0.003) * rng.normal(size=(POINTS, 2))
        lost = np.nonzero(rng.uniform(size=POINTS) < 0.1)[0]
        ids[lost] = np.arange(nxt, nxt + len(lost))
        pts[lost] = rng.uniform(-0.5, 0.5, (len(lost), 2))
        nxt += len(lost)
    return out


def remove_tracks(n, seed):
    """n rows as arrays (ids, start, depth, flag, off, pts): 1 .. 11 observations, ids above 2^31 and not sorted."""
    rng = np.random.RandomState(seed)
    k = rng.randint(1, 12, size=n)
    start = (rng.uniform(size=n) * (12 - k)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    return (rng.permutation(n).astype(np.int64) * 2500013 + 2 ** 31 + 11, start, rng.uniform(2.0, 9.0, n), np.zeros(n, dtype=np.int32), off,
            rng.uniform(-0.7, 0.7, (int(off[-1]), 2)))


def host_erase(tr, gone):
    """tracks_get's dict without the rows whose id is in `gone`, as tracks_set's arguments."""
    keep = ~np.isin(tr["ids"], gone)
    k = np.diff(tr["off"])
    off = np.concatenate([[0], np.cumsum(k[keep])]).astype(np.int64)
    return tr["ids"][keep], tr["start"][keep], tr["depth"][keep], tr["flag"][keep], off, tr["pts"][np.repeat(keep, k)]


def measure_remove(vio, args):
    batches = [int(b) for b in args.batches.split(",")]
    rows = []
    fh = vio.load_fm().create()
    for rep in range(args.repeats):
        for n in (150, 2048):
            for B in batches:
                tables = [remove_tracks(n, 100 * s + n) for s in range(B)]
                gone = [np.random.RandomState(s).choice(t[0], size=n // 10, replace=False) for s, t in enumerate(tables)]
                after = {}
                for leg in (("batch", "host") if rep % 2 == 0 else ("host", "batch")):
                    wall, lib, parts = [], [], []
                    for t in range(args.warmup + args.reps):
                        for s in range(B):
                            fh.tracks_set(s, *tables[s])
                        t0 = time.perf_counter()
                        if leg == "batch":
                            res = fh.remove_batch(list(zip(range(B), gone)))
                        else:
                            for s in range(B):
                                fh.tracks_set(s, *host_erase(fh.tracks_get(s), gone[s]))
                        dt = 1e3 * (time.perf_counter() - t0)
                        if leg == "batch":
                            assert all(r["n_rows"] == n // 10 for r in res)
                        if t >= args.warmup:
                            wall.append(dt)
                            if leg == "batch":
                                parts.append(fh.timing())
                    after[leg] = [fh.tracks_get(s) for s in range(B)]
                    row = dict(repeat=rep, tracks=n, batch=B, leg=leg, call_ms=float(np.median(wall)), call_ms_min=float(np.min(wall)),
                               call_ms_max=float(np.max(wall)), us_per_slot=1e3 * float(np.median(wall)) / B)
                    if leg == "batch":
                        row["stages_ms"] = {k: float(np.median([p[k] for p in parts])) for k in ("host_ms", "kernel_ms", "readback_ms", "total_ms")}
                    rows.append(row)
                    print("repeat %d  tracks %4d  B %3d  leg %-5s  %9.3f ms (%.3f .. %.3f)  %9.1f us/slot  %s"
                          % (rep, n, B, leg, row["call_ms"], row["call_ms_min"], row["call_ms_max"], row["us_per_slot"],
                             "lib %(total_ms).3f  h %(host_ms).3f k %(kernel_ms).3f r %(readback_ms).3f" % row["stages_ms"] if leg == "batch" else ""), flush=True)
                same = all(a[k].tobytes() == b[k].tobytes() for a, b in zip(after["batch"], after["host"]) for k in a)
                rows.append(dict(repeat=rep, tracks=n, batch=B, same=bool(same)))
                print("repeat %d  tracks %4d  B %3d  the two legs leave identical tables: %s" % (rep, n, B, same), flush=True)
    fh.close()
    res = dict(bench="fm_remove", erased_fraction=0.1, reps=args.reps, warmup=args.warmup, repeats=args.repeats, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def measure_predict(vio, args):
    """--predict: predictPtsInNextFrame of B slots of 150 tracks (include/vio_fm_predict.h), B = 1 and 64
    (--batches): leg batch is one FmHandle.predict_batch, leg numpy per slot tracks_get and tests/fm_predict_reference.predict, the
    route without the call.  Both legs must give the same bytes (`same`)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fm_predict_reference as fp
    import predict_inputs as pi
    fh = vio.load_fm().create()
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        tabs = [pi.table(POINTS, WINDOW, seed=s)[0] for s in range(B)]
        poses = [pi.poses(s) for s in range(B)]
        for s in range(B):
            fh.tracks_set(s, *[tabs[s][k] for k in ("ids", "start", "depth", "flag", "off", "pts")])
        items = [(s, WINDOW, poses[s][0], poses[s][1], None) for s in range(B)]
        wall, parts, ref = [], [], []
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            out = fh.predict_batch(items)
            dt = 1e3 * (time.perf_counter() - t0)
            if r >= args.warmup:
                wall.append(dt)
                parts.append(fh.timing())
        for r in range(max(args.reps // 4, 2)):
            t0 = time.perf_counter()
            want = [fp.predict(fh.tracks_get(s), WINDOW, poses[s][0], poses[s][1], None) for s in range(B)]
            ref.append(1e3 * (time.perf_counter() - t0))
        same = all(o["ids"].tobytes() == w[0].tobytes() and o["pts_cam"].tobytes() == w[1].tobytes() for o, w in zip(out, want))
        row = dict(batch=B, tracks=POINTS, rows_per_slot=float(np.mean([o["n_rows"] for o in out])), call_ms=float(np.median(wall)),
                   us_per_slot=1e3 * float(np.median(wall)) / B,
                   stages_ms={k: float(np.median([p[k] for p in parts])) for k in ("host_ms", "kernel_ms", "readback_ms", "total_ms")},
                   numpy_ms=float(np.median(ref)), numpy_us_per_slot=1e3 * float(np.median(ref)) / B, same=bool(same))
        rows.append(row)
        print("B %3d  tracks %d  rows %.1f  call %8.3f ms  %8.2f us/slot  (lib %.3f  h %.3f k %.3f r %.3f)   numpy loop %8.3f ms  %8.2f us/slot   same bytes: %s"
              % (B, POINTS, row["rows_per_slot"], row["call_ms"], row["us_per_slot"], row["stages_ms"]["total_ms"], row["stages_ms"]["host_ms"],
                 row["stages_ms"]["kernel_ms"], row["stages_ms"]["readback_ms"], row["numpy_ms"], row["numpy_us_per_slot"], same), flush=True)
    fh.close()
    res = dict(bench="fm_predict", tracks=POINTS, reps=args.reps, warmup=args.warmup, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--remove", action="store_true")
    ap.add_argument("--batches", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.batches is None:
        args.batches = "1,64" if args.predict else "1,16,64" if args.remove else "1,16,64,256"
    vio = g.load_package()
    vio.load_hip()
    if args.predict:
        return measure_predict(vio, args)
    if args.remove:
        return measure_remove(vio, args)
    host = build_host_leg(os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc"))
    batches = [int(b) for b in args.batches.split(",")]
    frames = WINDOW + args.warmup + args.reps
    streams = [make_stream(s, frames) for s in range(max(batches))]
    # camera poses of a moving window (the synthetic trajectory), the same for every stream and frame
    w = vio.synth.make_window(8, seed=1)
    poses, ext = np.ascontiguousarray(w.poses, dtype=np.float64).reshape(11, 7), np.ascontiguousarray(w.ext, dtype=np.float64).reshape(7)
    R = [vio.synth.quat_to_rot(poses[k, 3:7]) for k in range(2)]
    ric, tic = vio.synth.quat_to_rot(ext[3:7]), ext[0:3]
    mats = [np.ascontiguousarray(m, dtype=np.float64) for m in (R[0] @ ric, poses[0, 0:3] + R[0] @ tic, R[1] @ ric, poses[1, 0:3] + R[1] @ tic)]
    rows = []
    for rep in range(args.repeats):
        for B in batches:
            last = {}
            for leg in (("batch", "loop") if rep % 2 == 0 else ("loop", "batch")):
                wall, lib, parts = [], [], {c: [] for c in CALLS}
                if leg == "batch":
                    fh = vio.load_fm().create()
                    fm = vio.BatchFeatureManager(fh, range(B))
                else:
                    hh = host.fmh_create(B)
                    assert hh, "vio_create failed"
                    key, ntr = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
                for t in range(frames):
                    fc = min(t, WINDOW)
                    if leg == "batch":
                        fr_in = [streams[s][t] for s in range(B)]
                        tm = {}
                        t0 = time.perf_counter()
                        res = fm.add_feature_frames(fr_in, [fc] * B)
                        tm["add"] = fh.timing()
                        wins = fm.windows([poses] * B, ext)
                        tm["export"] = fh.timing()
                        xs = [np.where(np.arange(len(x["inv_depth"])) % 50 == 0, -1.0, 1.0) * np.abs(x["inv_depth"]) for x in wins]
                        out = fm.set_depths(xs, remove_failures=True)
                        tm["set_depth"] = fh.timing()
                        if fc == WINDOW:
                            kinds = [vio.fm.BACK_SHIFT_DEPTH if r["keyframe"] else vio.fm.FRONT for r in res]
                            out = fm.slide(kinds, [fc] * B, *[[m] * B for m in mats])
                            tm["slide"] = fh.timing()
                        dt = 1e3 * (time.perf_counter() - t0)
                        last[leg] = ([r["keyframe"] for r in res], [r["n_tracks"] for r in out])
                        if t >= WINDOW + args.warmup:
                            lib.append(sum(v["total_ms"] for v in tm.values()))
                            for c, v in tm.items():
                                parts[c].append(v)
                    else:
                        ids = np.ascontiguousarray(np.stack([streams[s][t][0] for s in range(B)]), dtype=np.int32)
                        pts = np.ascontiguousarray(np.stack([streams[s][t][1] for s in range(B)]))
                        dt = host.fmh_frame(hh, fc, POINTS, ids.ctypes.data, pts.ctypes.data, poses.ctypes.data, ext.ctypes.data,
                                            *[m.ctypes.data for m in mats], key.ctypes.data, ntr.ctypes.data)
                        assert dt >= 0, "vio_triangulate failed"
                        last[leg] = (key.tolist(), ntr.tolist())
                    if t >= WINDOW + args.warmup:
                        wall.append(dt)
                if leg == "batch":
                    fh.close()
                else:
                    host.fmh_destroy(hh)
                row = dict(repeat=rep, batch=B, leg=leg, frame_ms=float(np.median(wall)), frame_ms_min=float(np.min(wall)),
                           frame_ms_max=float(np.max(wall)), us_per_stream=1e3 * float(np.median(wall)) / B,
                           tracks_per_stream=float(np.mean(last[leg][1])))
                if leg == "batch":
                    row["lib_ms"] = float(np.median(lib))
                    row["stages_ms"] = {c: {k: float(np.median([p[k] for p in parts[c]])) for k in ("host_ms", "kernel_ms", "readback_ms", "total_ms")}
                                        for c in CALLS if parts[c]}
                rows.append(row)
                print("repeat %d  B %3d  leg %-5s  frame %9.3f ms (%.3f .. %.3f)  %9.1f us/stream  tracks %.1f  %s"
                      % (rep, B, leg, row["frame_ms"], row["frame_ms_min"], row["frame_ms_max"], row["us_per_stream"], row["tracks_per_stream"],
                         ("lib %.3f  " % row["lib_ms"] + "  ".join("%s h %.3f k %.3f r %.3f" % (c, v["host_ms"], v["kernel_ms"], v["readback_ms"])
                                                                    for c, v in row["stages_ms"].items())) if leg == "batch" else ""), flush=True)
            same = last["batch"] == last["loop"]
            rows.append(dict(repeat=rep, batch=B, same=bool(same), keyframes=int(sum(last["batch"][0]))))
            print("repeat %d  B %3d  decisions and track counts of the two legs identical: %s" % (rep, B, same), flush=True)
    res = dict(bench="fm_batch", points=POINTS, reps=args.reps, warmup=args.warmup, repeats=args.repeats, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
