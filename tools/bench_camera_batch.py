"""The camera model library (libvio_camera_hip.so): rejectWithF and undistortedPoints of B streams of n = 150 matched points (MAX_CNT)
through each of the four camera models, B = 1, 16, 64, 256, and PINHOLE beside libvio_reject_hip on the same inputs.  Per call: host
packing + upload, the kernel (HIP events through vio_camera_timing / vio_reject_timing) and the whole call, the median of --reps
calls after --warmup.

    python tools/bench_camera_batch.py [--out profiles/NAME.json]
    python tools/bench_camera_batch.py --project [--batches 1,64] [--out profiles/NAME.json]      # spaceToPlane (measure_project)

The pairs are synthetic two-view scenes (tests/camera_reference.two_view_scene: landmarks through the model from two poses, 0.1 px of
noise, 20 % planted outliers), scene k of a batch drawn with seed k mod 8; undistort matches every point against the other frame's
150 points.  A last row per batch mixes the four models in one call, item k on model k mod 4.
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


def timed(handle, pairs, und, warmup, reps):
    tr, tu = [], []
    for r in range(warmup + reps):
        out = handle.reject_batch(pairs)
        t1 = handle.timing()
        handle.undistort_batch(und)
        t2 = handle.timing()
        if r >= warmup:
            tr.append(t1)
            tu.append(t2)
    return median(tr), median(tu), out


def measure_project(vio, args):
    """--project: spaceToPlane of B items of N points (include/vio_camera_project.h), B = 1 and 64 (--batches),
    per model and mixed: leg batch is one CameraHandle.project_batch, leg numpy a loop over tests/camera_project_reference.project, the
    route without the call.  Both legs must give the same bytes (`same`)."""
    import time

    import camera_project_reference as cp
    import camera_reference as cr
    models = [("PINHOLE", cr.EUROC), ("KANNALA_BRANDT", cr.KB_FOUR), ("MEI", cr.MEI), ("SCARAMUZZA", cr.SCARAMUZZA)]
    cams = [cr.Camera(**p) for _, p in models]
    invs = [cp.fit_inv_poly(c) if c.model == cr.MODEL_SCARAMUZZA else None for c in cams]
    ch = vio.load_camera().create()
    for slot, (_, params) in enumerate(models):
        ch.set_camera(slot=slot, **params)
        if invs[slot] is not None:
            ch.set_inv_poly(slot, invs[slot])
    rng = np.random.RandomState(0)
    th, ph = rng.uniform(0.0, 0.45, (8, N)), rng.uniform(-np.pi, np.pi, (8, N))
    pts = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=2) * rng.uniform(0.5, 25.0, (8, N, 1))
    rows = []
    for B in [int(b) for b in (args.batches or "1,64").split(",")]:
        for name, slot_of in [(n, (lambda k, s=s: s)) for s, (n, _) in enumerate(models)] + [("mixed", lambda k: k % 4)]:
            items = [dict(points=pts[k % 8], slot=slot_of(k)) for k in range(B)]
            wall, parts, ref = [], [], []
            for r in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                out = ch.project_batch(items)
                dt = 1e3 * (time.perf_counter() - t0)
                if r >= args.warmup:
                    wall.append(dt)
                    parts.append(ch.timing())
            for r in range(max(args.reps // 4, 2)):
                t0 = time.perf_counter()
                want = [cp.project(cams[it["slot"]], it["points"], invs[it["slot"]]) for it in items]
                ref.append(1e3 * (time.perf_counter() - t0))
            same = all(o["pixels"].tobytes() == w[0].tobytes() and o["flags"].tobytes() == w[1].tobytes() for o, w in zip(out, want))
            row = dict(batch=B, n=N, model=name, call_ms=float(np.median(wall)), us_per_item=1e3 * float(np.median(wall)) / B, stages_ms=median(parts),
                       numpy_ms=float(np.median(ref)), numpy_us_per_item=1e3 * float(np.median(ref)) / B, same=bool(same))
            rows.append(row)
            print("B %3d  %-14s  call %8.3f ms  %8.2f us/item  (upload %.3f kernel %.3f total %.3f)   numpy loop %8.3f ms  %8.2f us/item   same bytes: %s"
                  % (B, name, row["call_ms"], row["us_per_item"], row["stages_ms"]["upload_ms"], row["stages_ms"]["kernel_ms"], row["stages_ms"]["total_ms"],
                     row["numpy_ms"], row["numpy_us_per_item"], same), flush=True)
    ch.close()
    res = dict(bench="camera_project", n=N, reps=args.reps, warmup=args.warmup, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--project", action="store_true")
    ap.add_argument("--batches", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    if args.project:
        return measure_project(vio, args)
    args.batches = args.batches or "1,16,64,256"
    import camera_reference as cr
    import reject_reference as rr
    models = [("PINHOLE", cr.EUROC), ("KANNALA_BRANDT", cr.KB_FOUR), ("MEI", cr.MEI), ("SCARAMUZZA", cr.SCARAMUZZA)]
    ch = vio.load_camera().create()
    rh = vio.load_reject().create()
    rh.set_camera(**rr.EUROC)
    rh.set_config()
    ch.set_config()
    ids = np.arange(N, dtype=np.int64)
    data = []
    for slot, (name, params) in enumerate(models):
        ch.set_camera(slot=slot, **params)
        cam = cr.Camera(**params)
        scenes = [cr.two_view_scene(cam, n=N, seed=s) for s in range(8)]
        prev = [cr.un_points(cam, s[0])[::-1].copy() for s in scenes]
        data.append((scenes, prev))

    def items(B, slot_of):
        pairs, und = [], []
        for k in range(B):
            s = slot_of(k)
            scenes, prev = data[s]
            pairs.append(dict(cur_pts=scenes[k % 8][0], forw_pts=scenes[k % 8][1], pair=k, slot=s))
            und.append(dict(pts=scenes[k % 8][1], ids=ids, prev_ids=ids[::-1].copy(), prev_un_pts=prev[k % 8], dt=0.05, slot=s))
        return pairs, und

    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        cases = [(name, (lambda k, s=slot: s)) for slot, (name, _) in enumerate(models)] + [("mixed", lambda k: k % 4)]
        for name, slot_of in cases:
            pairs, und = items(B, slot_of)
            mr, mu, out = timed(ch, pairs, und, args.warmup, args.reps)
            row = dict(batch=B, n=N, model=name, library="camera", reject=mr, undistort=mu, reject_kernel_us_per_pair=1e3 * mr["kernel_ms"] / B,
                       undistort_kernel_us_per_item=1e3 * mu["kernel_ms"] / B, inliers_per_pair=float(np.mean([o["n_inliers"] for o in out])),
                       ok_pairs=sum(o["status"] == 0 for o in out))
            rows.append(row)
            if name == "PINHOLE":
                rr_, ru, out2 = timed(rh, pairs, und, args.warmup, args.reps)
                same = all(a["mask"].tobytes() == b["mask"].tobytes() and a["hyp"] == b["hyp"] for a, b in zip(out, out2))
                rows.append(dict(batch=B, n=N, model=name, library="reject", reject=rr_, undistort=ru, reject_kernel_us_per_pair=1e3 * rr_["kernel_ms"] / B,
                                 undistort_kernel_us_per_item=1e3 * ru["kernel_ms"] / B, same_masks_as_camera=bool(same)))
        for row in rows[-6:]:
            print("B %3d  %-14s %-6s  reject: upload %7.3f ms  kernel %8.3f ms  total %8.3f ms  %8.2f us/pair   undistort: kernel %6.3f ms  total %7.3f ms"
                  % (row["batch"], row["model"], row["library"], row["reject"]["upload_ms"], row["reject"]["kernel_ms"], row["reject"]["total_ms"],
                     row["reject_kernel_us_per_pair"], row["undistort"]["kernel_ms"], row["undistort"]["total_ms"]))
    res = dict(bench="camera_batch", n=N, hypotheses=vio.reject.DEFAULT_HYPOTHESES, reps=args.reps, rows=rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ch.close()
    rh.close()


if __name__ == "__main__":
    main()
