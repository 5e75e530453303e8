"""Two timings of include/vio_est_init.h's hand-over.

  leg apply   vio_est_init_apply_batch over B full slots (20 IMU samples per interval) in one call, against the detour it replaces:
              per slot state_get, visualInitialAlign's state change in numpy on the host, state_set (the slot's samples travel down
              and up again, and every call waits).  Median of --reps after --warmup, per B, with the library's own split
              (vio_est_timing) of the batched call.
  leg round   batch_stream.initialize_batched over --drivers synthetic drivers that initialise at the first try (the alignment library
              on visual_trajectory's stand-in), without and with initialize=dict(state=): the second feeds every slot from its first
              sample (eleven imu_batch and eleven image_batch calls for the group) and ends in one init_apply_batch.  Wall time of the
              whole round, constructors excluded; --repeats runs with the order alternating.

    python tools/bench_est_init.py [--batches 1,64,256] [--reps 20] [--warmup 3] [--drivers 64] [--repeats 2] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as g  # noqa: E402
from bench_est_batch import WINDOW, make_intervals, seed_state  # noqa: E402


def host_apply(vio, s, poses, sb, grav, rot):
    """visualInitialAlign's state change on a downloaded state, as a caller without the call writes it."""
    s = dict(s)
    q = poses[:, 3:7] / np.linalg.norm(poses[:, 3:7], axis=1)[:, None]
    s["Ps"], s["Rs"] = poses[:, 0:3].copy(), np.array([vio.synth.quat_to_rot(x).reshape(9) for x in q])
    s["Vs"], s["Bas"], s["Bgs"] = sb[:, 0:3].copy(), sb[:, 3:6].copy(), sb[:, 6:9].copy()
    s["lin_bias"] = np.concatenate([np.zeros((11, 3)), sb[:, 6:9]], axis=1)
    s["g"] = rot @ grav
    return s


def leg_apply(vio, batches, reps, warmup):
    w = vio.synth.make_window(8, seed=1)
    seed = seed_state(vio, w, make_intervals(np.random.RandomState(0), WINDOW))
    poses, sb = w.poses.copy(), w.speed_bias.copy()
    sb[:, 3:6], sb[:, 6:9] = 0.0, (0.003, -0.002, 0.001)
    th = np.radians(20.0)
    rot = np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])
    grav = rot.T @ np.array([0.0, 0.0, 9.81])
    rows = []
    eh = vio.load_est().create()
    eh.set_config(w.ext[0:3], w.ext[3:7], (0, 0, 9.81))
    for B in batches:
        for s in range(B):
            eh.state_set(s, seed)
        items = [(s, poses, sb, grav, rot, True) for s in range(B)]
        batch, loop, parts = [], [], []
        for t in range(warmup + reps):
            t0 = time.perf_counter()
            res = eh.init_apply_batch(items)
            t1 = time.perf_counter()
            parts.append(eh.timing())
            assert all(r["status"] == 0 for r in res)
            t2 = time.perf_counter()
            for s in range(B):
                eh.state_set(s, host_apply(vio, eh.state_get(s), poses, sb, grav, rot))
            t3 = time.perf_counter()
            if t >= warmup:
                batch.append(1e3 * (t1 - t0))
                loop.append(1e3 * (t3 - t2))
        row = dict(leg="apply", batch=B, batch_ms=float(np.median(batch)), batch_ms_min=float(np.min(batch)), batch_ms_max=float(np.max(batch)),
                   detour_ms=float(np.median(loop)), detour_ms_min=float(np.min(loop)), detour_ms_max=float(np.max(loop)),
                   lib={k: float(np.median([p[k] for p in parts[warmup:]])) for k in ("host_ms", "kernel_ms", "readback_ms", "total_ms")})
        rows.append(row)
        print(json.dumps(row), flush=True)
    eh.close()
    return rows


def leg_round(vio, n, repeats):
    from vio_amd import batch_stream, stream as vs
    hip = vio.load_hip()
    streams = [vs.SyntheticStream(n_frames=12, seed=s) for s in range(n)]
    est = vio.load_est().create()
    rows = []
    for rep in range(repeats):
        for with_state in ((False, True) if rep % 2 == 0 else (True, False)):
            ds, sh = [], None
            for k, st in enumerate(streams):
                init = dict(scale=3.7, state=(est, k)) if with_state else dict(scale=3.7)
                ds.append(vs.StreamDriver(hip, st, seed=2, initialize=init, **(dict(ctx_kwargs=dict(stream=sh)) if sh is not None else {})))
                sh = ds[0].ctx.get_stream()
            t0 = time.perf_counter()
            rounds = batch_stream.initialize_batched(ds)
            ms = 1e3 * (time.perf_counter() - t0)
            assert all(d.initialized for d in ds)
            row = dict(leg="round", repeat=rep, drivers=n, state=with_state, rounds=rounds, round_ms=ms)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ds
    est.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--drivers", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    vio.load_hip()
    rows = leg_apply(vio, [int(b) for b in args.batches.split(",")], args.reps, args.warmup)
    if args.drivers > 0:
        rows += leg_round(vio, args.drivers, args.repeats)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_est_init.py", reps=args.reps, warmup=args.warmup, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
