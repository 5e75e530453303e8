"""A frame of the Estimator state for B streams on full 11-frame windows with 20 IMU samples per interval: the window's states and
ten pre-integrations, the re-anchoring after the solve with failureDetection, the slide, and processIMU over the next interval.

  leg batch  est.BatchEstimatorState over B slots of one EstHandle: four batched calls per frame (windows, update, slide, process_imu),
             each one wait
  leg loop   the same work the way StreamDriver does it without state=, one stream after the other in Python: window_arrays' copies,
             stream.anchor_gauge, slide_window_old's four matrices and shifts (slide_window_new's merge and its synth.preintegrate of
             the merged interval on the frames that are no keyframes), and take_next_frame's closed-form prediction from
             synth.preintegrate of the new interval (a StreamDriver on a SyntheticStream reads that record from the stream; a live
             stream has to compute it, as here)

Per leg and B: the wall time of a frame, the median of --reps frames after --warmup, with the least and the most; leg batch also as
lib_ms, the sum of the library's own whole-call times (vio_est_timing), with each call's stage split.  Every fourth frame slides the
new way.  The "solve" between windows and update is a fixed gauge drift (a yaw and a shift) applied on the host, outside the timed
calls of both legs.  The two legs of a B run back to back, and --repeats runs the whole measurement again with the order of the legs
alternating, for the spread.

    python tools/bench_est_batch.py [--batches 1,64,256] [--reps 20] [--warmup 3] [--repeats 3] [--out profiles/NAME.json]
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

SAMPLES, WINDOW = 20, 10
CALLS = ("windows", "update", "slide", "process_imu")


def make_intervals(rng, n):
    """n consecutive intervals of one sample stream: each starts from the sample the one before ended with (acc_0 / gyr_0)."""
    out, a0, g0 = [], rng.normal(0, 1, 3) + [0, 0, 9.81], rng.uniform(-0.2, 0.2, 3)
    for _ in range(n):
        acc, gyr = rng.normal(0, 1, (SAMPLES, 3)) + [0, 0, 9.81], rng.uniform(-0.2, 0.2, (SAMPLES, 3))
        out.append(dict(acc0=a0, gyr0=g0, dt=[0.005] * SAMPLES, acc=list(acc), gyr=list(gyr)))
        a0, g0 = acc[-1], gyr[-1]
    return out


def seed_state(vio, w, ivs):
    """A full window as StreamDriver(state=) seeds it: the synthetic window's states, interval j + 1 = ivs[j]."""
    R = np.array([vio.synth.quat_to_rot(q).reshape(9) for q in w.poses[:, 3:7]])
    first = np.zeros((11, 6))
    for j, iv in enumerate(ivs):
        first[j + 1, 0:3], first[j + 1, 3:6] = iv["acc0"], iv["gyr0"]
    cat = lambda k, n: np.concatenate([np.asarray(iv[k], dtype=np.float64).reshape(-1, n) for iv in ivs])
    off = np.concatenate([[0, 0], np.cumsum([len(iv["dt"]) for iv in ivs])]).astype(np.int64)
    return dict(frame_count=WINDOW, first_imu=1, failure_occur=0, exists=np.ones(11, dtype=np.int32), Ps=w.poses[:, 0:3], Rs=R,
                Vs=w.speed_bias[:, 0:3], Bas=w.speed_bias[:, 3:6], Bgs=w.speed_bias[:, 6:9], Headers=np.arange(11.0), tic=w.ext[0:3],
                ric=vio.synth.quat_to_rot(w.ext[3:7]).reshape(9), g=np.array([0, 0, 9.81]), acc_0=cat("acc", 3)[-1], gyr_0=cat("gyr", 3)[-1],
                first=first, lin_bias=np.zeros((11, 6)), last_R=R[10], last_P=w.poses[10, 0:3], last_R0=R[0], last_P0=w.poses[0, 0:3], off=off,
                dt=cat("dt", 1).reshape(-1), acc=cat("acc", 3), gyr=cat("gyr", 3))


def drift(vio, poses, sb, G):
    """What a solve hands back: the window moved by the gauge drift G (a yaw) and a shift."""
    out = poses.copy()
    for i in range(11):
        out[i, 0:3] = G @ poses[i, 0:3] + [0.3, -0.2, 0.1]
        out[i, 3:7] = vio.synth.rot_to_quat(G @ vio.synth.quat_to_rot(poses[i, 3:7]))
    return out, sb.copy()


class LoopStream:
    """One stream's window the way StreamDriver keeps it without state=: numpy arrays and Python lists."""

    def __init__(self, vio, w, ivs):
        self.vio, self.poses, self.sb, self.ext = vio, w.poses.copy(), w.speed_bias.copy(), w.ext.copy()
        self.intervals = [dict(iv) for iv in ivs]
        self.preint = [vio.synth.preintegrate(iv["acc0"], iv["gyr0"], np.zeros(3), np.zeros(3), iv["dt"], iv["acc"], iv["gyr"]) for iv in ivs]

    def window(self):
        return self.poses.copy(), self.sb.copy(), self.ext.copy(), list(self.preint)

    def update(self, before, poses, sb):
        self.poses, self.sb = self.vio.stream.anchor_gauge(before, poses, sb)

    def slide(self, old):
        synth = self.vio.synth
        if old:
            R0, R1 = synth.quat_to_rot(self.poses[0, 3:7]), synth.quat_to_rot(self.poses[1, 3:7])
            ric, tic = synth.quat_to_rot(self.ext[3:7]), self.ext[0:3]
            mats = (R0 @ ric, self.poses[0, 0:3] + R0 @ tic, R1 @ ric, self.poses[1, 0:3] + R1 @ tic)
            self.intervals.pop(0)
            self.preint.pop(0)
            self.poses[:-1], self.sb[:-1] = self.poses[1:].copy(), self.sb[1:].copy()
            return mats
        a, b = self.intervals[WINDOW - 2], self.intervals[WINDOW - 1]
        merged = dict(acc0=a["acc0"], gyr0=a["gyr0"], dt=a["dt"] + b["dt"], acc=a["acc"] + b["acc"], gyr=a["gyr"] + b["gyr"])
        self.intervals[WINDOW - 2:] = [merged]
        self.preint[WINDOW - 2:] = [synth.preintegrate(merged["acc0"], merged["gyr0"], np.zeros(3), np.zeros(3), merged["dt"], merged["acc"], merged["gyr"])]
        self.poses[WINDOW - 1], self.sb[WINDOW - 1] = self.poses[WINDOW].copy(), self.sb[WINDOW].copy()
        return None

    def next_frame(self, iv):
        synth = self.vio.synth
        pre = synth.preintegrate(iv["acc0"], iv["gyr0"], np.zeros(3), np.zeros(3), iv["dt"], iv["acc"], iv["gyr"])
        self.intervals.append(iv)
        self.preint.append(pre)
        dt, i = pre["sum_dt"], WINDOW - 1
        Ri, gv = synth.quat_to_rot(self.poses[i, 3:7]), np.array([0.0, 0.0, 9.81])
        Pi, Vi = self.poses[i, 0:3], self.sb[i, 0:3]
        self.poses[WINDOW, 0:3] = Pi + Vi * dt - 0.5 * gv * dt * dt + Ri @ pre["delta_p"]
        self.poses[WINDOW, 3:7] = synth.quat_mul(self.poses[i, 3:7], pre["delta_q"])
        self.sb[WINDOW, 0:3] = Vi - gv * dt + Ri @ pre["delta_v"]
        self.sb[WINDOW, 3:9] = self.sb[i, 3:9]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    vio.load_hip()
    batches = [int(b) for b in args.batches.split(",")]
    frames = args.warmup + args.reps
    w = vio.synth.make_window(8, seed=1)
    rng = np.random.RandomState(0)
    ivs = make_intervals(rng, WINDOW + frames)
    ivs0, nxt = ivs[:WINDOW], ivs[WINDOW:]
    th = np.radians(3.0)
    G = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    rows = []
    for rep in range(args.repeats):
        for B in batches:
            for leg in (("batch", "loop") if rep % 2 == 0 else ("loop", "batch")):
                wall, lib, parts, failures = [], [], {c: [] for c in CALLS}, 0
                if leg == "batch":
                    eh = vio.load_est().create()
                    eh.set_config(w.ext[0:3], w.ext[3:7], (0, 0, 9.81))
                    seed = seed_state(vio, w, ivs0)
                    for s in range(B):
                        eh.state_set(s, seed)
                    est = vio.BatchEstimatorState(eh, range(B))
                else:
                    streams = [LoopStream(vio, w, ivs0) for _ in range(B)]
                for t in range(frames):
                    old = t % 4 != 3
                    iv = nxt[t]
                    tm = {}
                    if leg == "batch":
                        t0 = time.perf_counter()
                        wins = est.windows()
                        tm["windows"] = eh.timing()
                        dt = time.perf_counter() - t0
                        solved = [drift(vio, x["poses"], x["speed_bias"], G) for x in wins]
                        t0 = time.perf_counter()
                        res = est.update([s[0] for s in solved], [s[1] for s in solved], [x["ext"] for x in wins])
                        tm["update"] = eh.timing()
                        est.slide([vio.est.MARG_OLD if old else vio.est.MARG_SECOND_NEW] * B)
                        tm["slide"] = eh.timing()
                        est.process_imu([iv] * B)
                        tm["process_imu"] = eh.timing()
                        dt += time.perf_counter() - t0
                        failures += sum(r["failure"] for r in res)
                    else:
                        t0 = time.perf_counter()
                        wins = [s.window() for s in streams]
                        dt = time.perf_counter() - t0
                        solved = [drift(vio, x[0], x[1], G) for x in wins]
                        t0 = time.perf_counter()
                        for s, x, (p, b) in zip(streams, wins, solved):
                            s.update(x[0], p, b)
                            s.slide(old)
                            s.next_frame(iv)
                        dt += time.perf_counter() - t0
                    if t >= args.warmup:
                        wall.append(1e3 * dt)
                        if leg == "batch":
                            lib.append(sum(v["total_ms"] for v in tm.values()))
                            for c, v in tm.items():
                                parts[c].append(v)
                if leg == "batch":
                    eh.close()
                row = dict(repeat=rep, batch=B, leg=leg, frame_ms=float(np.median(wall)), frame_ms_min=float(np.min(wall)),
                           frame_ms_max=float(np.max(wall)), us_per_stream=1e3 * float(np.median(wall)) / B)
                if leg == "batch":
                    row.update(lib_ms=float(np.median(lib)), failures=int(failures),
                               calls={c: {k: float(np.median([v[k] for v in parts[c]])) for k in ("host_ms", "kernel_ms", "readback_ms", "total_ms")} for c in CALLS})
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bench_est_batch.py", samples_per_interval=SAMPLES, reps=args.reps, warmup=args.warmup, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
