"""One JSON line: IMU pre-integration on the GPU (include/vio_imu.h, vio_imu_propagate on samples already loaded) against the host's
vio_preintegrate (one C call per interval, arguments prepared beforehand), median of --reps after --warmup, for
  window        one window: 10 intervals x 20 samples
  batch_256     256 windows: 2 560 intervals x 20 samples, one launch
  long_2000     one interval of 2 000 samples, re-propagated
GPU figures: the whole call (wall clock: bias upload, k_imu_propagate, read-back of the records, the finiteness scan) and the kernel
alone (HIP events).  Host figure: the sum of the vio_preintegrate calls (wall clock)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

NOISE = dict(acc_n=0.08, gyr_n=0.004, acc_w=2.0e-4, gyr_w=2.0e-6)


def intervals(n, S, seed):
    rng = np.random.RandomState(seed)
    return [dict(acc0=rng.normal(0, 1, 3) + [0, 0, 9.81], gyr0=rng.normal(0, 0.5, 3), dt=list(rng.uniform(0.0049, 0.0051, S)),
                 acc=list(rng.normal(0, 1, (S, 3)) + [0, 0, 9.81]), gyr=list(rng.normal(0, 0.5, (S, 3)))) for _ in range(n)]


def host_time(hip, ivs, ba, bg, reps, warmup):
    fn = hip.fn["preintegrate"] if "preintegrate" in hip.fn else hip.raw("preintegrate")
    fn.restype = C.c_int
    out = g.load_package().VioPreint()
    args = []
    keep = []
    for k, iv in enumerate(ivs):
        a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (iv["acc0"], iv["gyr0"], ba[k], bg[k], iv["dt"], iv["acc"], iv["gyr"])]
        keep.append(a)
        ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
        args.append([ptr(x) for x in a[:4]] + [C.c_int32(a[4].size)] + [ptr(x) for x in a[4:]]
                    + [C.c_double(NOISE[k2]) for k2 in ("acc_n", "gyr_n", "acc_w", "gyr_w")] + [C.byref(out)])
    ts = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        for a in args:
            fn(*a)
        if r >= warmup:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def gpu_time(imu, ivs, ba, bg, reps, warmup, which=None):
    h = imu.create()
    h.load(ivs, NOISE)
    rows = []
    for r in range(warmup + reps):
        h.propagate(ba + 1e-6 * r, bg, which=which)         # a new bias every call: a re-propagation
        if r >= warmup:
            rows.append(h.timing())
    return {k: float(np.median([t[k] for t in rows])) for k in rows[0]}


def case(vio, hip, imu, name, n, S, reps, warmup, seed):
    ivs = intervals(n, S, seed)
    rng = np.random.RandomState(seed + 1)
    ba, bg = rng.normal(0, 0.05, (n, 3)), rng.normal(0, 0.005, (n, 3))
    gt = gpu_time(imu, ivs, ba, bg, reps, warmup)
    ht = host_time(hip, ivs, ba, bg, reps, warmup)
    return {"case": name, "intervals": n, "samples_per_interval": S, "gpu_call_us": round(gt["total_ms"] * 1e3, 2),
            "gpu_kernel_us": round(gt["kernel_ms"] * 1e3, 2), "gpu_host_us": round(gt["host_ms"] * 1e3, 2),
            "host_preintegrate_us": round(ht * 1e3, 2), "host_over_gpu_call": round(ht / gt["total_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    vio = g.load_package()
    hip = vio.load_hip()
    imu = vio.load_imu()
    res = [case(vio, hip, imu, "window", 10, 20, args.reps, args.warmup, 1),
           case(vio, hip, imu, "batch_256", 2560, 20, args.reps, args.warmup, 2),
           case(vio, hip, imu, "long_2000", 1, 2000, args.reps, args.warmup, 3)]
    print(json.dumps({"metric": "imu_propagate", "reps": args.reps, "cases": res}))


if __name__ == "__main__":
    main()
