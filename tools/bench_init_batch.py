"""Batched visual-inertial alignment (include/vio_init.h) on the GPU: one JSON line.

For B = 1, 16, 64, 256, 1024 windows of F = 11 and F = 32 frames (SyntheticStream windows, every frame a keyframe, the SfM stand-in at
scale 3.7 with 1 mrad / 1 mm of noise), the median over --reps calls of:
  gyro_ms_per_window       vio_init_gyro_bias_batch, the whole call / B
  propagate_ms_per_window  vio_imu_propagate of the B (F-1) intervals at the new biases / B
  align_ms_per_window      vio_init_align_batch / B
  initialize_ms_per_window InitHandle.initialize_batch (gyro, imu.load, propagate, align, Python packing included) / B
  gyro_kernel_ms, align_kernel_ms   the kernels' HIP-event times per call
and python_restatement_ms_per_window: tests/init_reference.py's align() on one window, a Python figure (scalar numpy), not a CPU
baseline.

    python tools/bench_init_batch.py [--reps 5] [--batches 1,16,64,256,1024] [--frames 11,32]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64,256,1024")
    ap.add_argument("--frames", default="11,32")
    a = ap.parse_args()
    import __graft_entry__ as g
    vio = g.load_package()
    vio.load_hip()
    from vio_amd import stream as vs
    ih = vio.load_init().create()
    imu = vio.load_imu().create()
    tic, G = vio.synth.T_IC, vio.synth.G_NORM
    out = {"tool": "bench_init_batch", "reps": a.reps, "rows": []}
    for F in [int(v) for v in a.frames.split(",")]:
        st = vs.SyntheticStream(n_frames=F + 8, landmarks_per_frame=1, seed=0)
        base = []
        for k in range(8):
            fr = list(range(k, k + F))
            R, T = vs.visual_trajectory(st, fr, 0, 3.7, rot_noise=1e-3, pos_noise=1e-3, seed=k)
            base.append((dict(R=R, T=T, pre=[st.preint[f] for f in fr[:-1]]), [st.imu[f] for f in fr[:-1]]))
        for B in [int(v) for v in a.batches.split(",")]:
            items = [base[i % 8][0] for i in range(B)]
            ivs = [base[i % 8][1] for i in range(B)]
            flat = [iv for w in ivs for iv in w]
            rec = {k: [] for k in ("gyro", "gyro_k", "prop", "align", "align_k", "init")}
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                bg = ih.gyro_bias_batch(items)
                t1 = time.perf_counter()
                tg = ih.timing()
                imu.load(flat)
                t2 = time.perf_counter()
                recs = imu.propagate(np.zeros(3), np.repeat(bg, F - 1, axis=0))
                t3 = time.perf_counter()
                items2 = [dict(it, pre=recs[i * (F - 1):(i + 1) * (F - 1)]) for i, it in enumerate(items)]
                t4 = time.perf_counter()
                res = ih.align_batch(items2, tic, G, bg)
                t5 = time.perf_counter()
                ta = ih.timing()
                t6 = time.perf_counter()
                res2 = ih.initialize_batch(items, ivs, imu, tic, G)
                t7 = time.perf_counter()
                if rep == 0:
                    continue            # warm-up
                rec["gyro"].append((t1 - t0) * 1e3 / B)
                rec["gyro_k"].append(tg["kernel_ms"])
                rec["prop"].append((t3 - t2) * 1e3 / B)
                rec["align"].append((t5 - t4) * 1e3 / B)
                rec["align_k"].append(ta["kernel_ms"])
                rec["init"].append((t7 - t6) * 1e3 / B)
            ok = sum(r["status"] == 0 for r in res2)
            med = {k: float(np.median(v)) for k, v in rec.items()}
            out["rows"].append(dict(F=F, B=B, ok_windows=ok, gyro_ms_per_window=med["gyro"], propagate_ms_per_window=med["prop"],
                                    align_ms_per_window=med["align"], initialize_ms_per_window=med["init"],
                                    gyro_kernel_ms=med["gyro_k"], align_kernel_ms=med["align_k"]))
        # the numpy restatement (oracle LDLT), one window at a time
        import init_reference as ir
        orc = vio.VioLib(os.path.join(ROOT, "oracle", "liboracle.so"), "vioo_")
        ts = []
        for it, _ in base[:4]:
            t0 = time.perf_counter()
            ir.align(orc, it, tic, G, np.zeros(3))
            ts.append((time.perf_counter() - t0) * 1e3)
        out["python_restatement_ms_per_window_F%d" % F] = float(np.median(ts))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
