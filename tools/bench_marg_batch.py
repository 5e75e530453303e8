"""Batched marginalisation (include/vio_marg.h) against sequential vio_marginalize, in one process; prints one JSON line.

Cases: B = 1, 8, 64, 256 windows of the per_frame_small size, taken from running stream drivers in their steady state (the window
of frame 12, with the prior the stream's earlier marginalisations left: the live-row counts of a stream), at two track densities,
and one window of 20 000 landmarks.  Per case: the batched call's ms per window (median of --reps calls), the same windows through
vio_marginalize on contexts loaded with them (each call timed alone; the loads are not timed), the two kernels' times (HIP events),
the host pack + upload, and the live-row counts.

    python tools/bench_marg_batch.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    vio = g.load_package()
    hip = vio.load_hip()
    mh = vio.load_marg().create()
    from vio_amd import stream as vs
    base = {}
    for lpf in (30, 60):             # 8 distinct steady-state windows per density, each with the prior its stream left
        ws = []
        for s in range(8):
            d = vs.StreamDriver(hip, vs.SyntheticStream(n_frames=14, landmarks_per_frame=lpf, seed=2000 + 10 * lpf + s))
            for _ in range(12):
                d.step()
            d.ensure_depths()
            w, _ = d.window_arrays()
            ws.append(w)
            d.ctx.close()
        base[lpf] = ws
    big = vio.synth.make_window(20000, seed=4242)
    c = hip.context()
    c.load(big)
    big.prior = c.marginalize(vio.MARG_OLD)     # (a window's own prior: 20 000 landmarks is not a stream's size)
    c.close()
    cases = [("n%d_B%d" % (len(base[lpf][0].inv_depth), B), [base[lpf][i % 8] for i in range(B)]) for lpf in (30, 60)
             for B in (1, 8, 64, 256)]
    cases.append(("n20000_B1", [big]))
    out = {"metric": "marg_batch", "unit": "ms per window", "cases": {}}
    for name, ws in cases:
        B = len(ws)
        jobs = [(vio.MARG_OLD, w, w.prior) for w in ws]
        mh.compute_batch(jobs)                      # warm-up (allocations)
        tb, tk = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            mh.compute_batch(jobs)
            tb.append((time.perf_counter() - t0) * 1e3)
            tk.append(mh.timing())
        live = sorted({mh.live_rows(i) for i in range(B)})
        # sequential vio_marginalize: one context per distinct window, loaded once; every window's call timed
        ctxs = {}
        ts = []
        for rep in range(2):
            for w in ws:
                c = ctxs.get(id(w))
                if c is None:
                    c = ctxs[id(w)] = hip.context()
                c.load(w)
                t0 = time.perf_counter()
                c.marginalize(vio.MARG_OLD)
                if rep:
                    ts.append((time.perf_counter() - t0) * 1e3)
        for c in ctxs.values():
            c.close()
        k = np.median(np.array(tk), axis=0)
        batched = float(np.median(tb)) / B
        seq = float(np.median(ts))
        out["cases"][name] = {"windows": B, "batched_ms_per_window": round(batched, 4), "sequential_ms_per_window": round(seq, 4),
                              "speedup": round(seq / batched, 2), "host_pack_upload_ms": round(float(k[0]), 4),
                              "k_marg_build_ms": round(float(k[1]), 4), "k_marg_tail_ms": round(float(k[2]), 4),
                              "call_ms": round(float(k[3]), 4), "live_rows": live,
                              "landmarks": sorted({len(w.inv_depth) for w in ws})}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
