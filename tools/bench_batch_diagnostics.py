"""One JSON line: the batched covariance and residual queries (vio_cov_compute_batch, vio_res_compute_batch)
against the loop of single calls over the same contexts, at B = 1, 16, 64, 256 windows of N = 300 landmarks (throughput item
policy, bench.py's batched regime).  Every query follows a vio_batch_solve, so each one linearises its windows first, as a caller's
would.  Times are wall clock around the Python call, median of --reps; the split is the library's (vio_cov_timing / vio_res_timing
of the batch: host = linearise + read-back + upload of every window, then each kernel over all windows, then the whole call)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def well_posed(c, w):
    """Frame 0's speed and biases get 1e-2 of their diagonal of H_pp_schur as prior information (a synthetic window leaves a common
    accelerometer-bias offset unobservable): without it the covariance of such a window is singular."""
    w.prior = None
    c.load(w)
    c.linearize()
    S0, _ = c.get_schur_system()
    P = 156
    prior = {"H": np.zeros((P, P)), "b": np.zeros(P), "err": np.zeros(P), "jt_inv": np.zeros((P, P))}
    idx = np.arange(12, 21)
    prior["H"][idx, idx] = 1e-2 * np.diag(S0)[idx]
    w.prior = prior
    c.load(w)


def med(xs):
    return float(np.median(xs))


def one(vio, hip, B, n, reps):
    pol = vio.capi.ITEMS_THROUGHPUT
    lead = hip.context(item_policy=pol)
    ctxs = [lead] + [hip.context(stream=lead.get_stream(), item_policy=pol) for _ in range(B - 1)]
    ws = []
    for i, c in enumerate(ctxs):
        w = vio.synth.make_window(n, seed=100 + i)
        well_posed(c, w)
        ws.append(w)
    hip.batch_solve(ctxs, 10)
    hip.batch_covariance(ctxs, ws)          # handles and staging buffers at their size
    hip.batch_residuals(ctxs, ws)
    for c, w in zip(ctxs, ws):
        c.covariance(w)
        c.residuals(w)
    t = {k: [] for k in ("cov_batch", "cov_loop", "res_batch", "res_loop")}
    split_cov, split_res = [], []
    for _ in range(reps):
        hip.batch_solve(ctxs, 10)
        t0 = time.perf_counter()
        hip.batch_covariance(ctxs, ws)
        t["cov_batch"].append(time.perf_counter() - t0)
        split_cov.append(lead._cov.timing())
        hip.batch_solve(ctxs, 10)
        t0 = time.perf_counter()
        for c, w in zip(ctxs, ws):
            c.covariance(w)
        t["cov_loop"].append(time.perf_counter() - t0)
        hip.batch_solve(ctxs, 10)
        t0 = time.perf_counter()
        hip.batch_residuals(ctxs, ws)
        t["res_batch"].append(time.perf_counter() - t0)
        split_res.append(lead._res.timing())
        hip.batch_solve(ctxs, 10)
        t0 = time.perf_counter()
        for c, w in zip(ctxs, ws):
            c.residuals(w)
        t["res_loop"].append(time.perf_counter() - t0)
    out = {"windows": B, "landmarks": n}
    for k, v in t.items():
        out[k + "_ms"] = round(med(v) * 1e3, 3)
    out["cov_speedup"] = round(out["cov_loop_ms"] / out["cov_batch_ms"], 2)
    out["res_speedup"] = round(out["res_loop_ms"] / out["res_batch_ms"], 2)
    out["cov_batch_split_ms"] = {k: round(med([s[k] for s in split_cov]), 3) for k in split_cov[0]}
    out["res_batch_split_ms"] = {k: round(med([s[k] for s in split_res]), 3) for k in split_res[0]}
    for c in ctxs:
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--landmarks", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    vio = g.load_package()
    hip = vio.load_hip()
    vio.load_cov()
    vio.load_res()
    rows = [one(vio, hip, int(b), args.landmarks, args.reps) for b in args.batches.split(",")]
    print(json.dumps({"metric": "batch_diagnostics", "rows": rows}))


if __name__ == "__main__":
    main()
