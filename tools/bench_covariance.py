"""One JSON line: the time of one covariance query (include/vio_covariance.h) at N = 300 and N = 20 000 landmarks, split into
linearise + read-back + upload (host wall clock), k_cov_pose and k_cov_landmarks (HIP events on the context's stream), median of
--reps calls after --warmup.  Each window is bench.py's: synth.make_window with a marginalisation prior, solved first.  The prior gets
1 % of the window's own diagonal on frame 0's speed and biases on top: these windows leave a common accelerometer-bias offset unobservable
(DESIGN.md section 10), and the timed calls should compute covariances that mean something (pivot_ratio in the line says so)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def one(vio, hip, n, reps, warmup, relinearize):
    wp = vio.synth.make_window(300, seed=41, t0=0.9)
    cp = hip.context()
    cp.load(wp)
    cp.solve(5)
    w = vio.synth.make_window(n, seed=1)
    mp = cp.marginalize(vio.MARG_OLD)
    c = hip.context()
    w.prior = mp
    c.load(w)
    c.linearize()
    S0, _ = c.get_schur_system()
    prior = {k: np.array(v) for k, v in mp.items()}
    idx = np.arange(12, 21)                 # frame 0's speed and biases (the 156-ordering of the prior = the 171 one up to frame 9)
    prior["H"][idx, idx] += 1e-2 * np.diag(S0)[idx]
    w.prior = prior
    c.load(w)
    c.solve(5)
    rows = []
    for k in range(warmup + reps):
        if relinearize:
            c.solve(1)          # the state's linearisation is stale again: every call pays for vio_linearize, as after a solve
        c.covariance(w)
        if k >= warmup:
            rows.append(c._cov.timing())
    med = {key: float(np.median([r[key] for r in rows])) for key in rows[0]}
    return {"landmarks": n, "observations": int(w.n_observations), "pivot_ratio": c._cov.pivot_ratio(), **{k: round(v * 1000.0, 2) for k, v in
            (("host_us", med["host_ms"]), ("k_cov_pose_us", med["k_cov_pose_ms"]), ("k_cov_landmarks_us", med["k_cov_landmarks_ms"]),
             ("total_us", med["total_ms"]))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    vio = g.load_package()
    hip = vio.load_hip()
    vio.load_cov()
    out = {"metric": "covariance_query", "after_solve": [one(vio, hip, n, args.reps, args.warmup, True) for n in (300, 20000)],
           "linearised": [one(vio, hip, n, args.reps, args.warmup, False) for n in (300, 20000)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
