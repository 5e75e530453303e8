"""One JSON line: the time of one residual query (include/vio_residuals.h) at N = 300 and N = 20 000 landmarks, split into read-back of
the states + packing + upload (host wall clock), k_res_obs, k_res_lm and k_res_tail (HIP events on the context's stream) and the whole
call (wall clock), median of --reps calls after --warmup, with every output asked for and with the summary alone.  Each window is
bench.py's: synth.make_window with a marginalisation prior, solved first."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

ALL = ("obs", "lm", "flags", "summary")


def one(vio, hip, n, reps, warmup):
    wp = vio.synth.make_window(300, seed=41, t0=0.9)
    cp = hip.context()
    cp.load(wp)
    cp.solve(5)
    w = vio.synth.make_window(n, seed=1)
    w.prior = cp.marginalize(vio.MARG_OLD)
    c = hip.context()
    c.load(w)
    c.solve(5)
    c.residuals(w)                          # the handle, and its staging buffers at their size
    out = {"landmarks": n, "observations": int(w.n_observations)}
    for label, outputs in (("all_outputs", ALL), ("summary_only", ("summary",))):
        rows = []
        for k in range(warmup + reps):
            c._res.compute(w, outputs=outputs)
            if k >= warmup:
                rows.append(c._res.timing())
        med = {key: float(np.median([r[key] for r in rows])) for key in rows[0]}
        out[label] = {k: round(v * 1000.0, 2) for k, v in (("host_us", med["host_ms"]), ("k_res_obs_us", med["k_res_obs_ms"]),
                                                          ("k_res_lm_us", med["k_res_lm_ms"]), ("k_res_tail_us", med["k_res_tail_ms"]),
                                                          ("total_us", med["total_ms"]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    vio = g.load_package()
    hip = vio.load_hip()
    vio.load_res()
    print(json.dumps({"metric": "residual_query", "windows": [one(vio, hip, n, args.reps, args.warmup) for n in (300, 20000)]}))


if __name__ == "__main__":
    main()
