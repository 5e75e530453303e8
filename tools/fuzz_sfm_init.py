#!/usr/bin/env python3
"""Randomised windows through the batched structure-from-motion and the alignment behind it (diagnostic; the fixed cases live in
tests/test_gpu_sfm.py, test_gpu_sfm_limits.py and test_gpu_init.py).  What it is after are the shapes and settings no fixture
spells out: per case it draws F, the landmarks per frame (10 to 200, log-uniform), the track length (2 to F), the pixel noise, the
share of outliers in the newest frame (0 to 0.3), the share of inner tracks, the hypothesis count (1 to VIO_SFM_MAX_HYPOTHESES,
log-uniform) and the sampling seed.

The check, by the rules of tests/test_gpu_sfm.py and tests/test_gpu_init.py: sfm_batch's stage 1 must equal tests/sfm_reference.py's
exactly (status, l, hypothesis, counts, mask) and within 10x the restatement's spread under two one-ulp perturbations plus 1e-13 of
the size (R, T, parallax); construct_batch, fed the restatement's stage 1, is held to the same spread rule, statuses and fail frames
exactly, iteration counts where the perturbations leave the restatement's alone.  Where sfm_batch succeeds, initialize_batch runs
on its result and is compared with tests/init_reference.py on the same frames and the re-propagated records, as
test_gpu_init.py::test_initialize_batch_runs_the_whole_alignment does.

A case is skipped, and counted, when the restatement cannot decide it: its margin to the RANSAC gate is at most 1e-6, or one of
its statuses (or l, or the winning hypothesis) changes under a one-ulp perturbation.  Such a case is undecidable, not a failure.

  python tools/fuzz_sfm_init.py [cases] [seed] [cpu]        cpu: the restatement alone (no device), to see the skipped share"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import ORACLE_DIR, load_package  # noqa: E402
import init_reference as ir  # noqa: E402
import sfm_reference as sr  # noqa: E402
import test_gpu_init as ti  # noqa: E402
import test_gpu_sfm as tg  # noqa: E402

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
cpu_only = len(sys.argv) > 3 and sys.argv[3] == "cpu"

vio = load_package()
from vio_amd import stream as vs  # noqa: E402
orc = vio.VioLib(os.path.join(ORACLE_DIR, "liboracle.so"), "vioo_")
if not cpu_only:
    vio.load_hip()
    sfm_h, init_h, imu_h = vio.load_sfm().create(), vio.load_init().create(), vio.load_imu().create()
TIC, G = np.asarray(vio.synth.T_IC, dtype=np.float64), vio.synth.G_NORM


def draw(rng):
    F = int(rng.randint(3, sr.MAX_FRAMES + 1))
    c = dict(F=F, L=int(round(10 * 20 ** rng.rand())), T=int(rng.randint(2, F + 1)), noise=float(rng.choice([0.0, 0.05, 0.1, 0.3])),
             outliers=float(rng.choice([0.0, 0.0, 0.3 * rng.rand()])), inner=float(rng.choice([0.0, 0.4 * rng.rand()])),
             hyps=int(round(4096 ** rng.rand())), seed=int(rng.randint(0, 2 ** 32, dtype=np.uint64)), stream_seed=int(rng.randint(1000)))
    st = vs.SyntheticStream(n_frames=F + 1, landmarks_per_frame=c["L"], track_len=c["T"], pixel_noise=c["noise"] * tg.PX, seed=c["stream_seed"])
    item = sr.window_item(st, list(range(F)))[0]
    if c["inner"] > 0:
        item = tg.with_inner_tracks(item, c["inner"], seed=c["stream_seed"] + 1)
    if c["outliers"] > 0:
        item = tg.with_outliers(item, F - 1, c["outliers"], seed=c["stream_seed"] + 2)
    return c, st, item


def stage1_key(r):
    return (r["status"], r["l"], r["hyp"], r["n_inliers"], r["front"], r["mask"].tobytes())


def compare(what, got, ref, spread, errs):
    try:
        tg._close(got, ref, spread, what)
    except AssertionError as e:
        errs.append("%s: %s" % (what, e))


def run_case(c, st, item):
    """('ok' | 'skip' | 'FAIL', text)."""
    cfg = dict(seed=c["seed"], ransac_hypotheses=c["hyps"])
    ref = sr.sfm(item, cfg)
    rel = ref["rel"]
    if rel["status"] == sr.OK and not rel["margin"] > 1e-6:
        return "skip", "margin %.1e" % rel["margin"]
    rng = np.random.RandomState(5)
    runs = [sr.relative_pose(sr.perturb_ulp(item, rng), cfg) for _ in range(2)]
    if any(stage1_key(p) != stage1_key(rel) for p in runs):
        return "skip", "stage 1's outcome changes under one ulp"
    runs2 = []
    if rel["status"] == sr.OK:                              # stage 2 from the restatement's stage 1
        runs2 = [sr.construct(p_item, rel["l"], rel["R"], rel["T"]) for p_item in perturbed_items(item)]
        if any((p["status"], p["fail_frame"]) != (ref["status"], ref["fail_frame"]) for p in runs2):
            return "skip", "construct's outcome changes under one ulp"
    text = "sfm %d l %d hyp %d" % (ref["status"], rel["l"], rel["hyp"])
    if cpu_only:
        if ref["status"] == sr.OK:                          # the alignment's decidability, from the restatement's own SfM result
            F = c["F"]
            it = vio.sfm_items_to_init_items([ref], vio.synth.R_IC, [st.preint[:F - 1]])[0]
            bg = ir.gyro_bias(orc, it, np.zeros(3))[0]
            aref = ir.align(orc, it, TIC, G, bg)
            rng = np.random.RandomState(11)
            if any(ir.align(orc, ir.perturb_ulp(it, rng), TIC, G, bg)["status"] != aref["status"] for _ in range(2)):
                return "skip", "the alignment's status changes under one ulp"
            text += " init %d" % aref["status"]
        return "ok", text
    errs = []
    sfm_h.set_config(**cfg)
    both = sfm_h.sfm_batch([item])[0]
    g = both["rel"]
    if stage1_key(g) != stage1_key(rel) or g["n_corres"] != len(rel["mask"]) or not np.array_equal(g["corres"], rel["corres"]):
        errs.append("stage 1: device (%d, %d, %d, %d, %d) restatement (%d, %d, %d, %d, %d)" % (
            g["status"], g["l"], g["hyp"], g["n_inliers"], g["front"], rel["status"], rel["l"], rel["hyp"], rel["n_inliers"], rel["front"]))
    sp = tg._spread(rel, runs, ("R", "T", "parallax"))
    for k in ("R", "T", "parallax"):
        compare("rel." + k, g[k], rel[k], sp[k], errs)
    if both["status"] != ref["status"]:
        errs.append("sfm_batch status %d, restatement %d" % (both["status"], ref["status"]))
    if rel["status"] == sr.OK:
        two = sfm_h.construct_batch([item], [rel])[0]
        sp = tg._spread(ref, runs2, tg.STAGE2)
        if (two["status"], two["fail_frame"]) != (ref["status"], ref["fail_frame"]) or not np.array_equal(two["state"], ref["state"]):
            errs.append("stage 2: device (%d, %d) restatement (%d, %d)" % (two["status"], two["fail_frame"], ref["status"], ref["fail_frame"]))
        for k in tg.STAGE2:
            compare(k, two[k], ref[k], sp[k], errs)
        if all(np.array_equal(p["pnp_iterations"], ref["pnp_iterations"]) and p["ba_iterations"] == ref["ba_iterations"] for p in runs2):
            if not np.array_equal(two["pnp_iterations"], ref["pnp_iterations"]) or two["ba_iterations"] != ref["ba_iterations"]:
                errs.append("iterations: device %s %d restatement %s %d" % (two["pnp_iterations"], two["ba_iterations"],
                                                                           ref["pnp_iterations"], ref["ba_iterations"]))
        else:
            text += " (iteration counts left out)"
    if both["status"] == sr.OK and not errs:
        F = c["F"]
        it = vio.sfm_items_to_init_items([both], vio.synth.R_IC, [st.preint[:F - 1]])[0]
        out = init_h.initialize_batch([it], [st.imu[:F - 1]], imu_h, TIC, G)[0]
        bg_ref, bst = ir.gyro_bias(orc, it, np.zeros(3))
        rng = np.random.RandomState(2)
        bsp = max(np.abs(ir.gyro_bias(orc, ir.perturb_ulp(it, rng), np.zeros(3))[0] - bg_ref).max() for _ in range(2))
        if bst != ir.OK or not np.abs(out["bg"] - bg_ref).max() <= 10 * bsp + 1e-16:
            errs.append("gyro bias %s restatement %s (status %d)" % (out["bg"], bg_ref, bst))
        it2 = dict(it, pre=out["pre"])
        aref = ir.align(orc, it2, TIC, G, out["bg"])
        rng = np.random.RandomState(11)
        if any(ir.align(orc, ir.perturb_ulp(it2, rng), TIC, G, out["bg"])["status"] != aref["status"] for _ in range(2)):
            return "skip", "the alignment's status changes under one ulp"
        asp = ti._perturbed_spread(orc, it2, TIC, G, out["bg"], aref)
        if out["status"] != aref["status"] or out["n_key"] != aref["n_key"]:
            errs.append("alignment status %d, restatement %d" % (out["status"], aref["status"]))
        for k in ti.FIELDS:
            try:
                ti._close(out[k], aref[k], asp[k], "init." + k)
            except AssertionError as e:
                errs.append("init.%s: %s" % (k, e))
        text += " init %d" % aref["status"]
    return ("FAIL", "; ".join(errs)) if errs else ("ok", text)


def perturbed_items(item):
    rng = np.random.RandomState(6)
    return [sr.perturb_ulp(item, rng) for _ in range(2)]


count = {"ok": 0, "skip": 0, "FAIL": 0}
for k in range(n_cases):
    c, st, item = draw(np.random.RandomState(1000 * seed0 + k))
    verdict, text = run_case(c, st, item)
    count[verdict] += 1
    print("%-4s case %3d: F %2d L %3d T %2d noise %.2f outliers %.2f inner %.2f hyps %4d seed %10d, %4d tracks: %s" % (
        verdict, k, c["F"], c["L"], c["T"], c["noise"], c["outliers"], c["inner"], c["hyps"], c["seed"], len(item["start_frame"]), text), flush=True)
print("cases: %d  failures: %d  skipped: %d (share %.3f)" % (n_cases, count["FAIL"], count["skip"], count["skip"] / max(n_cases, 1)))
sys.exit(1 if count["FAIL"] else 0)
