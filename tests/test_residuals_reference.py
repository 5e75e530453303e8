"""The residual query's reference (tests/res_reference.py, built on the oracle's exported pieces) against the oracle itself: its chi2
breakdown adds up to the oracle context's vio_chi2 under every loss, with the extrinsic fixed and free, for XYZ landmarks, with a
marginalisation prior and with an IMU edge missing; and on the seeded outlier window its flags meet the recall and precision the GPU
tests hold the library to."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import res_reference as rr  # noqa: E402


@pytest.mark.parametrize("case", rr.CASES, ids=[c[0] for c in rr.CASES])
def test_breakdown_adds_up_to_the_oracle_chi2(vio, oracle_lib, case):
    w, kw = rr.make_case(vio, oracle_lib, case)
    c = oracle_lib.context(**kw)
    c.load(w)
    c.solve(5)
    obs, lmo, flags, s = rr.reference_of(oracle_lib, vio, c, w)
    chi = c.chi2()
    assert abs(s["chi2"] - chi) <= 1e-12 * abs(chi), (s["chi2"], chi)
    assert s["imu"] == s["imu_edge"].sum()
    if case[6] is not None:
        assert s["imu_edge"][case[6]] == 0.0
    assert (s["prior"] > 0) == bool(case[4])
    assert s["frame_edges"].sum() == len(w.lm)
    assert np.isclose(s["frame_robust"].sum(), s["visual_robust"], rtol=1e-12)
    if kw["loss_type"] == 0:
        assert np.array_equal(obs[:, 2], obs[:, 3])              # no loss: rho0 is e2
    else:
        assert np.all(obs[:, 3] <= obs[:, 2] * (1 + 1e-15))      # the robust losses only shrink
    assert not flags.any()                                        # a clean window: nothing to flag


def test_no_imu_gives_nan(vio, oracle_lib):
    w, kw = rr.make_case(vio, oracle_lib, rr.CASES[2])
    c = oracle_lib.context(**kw)
    c.load(w)
    _, _, _, s = rr.reference_of(oracle_lib, vio, c, w, imu=False)
    assert np.isnan(s["chi2"]) and np.isnan(s["imu"]) and np.all(np.isnan(s["imu_edge"]))
    assert np.isfinite(s["visual_robust"])


def test_seeded_outliers_recall_and_precision(vio, oracle_lib):
    w, truth = rr.outlier_window(vio)
    assert truth.sum() == 100
    c = oracle_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    c.solve(10)
    _, lmo, flags, s = rr.reference_of(oracle_lib, vio, c, w, outlier_px=3.0)
    recall, precision = rr.recall_precision(flags, truth)
    assert recall >= rr.RECALL_MIN and precision >= rr.PRECISION_MIN, (recall, precision)
    assert s["n_flagged"][0] == np.count_nonzero(flags & 1)
    # the margins the thresholds rest on
    assert lmo[~truth, 0].max() < 2.5 and lmo[truth, 0].min() > 9.0


def test_flag_rules_on_a_broken_state(vio, oracle_lib):
    """Bit 1 (a point behind the observing camera) and bit 2 (an inverse depth that is not positive and finite)."""
    w = vio.synth.make_window(30, seed=5)
    c = oracle_lib.context()
    c.load(w)
    poses, sb, ext = c.get_window()
    vals = np.array(c.get_landmarks())
    vals[3], vals[7] = -vals[3], np.nan
    _, err = c.get_prior()
    # (the initial state is unsolved: bit 0 is kept out of the way with a threshold no clean landmark reaches)
    _, lmo, flags, s = rr.reference(oracle_lib, vio, c.cfg, w, poses, sb, ext, vals, err, outlier_px=1e4)
    assert flags[3] & 2 and flags[3] & 4                         # negative depth: behind every camera, and solve_flag = 2
    assert flags[7] == 5                                          # NaN: the mean error is NaN too (a NaN depth is not <= 0)
    assert np.isnan(lmo[7, 0]) and np.isnan(lmo[7, 1])
    assert not np.delete(flags, [3, 7]).any()
    assert list(s["n_flagged"]) == [int(flags[3] & 1) + 1, 1, 2]


# ---- the rules test_gpu_residuals_limits.py asks the device for, established here first ------------------------------------------
def _state(c):
    poses, sb, ext = c.get_window()
    _, err = c.get_prior()
    return poses, sb, ext, err


def test_landmarks_and_frames_without_edges(vio, oracle_lib):
    """A landmark without an edge reports zeros and no REPROJ bit, a frame without an edge 0 edges and 0.0; everything else is what
    the full window's reference gives for the edges that are left."""
    n = 300
    w = vio.synth.make_window(n, seed=12)
    gone, frame = [0, 255, 256, n - 1], 5
    keep = ~np.isin(w.lm, gone) & (w.target != frame)
    wd = rr.take_edges(w, keep)
    assert 0 < wd.lm.size < w.lm.size and np.all(np.bincount(wd.lm, minlength=n)[gone] == 0)
    c = oracle_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    poses, sb, ext, err = _state(c)
    vals = np.array(c.get_landmarks())
    obs, lmo, flags, s = rr.reference(oracle_lib, vio, c.cfg, w, poses, sb, ext, vals, err, outlier_px=1e4)
    obd, lmd, fld, sd = rr.reference(oracle_lib, vio, c.cfg, wd, poses, sb, ext, vals, err, outlier_px=1e4)
    assert np.array_equal(obd, obs[keep])                          # an edge's row depends on that edge alone
    assert np.all(lmd[gone] == 0.0) and not fld[gone].any()
    whole = np.bincount(wd.lm, minlength=n) == np.bincount(w.lm, minlength=n)
    assert whole.sum() > n // 3 and np.array_equal(lmd[whole], lmo[whole]) and np.array_equal(fld[whole], flags[whole])
    assert sd["frame_edges"][frame] == 0 and sd["frame_robust"][frame] == 0.0
    assert np.array_equal(sd["frame_edges"], np.bincount(w.target[keep], minlength=rr.NF))
    assert sd["frame_edges"].sum() == wd.lm.size
    assert abs(sd["visual_robust"] - math.fsum(obs[keep, 3])) <= 1e-13 * sd["visual_robust"]
    assert abs(sd["visual_plain"] - math.fsum(obs[keep, 2])) <= 1e-13 * sd["visual_plain"]
    assert np.array_equal(sd["imu_edge"], s["imu_edge"]) and sd["prior"] == s["prior"]
    assert list(sd["n_flagged"]) == [0, 0, 0]


def test_xyz_point_behind_the_cameras_and_nan_coordinate(vio, oracle_lib):
    """XYZ: a finite point behind every camera that observes it has bit 1 alone and a finite mean; a NaN coordinate has bits 0 and 2,
    NaN mean and maximum, and no bit 1 (a NaN depth is not <= 0)."""
    w = vio.synth.make_window_xyz(40, seed=5)
    w.xyz = np.array(w.xyz)
    behind, nan = [3, 17], [7, 39]
    for l in behind:
        w.xyz[l] = rr.behind_every_camera(w, l)
    for k, l in enumerate(nan):
        w.xyz[l, k] = np.nan
    c = oracle_lib.context()
    c.load(w)
    poses, sb, ext, err = _state(c)
    obs, lmo, flags, s = rr.reference(oracle_lib, vio, c.cfg, w, poses, sb, ext, w.xyz, err, outlier_px=1e4)
    for l in behind:
        edges = np.nonzero(w.lm == l)[0]
        assert all(rr._depth(poses, ext, w, e, w.xyz, True) < 0.0 for e in edges)     # every observing camera, not just the first
        assert flags[l] == 2 and np.all(np.isfinite(lmo[l])) and np.all(np.isfinite(obs[edges]))
    for l in nan:
        assert flags[l] == 5 and np.isnan(lmo[l, 0]) and np.isnan(lmo[l, 1]) and np.isnan(lmo[l, 2])
    others = np.delete(np.arange(40), behind + nan)
    assert not flags[others].any() and np.all(np.isfinite(lmo[others]))
    assert list(s["n_flagged"]) == [2, 2, 2]
    assert np.isnan(s["visual_robust"]) and np.isnan(s["chi2"])
    nan_frames = np.unique(w.frame[np.isin(w.lm, nan)])
    assert np.array_equal(np.nonzero(np.isnan(s["frame_robust"]))[0], nan_frames)


def test_a_nan_maximum_sticks(vio, oracle_lib):
    """One NaN observation among a landmark's edges: the mean and the maximum are NaN whatever the edge's place in the list (the
    first edge's NaN is not replaced by the finite ones after it), bit 0 is set and nothing else."""
    w = vio.synth.make_window(20, seed=5)
    c = oracle_lib.context()
    c.load(w)
    poses, sb, ext, err = _state(c)
    vals = np.array(c.get_landmarks())
    for l, which in ((4, 0), (9, 2), (15, -1)):
        wn = w.copy()
        wn.pts_j[np.nonzero(w.lm == l)[0][which], 1] = np.nan
        _, lmo, flags, s = rr.reference(oracle_lib, vio, c.cfg, wn, poses, sb, ext, vals, err, outlier_px=1e4)
        assert np.isnan(lmo[l, 0]) and np.isnan(lmo[l, 1]) and np.isnan(lmo[l, 2]) and flags[l] == 1
        assert not np.delete(flags, l).any() and np.all(np.isfinite(np.delete(lmo, l, axis=0)))


def test_edges_in_any_order(vio, oracle_lib):
    """The caller's order is kept: a permuted list gives the permuted rows bit for bit, the same flags and frame counts, and the
    per-landmark and per-frame sums to the rounding of another summation order."""
    w = vio.synth.make_window(60, seed=8, ragged=True)
    c = oracle_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    c.solve(3)
    perm = np.random.RandomState(4).permutation(w.lm.size)
    wp = rr.take_edges(w, perm)
    assert not np.array_equal(wp.lm, w.lm) and np.array_equal(np.sort(wp.lm), w.lm)
    obs, lmo, flags, s = rr.reference_of(oracle_lib, vio, c, w)
    obp, lmp, flp, sp = rr.reference_of(oracle_lib, vio, c, wp)
    assert np.array_equal(obp, obs[perm])
    assert np.array_equal(lmp[:, 1], lmo[:, 1]) and np.allclose(lmp, lmo, rtol=1e-13, atol=0.0)
    assert np.array_equal(flp, flags) and np.array_equal(sp["frame_edges"], s["frame_edges"])
    assert np.allclose(sp["frame_robust"], s["frame_robust"], rtol=1e-13, atol=0.0)
    for k in ("visual_robust", "visual_plain", "chi2"):
        assert abs(sp[k] - s[k]) <= 1e-13 * abs(s[k]), k


def test_empty_windows(vio, oracle_lib):
    """No landmarks and no edges: empty outputs, the visual terms exactly 0, and chi2 still the oracle's (IMU alone).  Landmarks
    without any edge: rows of zeros and no flag."""
    w = vio.synth.make_window(0, seed=5)
    assert w.lm.size == 0 and w.n_landmarks == 0
    c = oracle_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    c.solve(3)
    obs, lmo, flags, s = rr.reference_of(oracle_lib, vio, c, w)
    assert obs.shape == (0, 4) and lmo.shape == (0, 3) and flags.shape == (0,)
    assert s["visual_robust"] == 0.0 and s["visual_plain"] == 0.0 and not s["frame_robust"].any() and not s["frame_edges"].any()
    chi = c.chi2()
    assert s["imu"] > 0.0 and abs(s["chi2"] - chi) <= 1e-12 * abs(chi) and list(s["n_flagged"]) == [0, 0, 0]
    wx = vio.synth.make_window_xyz(0, seed=5)                     # ... the same for an XYZ window
    cx = oracle_lib.context(loss_type=vio.LOSS_CAUCHY)
    cx.load(wx)
    ox, lx, fx, sx = rr.reference_of(oracle_lib, vio, cx, wx)
    assert ox.shape == (0, 4) and lx.shape == (0, 3) and fx.shape == (0,) and sx["visual_robust"] == 0.0 and sx["imu"] > 0.0
    w = rr.take_edges(vio.synth.make_window(5, seed=5), np.zeros(20, dtype=bool))
    c.load(w)
    poses, sb, ext, err = _state(c)
    obs, lmo, flags, s2 = rr.reference(oracle_lib, vio, c.cfg, w, poses, sb, ext, np.array(c.get_landmarks()), err)
    assert obs.shape == (0, 4) and lmo.shape == (5, 3) and not lmo.any() and not flags.any()
    assert s2["visual_robust"] == 0.0 and not s2["frame_edges"].any() and s2["chi2"] == 0.5 * (s2["imu"] + s2["prior"])


def test_the_limits_module_reads_its_tiles_from_the_source():
    t = rr.tile_constants()
    assert t == {"OBS_NT": 256, "LM_NT": 256, "TAIL_NT": 256}, t
