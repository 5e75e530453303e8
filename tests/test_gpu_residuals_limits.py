"""The residual query (csrc/libvio_res_hip.so) at the edges of its tiles and on the inputs that set its flags.

Rule: every output is held to the numpy reference of tests/res_reference.py at the state the HIP context holds, with the tolerances
of test_gpu_residuals.py (rr.check: residual entries 1e-12, e2, rho0 and every sum 1e-10 relative, flags exact); where two calls
must agree bit for bit (one thread computes one edge from the same inputs; a batch runs the single call's code) they are compared
bit for bit.  test_residuals_reference.py establishes each reference-side rule used here on the CPU first (landmarks and frames
without edges, the XYZ point behind the cameras, the sticky NaN maximum, edges in any order, empty windows).

Shapes, from the tiles vio_residuals.hip defines (rr.tile_constants reads OBS_NT, LM_NT and TAIL_NT from the source, so a changed
tile moves the shapes):
  k_res_lm    one thread per landmark, LM_NT = 256 per workgroup, four DPP wave sums added in order: 1, LM_NT - 1, LM_NT and
              LM_NT + 1 landmarks (the last lane, the last wave, a whole workgroup but one lane idle)
  k_res_tail  64 lanes stride over the workgroups' partials: 64 and 65 workgroups (64 LM_NT and 64 LM_NT + 1 landmarks, two edges
              each to keep the reference quick), where the strided loop wraps for the first time
  k_res_obs   one thread per edge, OBS_NT = 256: edge lists cut to 2 OBS_NT - 1, 2 OBS_NT and 2 OBS_NT + 1 edges
  flags       300 landmarks, the broken ones at 3, 63, 64, 255, 256 and 299: different waves and workgroups
  batch       windows of LM_NT, 0, LM_NT + 1, 1 and 0 landmarks (XYZ: 64, 0, 65, around the covariance kernel's LmNT<3>): the empty
              windows of vio_batch_grid.h sit in the middle and at the end

The windows come from rr.limits_window: 20 px of observation noise and outliers of 40 to 60 px on 5 % of the landmarks.  Its
docstring says why: bit 0 and the flag counts are then not all zero, and rr.check's relative bound on e2 and rho0, which an edge with
a residual under 0.03 px cannot meet in fp64 (measured: up to 2.6e-10 on clean windows at 1 px), can be decided.  The batch test's
windows keep 1 px (their covariances must stay well-posed) and carry the outliers alone.

What the solver refuses is queried at the loaded state: a landmark without an edge makes vio_linearize / vio_solve / vio_chi2
return VIO_ERR_UNSUPPORTED (its Hessian block would be singular), so those windows are loaded and not solved, and their summary is
held to the reference without the comparison with vio_chi2.  vio_set_landmarks takes any value, so the flagged states (negative,
NaN) arrive by loading a window that carries them; such a context is never solved or linearised.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_reference as cr  # noqa: E402
import res_reference as rr  # noqa: E402
import test_gpu_batch_diagnostics as tbd  # noqa: E402  (batch_of, topped_up, assert_res_equal, assert_cov_equal)

pytestmark = pytest.mark.gpu

TILES = rr.tile_constants()
OBS_NT, LM_NT, TAIL_NT = TILES["OBS_NT"], TILES["LM_NT"], TILES["TAIL_NT"]
TAIL_STRIDE = 64                       # k_res_tail: `for (b = lane; b < n_wg; b += 64)`, one wave per column


def test_tile_constants():
    """The literals this module's reasoning rests on, against the source text."""
    src = open(rr.RES_SOURCE).read()
    tail = open(os.path.join(os.path.dirname(rr.RES_SOURCE), "vio_res_tail_body.inc")).read()
    assert (OBS_NT, LM_NT, TAIL_NT) == (256, 256, 256)
    assert "for (int b = lane; b < a.n_wg; b += %d)" % TAIL_STRIDE in tail
    assert "const int n_wg = (int)((n + LM_NT - 1) / LM_NT);" in src
    assert "const unsigned g = (unsigned)((m + OBS_NT - 1) / OBS_NT);" in src


def solved(vio, hip_lib, w, iterations=3):
    c = hip_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    c.solve(iterations)
    return c


SIZES = [(1, False), (LM_NT - 1, False), (LM_NT, False), (LM_NT + 1, False), (TAIL_STRIDE * LM_NT, False), (TAIL_STRIDE * LM_NT + 1, False),
         (LM_NT - 1, True), (LM_NT, True), (LM_NT + 1, True)]


@pytest.mark.parametrize("n,xyz", SIZES, ids=["%s%d" % ("xyz" if x else "n", n) for n, x in SIZES])
def test_landmark_counts_around_a_workgroup_and_the_tail_stride(vio, hip_lib, oracle_lib, n, xyz):
    w = rr.limits_window(vio, n, xyz, seed=13, t0=1.05, obs_per_landmark=2 if n > 4 * LM_NT else 4)
    c = solved(vio, hip_lib, w)
    px = 25.0                                                      # of the order of these windows' mean errors: bit 0 is mixed
    got = c.residuals(w, outlier_px=px)
    rr.check(vio, oracle_lib, c, w, got, outlier_px=px)
    assert n < 100 or 0 < got["summary"]["n_flagged"][0] < n          # (set on some landmarks and clear on others; check() holds the count)
    assert got["obs"].shape == (len(w.lm), 4) and got["lm"].shape == (n, 3) and got["flags"].shape == (n,)
    assert got["summary"]["frame_edges"].sum() == len(w.lm)


@pytest.mark.parametrize("m", [2 * OBS_NT - 1, 2 * OBS_NT, 2 * OBS_NT + 1])
def test_edge_lists_cut_around_a_workgroup(vio, hip_lib, oracle_lib, m):
    """The last k_res_obs workgroup with 255, 256 and 1 edges.  Five edges a landmark and as many landmarks as keep an edge each when
    the list is cut, so the cut window still solves."""
    K = 5
    n = (2 * OBS_NT - 2) // K + 1
    w = rr.limits_window(vio, n, seed=14, obs_per_landmark=K)
    assert len(w.lm) == K * n >= 2 * OBS_NT + 1
    wt = rr.take_edges(w, slice(0, m))
    assert len(wt.lm) == m and np.bincount(wt.lm, minlength=n).min() >= 1
    c = solved(vio, hip_lib, wt)
    assert c.m == m
    rr.check(vio, oracle_lib, c, wt, c.residuals(wt))


def test_landmarks_and_a_frame_without_edges(vio, hip_lib, oracle_lib):
    """cnt == 0: mean, maximum and rho 0 and no REPROJ bit, for the first and last landmark and both sides of a workgroup boundary; a
    frame nobody observes: 0 edges, 0.0.  (Loaded, not solved: the solver refuses a landmark without an edge.)"""
    n = 300
    assert LM_NT < n < 2 * LM_NT
    w = rr.limits_window(vio, n, seed=12)
    gone, frame = [0, LM_NT - 1, LM_NT, n - 1], 5
    wd = rr.take_edges(w, ~np.isin(w.lm, gone) & (w.target != frame))
    c = hip_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(wd)
    with pytest.raises(vio.VioError) as ei:
        c.linearize()
    assert ei.value.status == -5 and "without observations" in str(ei.value)
    got = c.residuals(wd)
    rr.compare(got, rr.reference_of(oracle_lib, vio, c, wd))
    assert np.all(got["lm"][gone] == 0.0) and not got["flags"][gone].any()
    assert np.all(got["lm"][np.delete(np.arange(n), gone), 0] > 0.0)
    s = got["summary"]
    assert s["frame_edges"][frame] == 0 and s["frame_robust"][frame] == 0.0
    assert np.array_equal(s["frame_edges"], np.bincount(wd.target, minlength=rr.NF))


def test_the_callers_order_is_kept(vio, hip_lib, oracle_lib):
    """The same edges in a seeded random order, at the same state: eidx (CSR slot -> caller's edge) is far from the identity, and
    fr[e] / dneg[e] are read through it.  One thread computes one edge from the same inputs: the rows are the unpermuted call's,
    permuted, bit for bit."""
    n = 600
    w = rr.limits_window(vio, n, seed=15, ragged=True)
    c = solved(vio, hip_lib, w)
    a = c.residuals(w)
    perm = np.random.RandomState(6).permutation(len(w.lm))
    wp = rr.take_edges(rr.with_state(w, c), perm)
    assert np.count_nonzero(wp.lm[1:] < wp.lm[:-1]) > len(w.lm) // 4             # nowhere near landmark-major
    cp = hip_lib.context(loss_type=vio.LOSS_CAUCHY)
    cp.load(wp)
    b = cp.residuals(wp)
    assert np.array_equal(b["obs"], a["obs"][perm])
    rr.check(vio, oracle_lib, cp, wp, b)
    assert np.array_equal(b["summary"]["frame_edges"], a["summary"]["frame_edges"])
    assert np.array_equal(b["lm"][:, 1], a["lm"][:, 1])                            # a maximum does not depend on the order
    rr.check(vio, oracle_lib, c, w, a)


FLAGGED = [3, 63, 64, 255, 256, 299]


def check_flagged(got, ref, broken, nan, n):
    """The flag test's assertions: flags and counts exact, NaN where and only where the reference has NaN, the rest to rr.compare's
    tolerances."""
    obs, lmo, flags, s = ref
    assert not np.any(np.abs(lmo[:, 0] - 1e4) <= 1e-5)                       # no mean at the threshold: every flag is decided
    assert np.array_equal(got["flags"], flags)
    g = got["summary"]
    assert np.array_equal(g["n_flagged"], s["n_flagged"])
    assert np.array_equal(g["n_flagged"], [np.count_nonzero(got["flags"] & b) for b in (1, 2, 4)])
    for l in nan:
        assert np.isnan(got["lm"][l, 0]) and np.isnan(got["lm"][l, 1]), l      # the mean, and the sticky maximum
    assert np.array_equal(np.isnan(got["lm"]), np.isnan(lmo)) and np.array_equal(np.isnan(got["obs"]), np.isnan(obs))
    others = np.delete(np.arange(n), broken)
    assert not got["flags"][others].any() and np.all(np.isfinite(got["lm"][others]))
    fin = np.isfinite(lmo).all(axis=1)
    for k in range(3):
        assert rr.rel_err(got["lm"][fin, k], lmo[fin, k]) <= 1e-10, k
    efin = np.isfinite(obs).all(axis=1)
    assert np.abs(got["obs"][efin, :2] - obs[efin, :2]).max() <= 1e-12
    assert rr.rel_err(got["obs"][efin, 2], obs[efin, 2]) <= 1e-10 and rr.rel_err(got["obs"][efin, 3], obs[efin, 3]) <= 1e-10
    for key in ("visual_robust", "visual_plain", "chi2"):
        assert np.isnan(g[key]) == np.isnan(s[key]) and np.isnan(s[key]) == bool(len(nan)), key
    assert np.array_equal(np.isnan(g["frame_robust"]), np.isnan(s["frame_robust"]))
    ffin = np.isfinite(s["frame_robust"])
    assert rr.rel_err(g["frame_robust"][ffin], s["frame_robust"][ffin]) <= 1e-10
    assert np.array_equal(g["frame_edges"], s["frame_edges"])
    for k in range(rr.NW):
        assert abs(g["imu_edge"][k] - s["imu_edge"][k]) <= 1e-10 * abs(s["imu_edge"][k]), k


def test_state_and_depth_flags_of_inverse_depths(vio, hip_lib, oracle_lib):
    """VIO_RES_FLAG_STATE and VIO_RES_FLAG_DEPTH on the device: negative inverse depths (behind every camera, solve_flag 2) and NaN
    ones (NaN mean and maximum, REPROJ and STATE, no DEPTH), and one NaN observation among a landmark's finite ones (the maximum
    keeps it)."""
    n = 300
    w = rr.limits_window(vio, n, seed=16)
    w.inv_depth = np.array(w.inv_depth)
    neg, nan, nan_obs = FLAGGED[0::2], FLAGGED[1::2], 130
    w.inv_depth[neg] *= -1.0
    w.inv_depth[nan] = np.nan
    w.pts_j[np.nonzero(w.lm == nan_obs)[0][0], 0] = np.nan
    c = hip_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)                                                      # (loaded only: a non-finite state never reaches the solver)
    got = c.residuals(w, outlier_px=1e4)
    ref = rr.reference_of(oracle_lib, vio, c, w, outlier_px=1e4)
    check_flagged(got, ref, FLAGGED + [nan_obs], nan + [nan_obs], n)
    assert np.all(got["flags"][neg] & vio.FLAG_DEPTH) and np.all(got["flags"][neg] & vio.FLAG_STATE)
    assert np.all(got["flags"][nan] == (vio.FLAG_REPROJ | vio.FLAG_STATE))
    assert got["flags"][nan_obs] == vio.FLAG_REPROJ
    assert np.all(np.isfinite(got["lm"][neg]))


def test_state_and_depth_flags_of_xyz_points(vio, hip_lib, oracle_lib):
    """k_res_obs<3> on points behind every camera that observes them (DEPTH alone, finite residuals) and on NaN coordinates."""
    n = 300
    w = rr.limits_window(vio, n, True, seed=16)
    w.xyz = np.array(w.xyz)
    behind, nan = FLAGGED[0::2], FLAGGED[1::2]
    for l in behind:
        w.xyz[l] = rr.behind_every_camera(w, l)
    for k, l in enumerate(nan):
        w.xyz[l, k] = np.nan
    c = hip_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    got = c.residuals(w, outlier_px=1e4)
    ref = rr.reference_of(oracle_lib, vio, c, w, outlier_px=1e4)
    check_flagged(got, ref, FLAGGED, nan, n)
    assert np.all(got["flags"][behind] == vio.FLAG_DEPTH) and np.all(np.isfinite(got["lm"][behind]))
    assert np.all(got["flags"][nan] == (vio.FLAG_REPROJ | vio.FLAG_STATE))


def test_empty_window(vio, hip_lib, oracle_lib):
    """m == 0 and n == 0: no k_res_obs and no k_res_lm launch, one partial row nobody wrote, the tail's sums over zero workgroups."""
    w = vio.synth.make_window(0, seed=5)
    c = solved(vio, hip_lib, w)
    got = c.residuals(w)
    _, _, _, s = rr.check(vio, oracle_lib, c, w, got)
    assert got["obs"].shape == (0, 4) and got["lm"].shape == (0, 3) and got["flags"].shape == (0,)
    g = got["summary"]
    assert g["visual_robust"] == 0.0 and g["visual_plain"] == 0.0 and not g["frame_robust"].any() and not g["frame_edges"].any()
    assert not g["n_flagged"].any() and g["imu"] > 0.0 and g["chi2"] == 0.5 * g["imu"]
    # after a larger window on the same handle: the partial rows of that call are not summed again
    big = rr.limits_window(vio, 2 * LM_NT + 3, seed=5)
    c.load(big)
    c.solve(2)
    rr.check(vio, oracle_lib, c, big, c.residuals(big))
    c.load(w)
    c.solve(2)
    again = c.residuals(w)
    rr.check(vio, oracle_lib, c, w, again)
    assert again["summary"]["visual_robust"] == 0.0 and not again["summary"]["frame_edges"].any()


def test_landmarks_without_any_edge(vio, hip_lib, oracle_lib):
    """n > 0 and m == 0: every landmark reports zeros and no flag, the visual terms are 0."""
    n = LM_NT + 1
    w = vio.synth.make_window(n, seed=7)
    wd = rr.take_edges(w, np.zeros(len(w.lm), dtype=bool))
    c = hip_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(wd)
    got = c.residuals(wd)
    rr.compare(got, rr.reference_of(oracle_lib, vio, c, wd))
    assert got["obs"].shape == (0, 4) and got["lm"].shape == (n, 3) and not got["lm"].any() and not got["flags"].any()
    g = got["summary"]
    assert g["visual_robust"] == 0.0 and not g["frame_edges"].any() and not g["n_flagged"].any()
    assert g["chi2"] == 0.5 * (g["imu"] + g["prior"])


def batch(vio, hip_lib, sizes, xyz):
    """Contexts on one stream for windows of `sizes` landmarks, each with a prior that makes its covariance well-posed
    (cr.well_posed_prior through topped_up), solved one by one.  The extrinsic is held fixed: a window without an edge does not
    observe it."""
    make = vio.synth.make_window_xyz if xyz else vio.synth.make_window
    ws = [make(n, seed=70 + i, t0=1.0 + 0.01 * i) for i, n in enumerate(sizes)]
    ws = [rr.add_outliers(vio, w) if w.n_landmarks else w for w in ws]
    ctxs = tbd.batch_of(hip_lib, [(w, dict(loss_type=vio.LOSS_CAUCHY, ext_fixed=1)) for w in ws])
    for c, w in zip(ctxs, ws):
        tbd.topped_up(c, w)
        c.solve(3)
    return ctxs, ws


@pytest.mark.parametrize("xyz,sizes", [(False, (LM_NT, 0, LM_NT + 1, 1, 0)), (True, (64, 0, 65))], ids=["inverse_depth", "xyz"])
def test_batch_with_empty_windows(vio, hip_lib, oracle_lib, xyz, sizes):
    """vio_batch_grid.h's window without work (blk0[w] == blk0[w + 1]) in the middle and at the end of a batch whose other windows
    end on, and one past, a workgroup: every window's residual outputs and covariances are the single call's, bit for bit, the
    empty windows' summaries are the reference's, and every covariance is the reference's."""
    assert cr.lm_tile(3) == 64 and LM_NT == 2 * cr.lm_tile(1)
    ctxs, ws = batch(vio, hip_lib, sizes, xyz)
    covs = tbd.assert_cov_equal(vio, hip_lib, ctxs, ws, "fix_oldest", xyz)
    for c, w, (P, L) in zip(ctxs, ws, covs):
        cr.check_cov(oracle_lib, c, w, P, L, xyz)
        assert L.shape[0] == w.n_landmarks
    got = tbd.assert_res_equal(hip_lib, ctxs, ws)
    for c, w, r in zip(ctxs, ws, got):
        rr.check(vio, oracle_lib, c, w, r)
        if w.n_landmarks == 0:
            g = r["summary"]
            assert g["visual_robust"] == 0.0 and not g["frame_edges"].any() and not g["n_flagged"].any()
            assert g["imu"] > 0.0 and g["prior"] >= 0.0 and g["chi2"] == 0.5 * (g["imu"] + g["prior"])
