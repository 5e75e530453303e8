"""XYZ landmarks (VertexPointXYZ + EdgeReprojectionXYZ, VM/src/backend/edge_reprojection.cc:130-180; 3x3 blocks of Hmm
inverted by problem.cc:421-425): the oracle against structural known answers and — where the compiled reference exists —
against it on fresh seeds; the HIP kernels (k_linearize_xyz, k_backsub_xyz) against the oracle.  The golden files
window_xyz_*.npz are covered by test_oracle_golden.py (oracle) and test_gpu_parity.py (HIP)."""
import os

import numpy as np
import pytest

import vio_testutil as tu
from conftest import GOLDEN_DIR

CAM = [6 + 15 * f + k for f in range(11) for k in range(6)]          # the camera-pose columns of the 171-dim ordering


def nullspace_window(vio):
    """The reference's Hessian null-space demonstration (A/14-sliding-window/src/hessian_nullspace_test.cpp:46-144):
    poses on an arc (theta_n = n 2 pi / 40, radius 8), 20 landmarks in x, y in [-4, 4], z in [8, 10], every landmark
    seen from every pose, identity intrinsics and weights.  There: 10 poses; here the window's 11."""
    synth = vio.synth
    rng = np.random.RandomState(4)
    poses = np.zeros((11, 7))
    for n in range(11):
        th = n * 2 * np.pi / 40
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        poses[n, 0:3] = [8 * np.cos(th) - 8, 8 * np.sin(th), np.sin(2 * th)]
        poses[n, 3:7] = synth.rot_to_quat(R)
    xyz = np.stack([rng.uniform(-4, 4, 20), rng.uniform(-4, 4, 20), rng.uniform(8, 10, 20)], axis=1)
    ext = np.array([0, 0, 0, 0, 0, 0, 1.0])                         # camera == body
    lm = np.repeat(np.arange(20, dtype=np.int32), 11)
    frame = np.tile(np.arange(11, dtype=np.int32), 20)
    pts = np.zeros((220, 2))
    for e in range(220):
        pc = synth.quat_to_rot(poses[frame[e], 3:7]).T @ (xyz[lm[e]] - poses[frame[e], 0:3])
        pts[e] = pc[0:2] / pc[2]
    return synth.Window(poses=poses, speed_bias=np.zeros((11, 9)), ext=ext, xyz=xyz, lm=lm, frame=frame, pts=pts,
                        preint=[None] * 10, prior=None, n_landmarks=20, n_observations=220)


def check_nullspace(vio, lib):
    ctx = lib.context(loss_type=vio.LOSS_TRIVIAL, reproj_sqrt_info=1.0)
    ctx.load(nullspace_window(vio))
    ctx.linearize()
    H, _ = ctx.get_schur_system()
    Hc = H[np.ix_(CAM, CAM)]
    ev = np.linalg.eigvalsh(0.5 * (Hc + Hc.T))
    # monocular bundle adjustment: 7 unobservable directions (6 of the gauge + scale); the landmark Schur complement
    # keeps the nullity of the full Hessian the reference prints
    assert np.abs(ev[:7]).max() <= 1e-9 * ev[-1], ev[:8]
    assert ev[7] >= 1e-5 * ev[-1], ev[:9]
    other = [i for i in range(171) if i not in CAM]
    assert np.abs(H[other]).max() == 0.0                             # no IMU, no prior: nothing else gets information


def test_hessian_nullspace_of_the_oracle(vio, oracle_lib):
    check_nullspace(vio, oracle_lib)


def test_xyz_solve_brings_the_residuals_down_to_the_pixel_noise(vio, oracle_lib):
    w = vio.synth.make_window_xyz(150, seed=5)
    ctx = oracle_lib.context()
    ctx.load(w)
    rep = ctx.solve(10)
    assert rep.final_chi2 < 1e-3 * rep.initial_chi2
    # whitened residuals of N(0, 1/460) pixel noise at information (460/1.5)^2: e2 ~ 2 / 1.5^2 per edge, Cauchy rho(e2) below that
    assert rep.final_chi2 < 0.5 * w.n_observations


def test_kind_switch_and_unsupported_calls(vio, oracle_lib):
    w3, w1 = vio.synth.make_window_xyz(20, seed=1), vio.synth.make_window(20, seed=1)
    ctx = oracle_lib.context()
    ctx.load(w3)
    a = ctx.solve(10).final_chi2
    with pytest.raises(vio.VioError):
        ctx.set_observations(w1.lm, w1.host, w1.target, w1.pts_i, w1.pts_j)    # wrong kind of observation list
    ctx.load(w1)
    b = ctx.solve(10).final_chi2
    ctx.load(w3)
    assert ctx.solve(10).final_chi2 == a and a != b


@pytest.mark.parametrize("n,seed,ragged,ext_fixed,kw", [(1, 1, False, 1, {}), (12, 2, True, 1, {}), (80, 3, True, 0, {}),
                                                        (40, 4, False, 1, dict(obs_per_landmark=10))])
def test_oracle_vs_reference_on_fresh_xyz_windows(vio, oracle_lib, ref_runs, n, seed, ragged, ext_fixed, kw):
    w = vio.synth.make_window_xyz(n, seed=seed, ragged=ragged, **kw)

    def reference(ref_lib):
        cr = ref_lib.context(ext_fixed=ext_fixed)
        cr.load(w)
        out = tu.run_stepwise(cr)
        cr.load(w)
        out.update(tu.run_solve(cr)[0])
        return out
    b = sb = ref_runs.get("xyz_stepwise_and_solve_n%d_s%d" % (n, seed), reference)
    co = oracle_lib.context(ext_fixed=ext_fixed)
    co.load(w)
    a = tu.run_stepwise(co)
    assert tu.scaled_sym_err(a["Hs"][np.ix_(CAM, CAM)], b["Hs"][np.ix_(CAM, CAM)]) <= 1e-9
    assert np.abs(a["dx_pose"] - b["dx_pose"]).max() <= 1e-9 and np.abs(a["dx_lm"] - b["dx_lm"]).max() <= 1e-9
    assert tu.rel_max(a["hll"], b["hll"]) <= 1e-11 and int(a["accepted"]) == int(b["accepted"])
    co.load(w)
    sa, _ = tu.run_solve(co)
    assert int(sa["iterations"]) == int(sb["iterations"])
    assert np.abs(sa["posesF"] - sb["posesF"]).max() <= 1e-6 and np.abs(sa["invdF"] - sb["invdF"]).max() <= 1e-6


# ------------------------------------------------------- GPU ----------------------------------------------------------------
def compare_stepwise(a, b, dx_tol=1e-8):
    assert tu.scaled_sym_err(a["Hs"][np.ix_(CAM, CAM)], b["Hs"][np.ix_(CAM, CAM)]) <= 1e-9
    assert np.abs(a["bs"] - b["bs"]).max() <= 1e-10 * max(np.abs(b["bs"]).max(), 1e-300)
    assert np.abs(a["bpp"] - b["bpp"]).max() <= 1e-10 * max(np.abs(b["bpp"]).max(), 1e-300)
    assert tu.rel_max(a["diag"], b["diag"]) <= 1e-11
    assert tu.rel_max(a["hll"], b["hll"]) <= 1e-10 and tu.rel_max(a["bl"], b["bl"]) <= 1e-9
    assert abs(a["chi0"] - b["chi0"]) <= 1e-10 * abs(b["chi0"])
    assert a["lambda0"] == b["lambda0"]
    assert np.abs(a["dx_pose"] - b["dx_pose"]).max() <= dx_tol
    assert np.abs(a["dx_lm"] - b["dx_lm"]).max() <= dx_tol
    for k in ("poses1", "sb1", "ext1", "invd1"):
        assert np.abs(a[k] - b[k]).max() <= dx_tol, k
    assert abs(a["chi1"] - b["chi1"]) <= 1e-8 * abs(b["chi1"])
    assert int(a["accepted"]) == int(b["accepted"])
    assert abs(a["lambda1"] - b["lambda1"]) <= 1e-9 * abs(b["lambda1"])


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,ragged,ext_fixed,loss,kw", [
    (1, 1, False, 1, 2, {}),                                   # one landmark, five observations
    (9, 2, True, 1, 2, {}),                                    # ragged: 2 .. 11 observations per landmark
    (57, 3, False, 1, 2, {}),                                  # item boundaries
    (300, 5, True, 0, 2, {}),                                  # every pattern, extrinsic vertex free (it gets no information)
    (1000, 6, True, 1, 2, {}),
    (300, 7, False, 1, 0, {}),                                 # no loss object
    (300, 8, False, 1, 3, dict(pos_noise=0.001, rot_noise=0.0002, pixel_noise=0.25 / 460, outlier_fraction=0.05, xyz_noise=0.003)),
    (120, 9, False, 1, 2, dict(obs_per_landmark=10)),          # every landmark seen from all 11 frames (K = 11, 66 pattern columns)
    (5000, 10, False, 1, 2, {}),
])
def test_hip_stepwise_against_oracle(vio, oracle_lib, hip_lib, n, seed, ragged, ext_fixed, loss, kw):
    w = vio.synth.make_window_xyz(n, seed=seed, ragged=ragged, **kw)
    ch, co = hip_lib.context(ext_fixed=ext_fixed, loss_type=loss), oracle_lib.context(ext_fixed=ext_fixed, loss_type=loss)
    ch.load(w)
    co.load(w)
    compare_stepwise(tu.run_stepwise(ch), tu.run_stepwise(co))


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,ragged", [(50, 11, False), (300, 12, True), (2000, 14, False)])
def test_hip_full_solve_against_oracle(vio, oracle_lib, hip_lib, n, seed, ragged):
    w = vio.synth.make_window_xyz(n, seed=seed, ragged=ragged)
    ch, co = hip_lib.context(), oracle_lib.context()
    ch.load(w)
    co.load(w)
    sh, rh = tu.run_solve(ch)
    so, ro = tu.run_solve(co)
    assert rh.iterations == ro.iterations and rh.trials == ro.trials and rh.accepted == ro.accepted
    np.testing.assert_allclose(sh["chi2_trace"], so["chi2_trace"], rtol=1e-6)
    assert abs(rh.final_chi2 - ro.final_chi2) <= 1e-6 * ro.final_chi2
    for k in ("posesF", "sbF", "extF", "invdF"):
        assert np.abs(sh[k] - so[k]).max() <= 1e-6, k


@pytest.mark.gpu
def test_hip_gn_iterations_against_oracle(vio, oracle_lib, hip_lib):
    w = vio.synth.make_window_xyz(400, seed=21)
    ch, co = hip_lib.context(), oracle_lib.context()
    ch.load(w)
    co.load(w)
    for _ in range(5):
        ch.gn_iteration(1e3)
        co.gn_iteration(1e3)
    ch.synchronize()
    ph, sh, _ = ch.get_window()
    po, so, _ = co.get_window()
    # five steps at a damping of 1e3 on a window without a prior: the gauge directions are held by lambda alone, so the
    # accumulated difference is bounded as the end state of a solve is, not as a single update (the per-step contract of 1e-6 is
    # tests/test_gpu_parity.py::test_every_step_from_the_reference_state_within_1e_6).  The oracle solves in Eigen's pivot order,
    # which at lambda = 1e3 is itself 1.2e-7 per step from the exact solution of its system (tests/golden/ldlt_exact.npz); the HIP
    # library's chain order is 1e-9 from it, so five steps differ by Eigen's own rounding: measured 1.2e-6 on the landmarks
    # (VIO_SOLVE_ORDER=eigen: 4e-7).
    assert np.abs(ph - po).max() <= 1e-6 and np.abs(sh - so).max() <= 1e-6
    assert np.abs(ch.get_landmarks_xyz() - co.get_landmarks_xyz()).max() <= 3e-6
    assert abs(ch.chi2() - co.chi2()) <= 1e-7 * co.chi2()


@pytest.mark.gpu
def test_hip_gn_loop_defers_and_flushes_consistently(vio, oracle_lib, hip_lib):
    """The GN loop of an XYZ window leaves a step's landmark back-substitution, chi2 and test to the head of the next
    k_linearize_xyz, which forms W^T dx again from the state the step was linearised at; anybody else who asks first gets them
    from k_backsub_xyz + k_lm_decide (flush).  Both form the same per-observation terms in the same order: the same bits,
    whatever is interleaved; and the stepwise entry points (linearize / solve_linear / update) are the same arithmetic."""
    w = vio.synth.make_window_xyz(900, seed=23, ragged=True)
    lam = 2e5
    plain, mixed, steps = hip_lib.context(), hip_lib.context(), hip_lib.context()
    for c in (plain, mixed, steps):
        c.load(w)
    for _ in range(6):
        plain.gn_iteration(lam)
        steps.linearize()
        steps.solve_linear(lam)
        steps.update_states()
    mixed.gn_iteration(lam)
    mixed.get_window()                                   # read-back: flush
    mixed.gn_iteration(lam)
    mixed.gn_iteration(lam)
    c3 = mixed.chi2()
    mixed.get_landmarks_xyz()
    mixed.gn_iteration(lam)
    mixed.linearize()
    mixed.gn_iteration(lam)
    mixed.gn_iteration(lam)
    for c in (mixed, steps):
        for a, b in zip(c.get_window(), plain.get_window()):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(c.get_landmarks_xyz(), plain.get_landmarks_xyz())
        assert c.chi2() == plain.chi2()
    o = oracle_lib.context()
    o.load(w)
    for _ in range(3):
        o.gn_iteration(lam)
    assert abs(c3 - o.chi2()) <= 1e-9 * c3
    rep = mixed.solve(5)                                  # an LM solve straight after GN iterations starts from the flushed state
    assert np.isfinite(rep.final_chi2) and rep.final_chi2 <= plain.chi2() * (1 + 1e-9)


# ---- Problem::Marginalize of an XYZ graph (problem.cc:617-795: generic over the landmark dimension; no caller in Estimator).
# Only the edges connected to pose 0 enter (:621): every landmark seen from frame 0 has ONE observation and a 3x3 Hmm block of rank
# 2, which the reference inverts all the same (:697-700).  A single view of a free point says nothing about the pose, so in exact
# arithmetic the result is the marginalisation of the graph without reprojection edges; what the reference adds to that is what the
# inverse of a matrix whose third pivot is rounding residue leaves of H_pl H_ll^-1 H_lp - H_pp: a deviation the size of a few
# per cent of the visual information itself (fixture field marg0_free_*: the reference's own edge-free result), reproducible only
# by the identical arithmetic (the oracle mirrors Eigen's: it lands within 0.3 % of that deviation), and NaN whenever an
# elimination meets an exact zero pivot (about one landmark in eight).  So: the oracle against the reference closely; any other
# arithmetic (the HIP kernels) inside the same ball around the edge-free result; the NaN outcome exactly.
MARG0_FIXTURES = sorted(f for f in os.listdir(GOLDEN_DIR) if f.startswith("marg0_xyz_") and not f.endswith("_nan.npz"))


def marg0_window(vio, z):
    kw = {"loss_type": int(z["cfg_loss_type"])} if "cfg_loss_type" in z else {}
    return tu.arrays_to_window(vio, z), kw


def check_xyz_marg0(m, z, same_arithmetic):
    Hf, bf = z["marg0_free_H"], z["marg0_free_b"]
    g, gb = np.abs(z["marg0_H"] - Hf).max(), np.abs(z["marg0_b"] - bf).max()        # the reference's own deviation from the edge-free result
    assert all(np.isfinite(m[k]).all() for k in tu.PRIOR_FIELDS)
    if same_arithmetic:
        assert np.abs(m["H"] - z["marg0_H"]).max() <= 2e-2 * g and np.abs(m["b"] - z["marg0_b"]).max() <= 2e-2 * gb
    else:       # another evaluation order: another draw of the same deviation (its fixtures span 2.5e3 .. 6e4 on a prior of 3.5e5)
        assert np.abs(m["H"] - Hf).max() <= 50 * g and np.abs(m["b"] - bf).max() <= 50 * gb
    # whatever the deviation: a consistent prior (err = -Jt b; Jt^T Jt the pseudo-inverse of H on the kept eigenspace)
    assert np.abs(m["err"] + m["jt_inv"] @ m["b"]).max() <= 1e-9 * max(np.abs(m["err"]).max(), 1e-12)
    P = m["jt_inv"].T @ m["jt_inv"]
    assert np.abs(m["H"] @ P @ m["H"] - m["H"]).max() <= 1e-5 * np.abs(m["H"]).max()


def check_xyz_marg0_nan(lib, vio, allow_another_outcome=False):
    z = np.load(os.path.join(GOLDEN_DIR, "marg0_xyz_n40_s71_tukey_nan.npz"))
    assert int(z["marg0_finite"]) == 0 and (z["marg0_H"] == 0).all() and np.isnan(z["marg0_b"]).all()      # what the reference left
    w, kw = marg0_window(vio, z)
    ctx = lib.context(**kw)
    ctx.load(w)
    with pytest.raises(vio.VioError) as ei:
        ctx.marginalize(vio.MARG_OLD)
    assert ei.value.status == -3                      # VIO_ERR_NOT_FINITE
    m = ctx.marginalize(vio.MARG_OLD, allow_nonfinite=True)
    assert (m["H"] == 0).all() and np.isnan(m["b"]).all() and np.isnan(m["err"]).all() and np.isnan(m["jt_inv"]).all()


def test_oracle_xyz_marginalize_against_the_reference_fixtures(vio, oracle_lib):
    assert len(MARG0_FIXTURES) >= 2
    for f in MARG0_FIXTURES:
        z = np.load(os.path.join(GOLDEN_DIR, f))
        assert int(z["marg0_finite"]) == 1
        w, kw = marg0_window(vio, z)
        ctx = oracle_lib.context(**kw)
        ctx.load(w)
        check_xyz_marg0(ctx.marginalize(vio.MARG_OLD), z, same_arithmetic=True)
        # the well-posed part on its own: the same graph without reprojection edges (prior + IMU edge 0 -> 1 + the dense tail)
        w0 = w.copy()
        w0.xyz, w0.lm, w0.frame, w0.pts = np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2))
        w0.n_landmarks = w0.n_observations = 0
        ctx.load(w0)
        e = ctx.marginalize(vio.MARG_OLD)
        assert np.abs(e["H"] - z["marg0_free_H"]).max() <= 2e-5 * np.abs(z["marg0_free_H"]).max()
        # (b = brr - Arm Amm^+ bmm cancels the O(1e16) bias terms of the IMU edge: 7e-5 of max |b| between the oracle's and Eigen's
        # evaluation orders on these windows)
        assert np.abs(e["b"] - z["marg0_free_b"]).max() <= 5e-4 * max(np.abs(z["marg0_free_b"]).max(), 1.0)
    check_xyz_marg0_nan(oracle_lib, vio)


def test_reference_xyz_marginalize_reproduces_its_fixtures(vio, ref_runs):
    for f in MARG0_FIXTURES + ["marg0_xyz_n40_s71_tukey_nan.npz"]:
        z = np.load(os.path.join(GOLDEN_DIR, f))
        w, kw = marg0_window(vio, z)

        def reference(ref_lib):
            ctx = ref_lib.context(**kw)
            ctx.load(w)
            return ctx.marginalize(vio.MARG_OLD, allow_nonfinite=True)
        m = ref_runs.get("xyz_marginalize_" + f[:-4], reference)
        for k in tu.PRIOR_FIELDS:
            np.testing.assert_array_equal(m[k], z["marg0_" + k])


@pytest.mark.gpu
def test_hip_xyz_marginalize(vio, hip_lib, oracle_lib):
    for f in MARG0_FIXTURES:
        z = np.load(os.path.join(GOLDEN_DIR, f))
        w, kw = marg0_window(vio, z)
        ctx = hip_lib.context(**kw)
        ctx.load(w)
        check_xyz_marg0(ctx.marginalize(vio.MARG_OLD), z, same_arithmetic=False)
        # straight after a solve, as a frame loop would call it, and a solve after it (the context goes on)
        ctx.load(w)
        ctx.solve(3)
        m = ctx.marginalize(vio.MARG_OLD, allow_nonfinite=True)
        assert m["H"].shape == (156, 156)
        assert ctx.solve(2).iterations >= 1
    check_xyz_marg0_nan(hip_lib, vio)
    # the well-posed part against the oracle: an XYZ context without landmarks (prior + IMU edge 0 -> 1 + the dense tail)
    z = np.load(os.path.join(GOLDEN_DIR, MARG0_FIXTURES[0]))
    w, _ = marg0_window(vio, z)
    w.xyz, w.lm, w.frame, w.pts = np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2))
    w.n_landmarks = w.n_observations = 0
    ch, co = hip_lib.context(), oracle_lib.context()
    ch.load(w)
    co.load(w)
    mh, mo = ch.marginalize(vio.MARG_OLD), co.marginalize(vio.MARG_OLD)
    assert np.abs(mh["H"] - mo["H"]).max() <= 2e-5 * np.abs(mo["H"]).max()
    assert np.abs(mh["b"] - mo["b"]).max() <= 5e-4 * np.abs(mo["b"]).max()          # (see the oracle's test above)
    assert np.abs(np.linalg.eigvalsh(mh["H"]) - np.linalg.eigvalsh(mo["H"])).max() <= 2e-5 * np.linalg.eigvalsh(mo["H"]).max()


@pytest.mark.gpu
def test_hip_hessian_nullspace(vio, hip_lib):
    check_nullspace(vio, hip_lib)


@pytest.mark.gpu
def test_hip_kind_switch_prior_and_marg_new(vio, oracle_lib, hip_lib):
    """One context across both kinds of landmark; a window with a prior; MargNewFrame (edge-free, any kind)."""
    w1 = vio.synth.make_window(120, seed=31)
    ch, co = hip_lib.context(), oracle_lib.context()
    ch.load(w1)
    co.load(w1)
    sh, _ = tu.run_solve(ch)
    so, _ = tu.run_solve(co)
    ws = w1.copy()
    ws.poses, ws.speed_bias, ws.ext, ws.inv_depth = so["posesF"], so["sbF"], so["extF"], so["invdF"]
    co.load(ws)
    prior = co.marginalize(vio.MARG_OLD)
    w3 = vio.synth.make_window_xyz(200, seed=32, t0=1.1)
    w3.prior = prior
    ch.load(w3)                                                  # the same context, now with XYZ landmarks
    co.load(w3)
    compare_stepwise(tu.run_stepwise(ch), tu.run_stepwise(co))
    ch.load(w3)
    co.load(w3)
    sh, rh = tu.run_solve(ch)
    so, ro = tu.run_solve(co)
    assert rh.iterations == ro.iterations
    assert np.abs(sh["posesF"] - so["posesF"]).max() <= 1e-6 and np.abs(sh["invdF"] - so["invdF"]).max() <= 1e-6
    assert tu.rel_max(sh["bpriorF"], so["bpriorF"]) <= 1e-7
    from test_oracle_golden import check_prior
    check_prior(ch.marginalize(vio.MARG_SECOND_NEW), co.marginalize(vio.MARG_SECOND_NEW))
    ch.load(w1)                                                  # and back to inverse depths
    co.load(w1)
    assert abs(ch.solve(10).final_chi2 - co.solve(10).final_chi2) <= 1e-6 * co.solve(10).final_chi2 + 1e-9


@pytest.mark.gpu
def test_hip_headline_size_properties(vio, oracle_lib, hip_lib):
    """20 000 XYZ landmarks / 100 000 observations: the update against the oracle, chi2 decreasing over GN iterations,
    run-to-run bitwise reproducibility."""
    w = vio.synth.make_window_xyz(20000, seed=42)
    ch, co = hip_lib.context(), oracle_lib.context()
    ch.load(w)
    co.load(w)
    ch.linearize(); co.linearize()
    (chi_h, lam_h), (chi_o, lam_o) = ch.init_lm(), co.init_lm()
    assert lam_h == lam_o and abs(chi_h - chi_o) <= 1e-10 * chi_o
    ch.solve_linear(lam_o); co.solve_linear(lam_o)
    (dph, dlh), (dpo, dlo) = ch.get_delta(), co.get_delta()
    assert np.abs(dph - dpo).max() <= 1e-8 and np.abs(dlh - dlo).max() <= 1e-8
    runs = []
    for _ in range(2):
        c = hip_lib.context()
        c.load(w)
        chis = []
        for _ in range(4):
            c.gn_iteration(1e2)
            chis.append(c.chi2())
        assert all(b <= a for a, b in zip(chis, chis[1:])), chis
        runs.append((c.get_window()[0], c.get_landmarks_xyz(), chis))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]


@pytest.mark.gpu
def test_xyz_observation_list_in_any_order(vio, hip_lib):
    """A landmark-major list with ascending frames (what make_window_xyz and the reference's loops emit) takes build_plan_xyz's fast
    path — the list is its own CSR, the observations are put into item order on the device —; any other order goes through the table
    of observations by (landmark, frame).  An XYZ pattern is a SET of frames, so the items and every sum are the same: the shuffled
    list gives the same bits, through Solve(10) and MargOldFrame."""
    w = vio.synth.make_window_xyz(900, seed=77, ragged=True)
    order = np.random.RandomState(5).permutation(w.n_observations)
    v = w.copy()
    v.lm, v.frame, v.pts = (np.ascontiguousarray(a[order]) for a in (w.lm, w.frame, w.pts))
    out = []
    for win in (w, v):
        c = hip_lib.context()
        c.load(win)
        rep = c.solve(10)
        pr = c.marginalize(vio.MARG_OLD, allow_nonfinite=True)
        out.append((rep.final_chi2, rep.iterations, c.get_landmarks_xyz(), c.get_window()[0], pr["H"]))
    a, b = out
    assert a[0] == b[0] and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4], equal_nan=True)
