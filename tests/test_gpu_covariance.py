"""Marginal covariances on the GPU (csrc/libvio_cov_hip.so, include/vio_covariance.h) against the numpy reference of
tests/cov_reference.py, which test_covariance_reference.py pins to the dense inverse of the whole window's Hessian."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu


reference, lm_err = cr.reference_at, cr.lm_err         # (shared with the limits modules)


@pytest.mark.parametrize("case", cr.CASES, ids=[c[0] for c in cr.CASES])
def test_covariance_matches_the_reference(vio, hip_lib, oracle_lib, case):
    w, kw, gauge = cr.make_case(vio, oracle_lib, case)
    xyz = case[7]
    c = hip_lib.context(**kw)
    c.load(w)
    c.solve(5)
    P, L = c.covariance(w, gauge=["none", "fix_oldest"][gauge])
    Pr, Lr, S, keep, h = reference(oracle_lib, c, w, gauge, xyz)
    tol = cr.tolerance(S, keep)
    assert tol < 1e-6, tol
    assert cr.scaled_err(P, Pr) <= tol
    assert np.array_equal(P, P.T)                                  # both triangles written from the one packed entry
    fixed = np.setdiff1d(np.arange(cr.PD), keep)
    assert np.all(P[fixed] == 0.0) and np.all(P[:, fixed] == 0.0)
    # (Huber windows: landmarks with an edge beyond delta, where the robust weight's correction term follows the rounding, are left out)
    poses, _, ext = c.get_window()
    ok = ~cr.huber_ambiguous(oracle_lib, c.cfg, w, poses, ext, c.get_landmarks_xyz() if xyz else c.get_landmarks())
    assert ok.sum() >= 0.5 * ok.size
    assert lm_err(L[ok], Lr[ok]) <= tol
    # the kernel's recomputed information is MakeHessian's (vio_get_landmark_system)
    hk = c._cov.landmark_information(xyz)
    hll, _ = c.get_landmark_system()
    assert np.abs(hk[ok] - hll[ok]).max() <= 1e-12 * np.abs(hll).max()
    assert np.abs(hk[ok] - h.reshape(hk.shape)[ok]).max() <= 1e-12 * np.abs(h).max()


def test_bench_window_with_prior(vio, hip_lib, oracle_lib):
    """bench.py's steady-state window: 20 000 landmarks and a marginalisation prior (topped up to be well-posed)."""
    wp = vio.synth.make_window(300, seed=41, t0=0.9)
    cp = oracle_lib.context()
    cp.load(wp)
    cp.solve(5)
    mp = cp.marginalize(vio.MARG_OLD)
    w = vio.synth.make_window(20000, seed=1)
    c = hip_lib.context()
    w.prior = mp
    c.load(w)
    c.linearize()
    S0, _ = c.get_schur_system()
    w.prior = cr.well_posed_prior(np.diag(S0), mp)
    c.load(w)
    c.solve(5)
    P, L = c.covariance(w)
    sample = np.sort(np.random.RandomState(5).choice(w.n_landmarks, 500, replace=False))
    Pr, Lr, S, keep, _ = reference(oracle_lib, c, w, 1, False, sample)
    ref_inv = np.zeros_like(P)
    ref_inv[np.ix_(keep, keep)] = np.linalg.inv(S[np.ix_(keep, keep)])      # numpy.linalg.inv of vio_get_schur_system as it is
    tol = cr.tolerance(S, keep)
    assert tol < 1e-6, tol
    assert cr.scaled_err(P, ref_inv) <= tol
    assert lm_err(L[sample], Lr) <= tol
    assert np.all(L > 0)


def test_rank_deficient_window_is_refused_and_outputs_untouched(vio, hip_lib):
    """Frame 10 without observations and without its IMU edge: its rows of H_pp_schur are zero."""
    w = vio.synth.make_window(120, seed=9)
    keep = (w.host != 10) & (w.target != 10)
    for k in ("lm", "host", "target", "pts_i", "pts_j"):
        setattr(w, k, getattr(w, k)[keep])
    w.preint = list(w.preint)
    w.preint[9] = None
    c = hip_lib.context()
    c.load(w)
    c.linearize()
    P, L = np.full((cr.PD, cr.PD), 7.0), np.full(w.n_landmarks, 7.0)
    with pytest.raises(vio.VioError) as ei:
        c.covariance(w)                   # creates the handle; then the same call with caller-owned outputs
    assert ei.value.status == -3 and "not positive and finite" in str(ei.value), str(ei.value)
    with pytest.raises(vio.VioError) as ei:
        c._cov.compute(w, "fix_oldest", pose_cov=P, lm_out=L)
    assert ei.value.status == -3
    assert np.all(P == 7.0) and np.all(L == 7.0)


def run_stream(vio, hip_lib, with_cov):
    """Three frames of solve -> (covariance) -> marginalise -> next frame; what every frame leaves behind."""
    c = hip_lib.context()
    prior, out = None, []
    for k in range(3):
        w = vio.synth.make_window(400, seed=20 + k, t0=1.0 + 0.1 * k)
        w.prior = prior
        c.load(w)
        rep = c.solve(5)
        if with_cov:
            try:
                c.covariance(w)
            except vio.VioError as e:      # (a first window without a prior may be singular; the state must not care either way)
                assert e.status == -3
        poses, sb, ext = c.get_window()
        rec = [poses, sb, ext, c.get_landmarks(), np.array([rep.iterations, rep.trials, rep.accepted, rep.stop_reason]),
               np.array([rep.initial_chi2, rep.final_chi2, rep.final_lambda]), np.array(rep.chi2_trace), np.array(rep.lambda_trace)]
        prior = c.marginalize(vio.MARG_OLD)
        rec += [prior[x] for x in ("H", "b", "err", "jt_inv")]
        out.append(rec)
    c.close()
    return out


def test_the_query_changes_nothing(vio, hip_lib):
    a, b = run_stream(vio, hip_lib, False), run_stream(vio, hip_lib, True)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            assert np.array_equal(x, y, equal_nan=True)


def test_two_calls_are_bitwise_identical(vio, hip_lib, oracle_lib):
    for case in (cr.CASES[1], cr.CASES[6]):
        w, kw, gauge = cr.make_case(vio, oracle_lib, case)
        c = hip_lib.context(**kw)
        c.load(w)
        c.solve(5)
        P1, L1 = c.covariance(w, gauge=["none", "fix_oldest"][gauge])
        P2, L2 = c.covariance(w, gauge=["none", "fix_oldest"][gauge])
        assert np.array_equal(P1, P2) and np.array_equal(L1, L2)


def test_sharded_context_is_unsupported(vio, hip_lib):
    c = hip_lib.context(shard_rank=0, shard_count=2)
    with pytest.raises(vio.VioError) as ei:
        vio.load_cov().create(c)
    assert ei.value.status == -5


def test_set_config_between_two_queries(vio, hip_lib, oracle_lib):
    """vio_set_config on a living context (one context for many graphs): the next query follows the new loss and ext_fixed."""
    case = cr.CASES[0]                                  # Cauchy, extrinsic free
    w, kw, gauge = cr.make_case(vio, oracle_lib, case)
    c = hip_lib.context(**kw)
    c.load(w)
    c.solve(5)
    c.covariance(w)                                     # the handle exists from here on
    c.set_config(loss_type=vio.LOSS_HUBER, loss_delta=5.0, ext_fixed=1)
    P, L = c.covariance(w)                              # no solve in between: the context still holds the Cauchy linearisation
    Pr, Lr, S, keep, h = reference(oracle_lib, c, w, 1, False)
    assert not np.isin(np.arange(6), keep).any()        # the extrinsic is now held fixed ...
    assert np.all(P[:6] == 0.0) and np.all(P[:, :6] == 0.0)
    hll, _ = c.get_landmark_system()                    # ... and the system is the Huber one
    poses, _, ext = c.get_window()
    ok = ~cr.huber_ambiguous(oracle_lib, c.cfg, w, poses, ext, c.get_landmarks())
    assert ok.sum() >= 0.5 * ok.size
    tol = cr.tolerance(S, keep)
    assert cr.scaled_err(P, Pr) <= tol
    assert lm_err(L[ok], Lr[ok]) <= tol
    hk = c._cov.landmark_information()
    assert np.abs(hk[ok] - hll[ok]).max() <= 1e-12 * np.abs(hll).max()
    # the same through the C entry point alone: a handle told of the change by vio_cov_set_config
    c2 = hip_lib.context(**kw)
    c2.load(w)
    c2.solve(5)
    h2 = vio.load_cov().create(c2)
    h2.compute(w)
    c2.set_config(loss_type=vio.LOSS_HUBER, loss_delta=5.0, ext_fixed=1)    # (VioContext.set_config forwards only to c2._cov)
    h2.set_config(c2.cfg)
    P2, L2 = h2.compute(w)
    assert np.array_equal(P2, P) and np.array_equal(L2, L)
    h2.close()


def test_pivot_ratio_reports_conditioning(vio, hip_lib, oracle_lib):
    """VIO_OK on a nearly singular window (the synthetic windows' common accelerometer-bias offset, no prior) is told apart by the
    pivot ratio; a well-posed one has a ratio far from eps."""
    w, kw, gauge = cr.make_case(vio, oracle_lib, cr.CASES[0])
    c = hip_lib.context(**kw)
    c.load(w)
    c.solve(5)
    c.covariance(w)
    good = c._cov.pivot_ratio()
    w.prior = None
    c.load(w)
    c.solve(5)
    try:
        c.covariance(w)
        bad = c._cov.pivot_ratio()
    except vio.VioError as e:                           # (or rounding left that direction's pivot non-positive)
        assert e.status == -3
        bad = 0.0
    assert good > 1e-8 and bad < 1e-10, (good, bad)
