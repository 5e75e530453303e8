"""The math of the marginal covariances (include/vio_covariance.h) against the dense inverse of the whole
window's Hessian, built in numpy from the oracle's own pieces (tests/cov_reference.py).  This pins the reference numbers the GPU
tests use: the pose block of inv(H_full) is inv of the oracle's H_pp_schur, and its landmark diagonal blocks are the formula."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_reference as cr  # noqa: E402


def pose_hessian(oracle_lib, ctx):
    f = oracle_lib.dll.vioo_get_pose_hessian
    H = np.zeros((cr.PD, cr.PD))
    assert f(ctx.h, cr._dp(H)) == 0
    return H


@pytest.mark.parametrize("case", cr.CASES, ids=[c[0] for c in cr.CASES])
def test_schur_inverse_is_the_dense_inverse(vio, oracle_lib, case):
    w, kw, gauge = cr.make_case(vio, oracle_lib, case)
    xyz = case[7]
    c = oracle_lib.context(**kw)
    c.load(w)
    c.solve(5)
    c.linearize()
    S, _ = c.get_schur_system()
    poses, _, ext = c.get_window()
    vals = c.get_landmarks_xyz() if xyz else c.get_landmarks()
    h, Wl = cr.landmark_terms(oracle_lib, c.cfg, w, poses, ext, vals)
    hll, _ = c.get_landmark_system()
    ok = ~cr.huber_ambiguous(oracle_lib, c.cfg, w, poses, ext, vals)
    assert ok.sum() >= 0.5 * ok.size
    assert np.abs(h[ok] - hll[ok]).max() <= 1e-12 * np.abs(hll).max()  # the recomputed information is MakeHessian's

    keep = cr.keep_index(kw["ext_fixed"], gauge, xyz)
    tol = cr.tolerance(S, keep)
    assert tol < 1e-6, "window too ill-conditioned to pin anything: %g" % tol
    P = cr.pose_cov_from_schur(S, keep)
    Fi = np.linalg.inv(cr.full_hessian(pose_hessian(oracle_lib, c), h, Wl, keep))
    nk = keep.size
    Pf = np.zeros((cr.PD, cr.PD))
    Pf[np.ix_(keep, keep)] = Fi[:nk, :nk]
    assert cr.scaled_err(Pf, P) <= tol

    lm = cr.landmark_cov(P, h, Wl)
    D = 3 if xyz else 1
    n = h.shape[0]
    blocks = np.stack([Fi[nk + D * l:nk + D * l + D, nk + D * l:nk + D * l + D] for l in range(n)])
    want = blocks[:, 0, 0] if D == 1 else blocks
    scale = np.sqrt(np.abs(np.einsum("...ii->...i", want.reshape(n, D, D))))
    err = np.abs(lm.reshape(n, D, D) - want.reshape(n, D, D)) / (scale[:, :, None] * scale[:, None, :])
    assert err.max() <= tol

    # fixed variables are zero rows and columns
    fixed = np.setdiff1d(np.arange(cr.PD), keep)
    assert not P[fixed].any() and not P[:, fixed].any()


def test_pose_block_helper(vio):
    P = np.arange(cr.PD * cr.PD, dtype=np.float64).reshape(cr.PD, cr.PD)
    assert np.array_equal(vio.pose_block(P, 10), P[156:162, 156:162])
    assert np.array_equal(vio.speed_bias_block(P, 0), P[12:21, 12:21])
    with pytest.raises(IndexError):
        vio.pose_block(P, 11)
