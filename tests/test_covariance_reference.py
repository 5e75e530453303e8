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


def test_a_landmark_without_an_edge_has_no_information(vio, oracle_lib):
    """What test_gpu_covariance_limits.py asks the device to refuse: with every edge of a landmark taken out of the list its h_l and
    its coupling are exactly 0 (so 1 / h_l is no variance), and the other landmarks' terms do not change by a bit."""
    import res_reference as rr
    n = cr.lm_tile(1) + 1
    w = vio.synth.make_window(n, seed=18)
    c = oracle_lib.context(loss_type=vio.LOSS_CAUCHY)
    c.load(w)
    c.solve(3)
    poses, _, ext = c.get_window()
    vals = c.get_landmarks()
    h, Wl = cr.landmark_terms(oracle_lib, c.cfg, w, poses, ext, vals)
    assert np.all(h > 0)
    for gone in ([0], [n - 1], [5, n - 1]):
        bare = rr.take_edges(w, ~np.isin(w.lm, gone))
        hb, Wb = cr.landmark_terms(oracle_lib, c.cfg, bare, poses, ext, vals)
        assert np.all(hb[gone] == 0.0) and not Wb[gone].any()
        rest = np.delete(np.arange(n), gone)
        assert np.array_equal(hb[rest], h[rest]) and np.array_equal(Wb[rest], Wl[rest])
        assert int(np.nonzero(~(hb > 0))[0].min()) == min(gone)           # the landmark the library names
    # XYZ: H_ll = 0 fails Sylvester's criterion at its first minor
    wx = vio.synth.make_window_xyz(cr.lm_tile(3) + 1, seed=18)
    cx = oracle_lib.context(loss_type=vio.LOSS_CAUCHY)
    cx.load(wx)
    posx, _, extx = cx.get_window()
    Hb, Wx = cr.landmark_terms(oracle_lib, cx.cfg, rr.take_edges(wx, wx.lm != 64), posx, extx, cx.get_landmarks_xyz())
    assert not Hb[64].any() and not Wx[64].any() and np.all(np.linalg.det(Hb[:64]) > 0)


def test_the_limits_module_reads_its_tiles_from_the_source():
    assert (cr.lm_tile(1), cr.lm_tile(3)) == (128, 64)
