"""The reference's own bundle-adjustment acceptance test, TestMonoBA (A/15-vio-backend/app/TestMonoBA.cpp, result published
in A/15-vio-backend/README.md:21-73), through the C ABI: three cameras on an arc, 20 landmarks as inverse depths hosted in
camera 0 and seen from cameras 1 and 2 (EdgeReprojection, identity extrinsic, identity information, no loss), the gauge held
by a prior of weight 1e4 on the first two camera poses, LM for up to 100 iterations.

In the 11-frame window of the ABI the cameras are frames 0..2, frames 3..10 carry no edge at all (their rows of the system
are zero: LM's damping keeps them where they are), there is no IMU factor, and the two EdgeSE3Prior edges are the
marginalisation prior's form of the same quadratic: H = 1e4 on the 12 pose coordinates, err = 100 * (pose (-) ground truth),
b = -J^T err, updated to first order with every accepted step (problem.cc:466-475).

The scene is tests/golden/monoba.npz (make_golden_monoba.py: the generator of the source restated, pinned to the README's
depth-noise column).  The reference's verdict is "the estimation has converged to ground truth": |opt - gt| <= 3e-4 in
inverse depth on every landmark of its table; here the observations carry the 1e-3 of noise the current source adds, which
bounds what any estimator can recover at about 1.3e-4 (1 sigma) per landmark.
"""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def quat_z(theta):
    return np.array([0.0, 0.0, np.sin(theta / 2), np.cos(theta / 2)])


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def monoba_window(vio):
    z = np.load(os.path.join(HERE, "golden", "monoba.npz"))
    poses, poses_gt = np.zeros((11, 7)), np.zeros((11, 7))
    for f in range(11):
        c = min(f, 2)
        poses[f, 0:3], poses[f, 3:7] = z["t_obs"][c], quat_z(z["theta_obs"][c])
        poses_gt[f, 0:3], poses_gt[f, 3:7] = z["t_gt"][c], quat_z(z["theta_gt"][c])
    n = 20
    lm = np.repeat(np.arange(n, dtype=np.int32), 2)
    host = np.zeros(2 * n, dtype=np.int32)
    target = np.tile(np.array([1, 2], dtype=np.int32), n)
    pts_i = z["obs"][lm, 0, :].copy()
    pts_j = z["obs"][lm, target, :].copy()
    # the gauge prior on cameras 0 and 1 in the marginalisation prior's form
    H, b, err, jt = np.zeros((156, 156)), np.zeros(156), np.zeros(156), np.zeros((156, 156))
    for f in (0, 1):
        qg = poses_gt[f, 3:7]
        dq = quat_mul(np.array([-qg[0], -qg[1], -qg[2], qg[3]]), poses[f, 3:7])
        delta = np.concatenate([poses[f, 0:3] - poses_gt[f, 0:3], 2.0 * dq[0:3] * np.sign(dq[3])])
        idx = 6 + 15 * f + np.arange(6)
        H[idx, idx] = 1e4
        jt[idx, idx] = 1e-2
        err[idx] = 100.0 * delta
        b[idx] = -1e4 * delta
    w = vio.synth.Window(poses=poses, speed_bias=np.zeros((11, 9)), ext=np.array([0, 0, 0, 0, 0, 0, 1.0]), inv_depth=z["inv_depth_init"].copy(),
                         lm=lm, host=host, target=target, pts_i=pts_i, pts_j=pts_j, preint=[None] * 10,
                         prior=dict(H=H, b=b, err=err, jt_inv=jt), n_landmarks=n, n_observations=2 * n)
    return w, z, poses_gt


def check_converged(ctx, z, poses_gt, landmarks=None, poses=None):
    """ctx: a context after its solve (or None, with what one handed back after its solve as `landmarks` and `poses`)"""
    inv_gt = 1.0 / z["points"][:, 2]
    opt = ctx.get_landmarks() if ctx is not None else landmarks
    e0, e1 = np.abs(z["inv_depth_init"] - inv_gt), np.abs(opt - inv_gt)
    assert e0.max() > 0.05                                   # the start is far off (the README's "with noise" column: up to 0.09)
    assert e1.max() <= 6e-4 and e1.mean() <= 2.5e-4          # the README's table: <= 3e-4, without observation noise
    p = ctx.get_window()[0] if ctx is not None else poses
    assert np.abs(p[0:2, 0:3] - poses_gt[0:2, 0:3]).max() <= 1e-4          # held by the prior
    # camera 2 is held by its 20 observations alone: 1e-3 of pixel noise trades 1e-3 rad of rotation against 8 mm of translation
    assert np.abs(p[2, 0:3] - poses_gt[2, 0:3]).max() <= 3e-2 and np.linalg.norm(p[2, 0:3] - poses_gt[2, 0:3]) < np.linalg.norm(z["t_obs"][2] - z["t_gt"][2])
    assert np.abs(p[3:, :] - ctx_initial_unused(z)).max() == 0.0           # frames without edges have not moved


def ctx_initial_unused(z):
    return np.tile(np.concatenate([z["t_obs"][2], quat_z(z["theta_obs"][2])]), (8, 1))


def test_fixture_is_pinned_to_the_readme():
    z = np.load(os.path.join(HERE, "golden", "monoba.npz"))
    mine = 1.0 / z["inv_depth_init"] - z["points"][:, 2]
    theirs = 1.0 / z["readme_inv_depth_noisy"] - 1.0 / z["readme_inv_depth_gt"]
    assert np.abs(mine - theirs).max() <= 0.06                # the depth-noise draws (camera 0's height noise is within 0.05)
    assert np.abs(1.0 / z["points"][2:18, 2] - z["readme_inv_depth_gt"][4:20]).max() <= 5.1e-5
    assert np.abs(z["readme_inv_depth_opt"] - z["readme_inv_depth_gt"]).max() <= 3.01e-4      # the reference's acceptance level
    assert np.abs(z["readme_cam_t_opt"] - z["t_gt"]).max() <= 5.1e-5


def test_oracle_converges_to_ground_truth(vio, oracle_lib):
    w, z, poses_gt = monoba_window(vio)
    c = oracle_lib.context(ext_fixed=1, loss_type=0, reproj_sqrt_info=1.0)
    c.load(w)
    rep = c.solve(100)
    assert rep.final_chi2 < 1e-3 * rep.initial_chi2
    check_converged(c, z, poses_gt)


def test_reference_objects_converge_the_same_way(vio, oracle_lib, ref_runs):
    """The compiled reference backend (VM's problem.cc, the successor of A/15's) on the same window: the oracle follows it."""
    w, z, poses_gt = monoba_window(vio)

    def reference(ref_lib):
        cr = ref_lib.context(ext_fixed=1, loss_type=0, reproj_sqrt_info=1.0)
        cr.load(w)
        rr = cr.solve(100)
        return {"iterations": rr.iterations, "landmarks": cr.get_landmarks(), "poses": cr.get_window()[0]}
    r = ref_runs.get("monoba", reference)
    co = oracle_lib.context(ext_fixed=1, loss_type=0, reproj_sqrt_info=1.0)
    co.load(w)
    ro = co.solve(100)
    assert int(r["iterations"]) == ro.iterations
    assert np.abs(r["landmarks"] - co.get_landmarks()).max() <= 1e-7
    assert np.abs(r["poses"] - co.get_window()[0]).max() <= 1e-7
    check_converged(None, z, poses_gt, landmarks=r["landmarks"], poses=r["poses"])


@pytest.mark.gpu
def test_hip_converges_to_ground_truth(vio, oracle_lib, hip_lib):
    w, z, poses_gt = monoba_window(vio)
    ch, co = hip_lib.context(ext_fixed=1, loss_type=0, reproj_sqrt_info=1.0), oracle_lib.context(ext_fixed=1, loss_type=0, reproj_sqrt_info=1.0)
    ch.load(w)
    co.load(w)
    rh, ro = ch.solve(100), co.solve(100)
    assert rh.iterations == ro.iterations
    assert np.abs(ch.get_landmarks() - co.get_landmarks()).max() <= 1e-7
    assert np.abs(ch.get_window()[0] - co.get_window()[0]).max() <= 1e-7
    check_converged(ch, z, poses_gt)
