"""The numpy restatement of rejectWithF and undistortedPoints (tests/reject_reference.py) against what it restates: the lift inverts
the projection up to the fixed-point residual of its eight evaluations, the RANSAC removes planted outliers from synthetic two-view
scenes and keeps the true matches, the gates and the degenerate outcome, and the velocities with the reference's first-two-frames quirk.
The GPU is held to the restatement in tests/test_gpu_reject.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import reject_reference as rr  # noqa: E402
import sfm_reference as sr  # noqa: E402
from test_frontend_reference import Tracker, fixture_frames  # noqa: E402


def euroc():
    return rr.Camera(**rr.EUROC)


def collinear_pair():
    """8 points on a horizontal line and the same shifted: with the EuRoC distortion no hypothesis reaches 8 inliers."""
    x = np.arange(8, dtype=np.float32) * 40 + 100
    y = np.full(8, 200, dtype=np.float32)
    return np.stack([x, y], axis=1), np.stack([x + 7, y], axis=1)


def test_lift_inverts_the_projection_up_to_the_fixed_point_residual():
    cam = euroc()
    corners = np.array([[0, 0], [751, 0], [0, 479], [751, 479]], dtype=np.float32)
    # The fixed-point residual.  The ninth iterate is m_d - d(m_u8), so project(m_u8) - p = f (m_u8 + d(m_u8) - m_d) = f (m_u8 - m_u9):
    # the round trip's error at a pixel is exactly the step the iteration would still take there, in pixels.
    # It is measured, not guessed: at the corners, and along the whole border, because the corners are not where it is largest (with
    # k1 < 0 < k2 the iteration contracts most slowly at a radius near 1, which the right edge crosses: 0.036 px at the corners,
    # 0.127 px at the middle of the right edge).
    def step(p):
        return np.abs((cam.lift(p) - cam.lift(p, evaluations=9)) * np.array([cam.fx, cam.fy])).max(axis=1)

    xs, ys = np.arange(752, dtype=np.float32), np.arange(480, dtype=np.float32)
    border = np.concatenate([np.stack([xs, 0 * xs], 1), np.stack([xs, 0 * xs + 479], 1), np.stack([0 * ys, ys], 1), np.stack([0 * ys + 751, ys], 1)])
    at_corners, residual = float(step(corners).max()), float(step(border).max())
    assert 0 < at_corners <= residual < 0.5, (at_corners, residual)      # (the reference accepts this error: its n = 8 is fixed)
    assert np.abs(np.abs(cam.project(cam.lift(corners)) - corners).max(axis=1) - step(corners)).max() <= 1e-9    # the identity
    gx, gy = np.meshgrid(np.linspace(0, 751, 48), np.linspace(0, 479, 31))
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)
    err = float(np.abs(cam.project(cam.lift(grid)) - grid.astype(np.float64)).max())
    # Margin: the first iterate's error is d(m_d), which grows with the radius, and every later one is that error contracted, so the
    # residual inside the image stays below the border's.  The identity holds up to the rounding of a few double operations on values
    # of size 1e3: 1 % of the residual plus 1e-9 px is ample.
    print("residual: corners %.3e px, border %.3e px; round trip over the grid %.3e px" % (at_corners, residual, err))
    assert err <= 1.01 * residual + 1e-9, (err, residual)
    # ... and the converged lift inverts the projection to rounding
    err64 = float(np.abs(cam.project(cam.lift(grid, evaluations=200)) - grid.astype(np.float64)).max())
    assert err64 <= 1e-9, err64


def test_distortion_and_lift_against_literal_values():
    """Values that do not come from Camera.distortion.  The first pair is PinholeCamera::distortion (PinholeCamera.cc:657-673) worked out
    by hand for (x, y) = (0.5, -0.25) with the EuRoC coefficients: r2 = 0.3125, rad = k1 r2 + k2 r2^2 = -0.08312109375,
        dx = x rad + 2 p1 x y + p2 (r2 + 2 x^2) = -0.041560546875 - 0.0000133325 - 0.0001282125     = -0.041702091875
        dy = y rad + 2 p2 x y + p1 (r2 + 2 y^2) =  0.0207802734375 + 0.00003945 + 0.000023331875    =  0.0208430553125
    (exact decimals; swapping p1 and p2 gives -0.0416747... and 0.0207782...).  The lifts are liftProjective's eight evaluations
    (:461-521) carried out in 50-digit decimal arithmetic from the same formula.  Doubles follow them to a few ulps."""
    cam = euroc()
    dx, dy = cam.distortion(np.float64(0.5), np.float64(-0.25))
    assert abs(dx - (-0.041702091875)) <= 1e-16 and abs(dy - 0.0208430553125) <= 1e-16, (dx, dy)
    got = cam.lift(np.array([[100, 50], [751, 479]], dtype=np.float32))
    want = np.array([[-0.6869600032062430374, -0.5190557286407535230], [1.13432621761350306669, 0.67660058858520892654]])
    assert np.abs(got - want).max() <= 1e-14, got - want


def test_zero_distortion_is_exact():
    cam = rr.Camera(460.0, 460.0, 320.0, 240.0, width=640, height=480)        # VM/config/vio_simulation.yaml
    assert cam.no_distortion and not euroc().no_distortion
    rng = np.random.RandomState(3)
    p = rng.uniform(0, 640, (500, 2)).astype(np.float32)
    want = np.stack([cam.ik11 * p[:, 0].astype(np.float64) + cam.ik13, cam.ik22 * p[:, 1].astype(np.float64) + cam.ik23], axis=1)
    assert cam.lift(p).tobytes() == want.tobytes()
    assert cam.lift(p, evaluations=1).tobytes() == want.tobytes()              # (no iteration runs)
    assert np.abs(cam.project(cam.lift(p)) - p).max() <= 1e-10
    # one non-zero coefficient switches the iteration on
    assert not rr.Camera(460.0, 460.0, 320.0, 240.0, p2=1e-9).no_distortion


def true_line_distance(cam, cur, clean, forw):
    """The distance of every forw point from the epipolar line of its cur point, in virtual pixels, under the model of the clean matches."""
    a = rr.virtual_pixels(cam, cur).astype(np.float64)
    Fm = sr.eight_point(a, rr.virtual_pixels(cam, clean).astype(np.float64))
    b = rr.virtual_pixels(cam, forw).astype(np.float64)
    A = Fm[0, 0] * a[:, 0] + Fm[0, 1] * a[:, 1] + Fm[0, 2]
    B = Fm[1, 0] * a[:, 0] + Fm[1, 1] * a[:, 1] + Fm[1, 2]
    Cc = Fm[2, 0] * a[:, 0] + Fm[2, 1] * a[:, 1] + Fm[2, 2]
    return np.abs(b[:, 0] * A + b[:, 1] * B + Cc) / np.sqrt(A * A + B * B)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_planted_outliers_are_rejected(vio, seed):
    cam = euroc()
    cur, forw, planted, clean = rr.two_view_scene(cam, seed=seed, n=150, outlier_share=0.2, noise_px=0.1)
    assert planted.sum() == 30
    r = rr.reject(cam, cur, forw, pair=seed)
    assert r["status"] == rr.OK and r["n_inliers"] == r["mask"].sum()
    d = true_line_distance(cam, cur, clean, forw)
    gross = planted & (d > 3.0)
    assert gross.sum() >= 20, gross.sum()                    # (most planted points are far from their lines)
    assert not r["mask"][gross].any(), np.nonzero(r["mask"] & gross)[0]
    kept = r["mask"][~planted].mean()
    print("seed %d: %d gross outliers rejected, %.1f %% of the true matches kept, margin %.2e" % (seed, gross.sum(), 100 * kept, r["margin"]))
    assert kept >= 0.95, kept


def test_size_gate():
    cam = euroc()
    cur, forw = collinear_pair()
    r = rr.reject(cam, cur[:7], forw[:7] + 50.0)
    assert (r["status"], r["hyp"], r["n_inliers"]) == (rr.OK, -1, 7) and r["mask"].all() and np.isnan(r["F"]).all()
    r = rr.reject(cam, cur[:0], forw[:0])
    assert (r["status"], r["hyp"], r["n_inliers"]) == (rr.OK, -1, 0) and r["mask"].shape == (0,)
    bad = cur.copy()
    bad[3, 1] = np.nan
    r = rr.reject(cam, bad, forw)
    assert r["status"] == rr.NOT_FINITE and not r["mask"].any()


def test_no_model_keeps_every_pair():
    cam = euroc()
    cur, forw = collinear_pair()
    r = rr.reject(cam, cur, forw, pair=3)
    assert r["status"] == rr.FAIL_NO_MODEL and r["mask"].all() and r["n_inliers"] == 8 and r["hyp"] >= 0 and np.isnan(r["F"]).all()
    assert r["margin"] >= 1e-6


def test_velocity():
    cam = euroc()
    rng = np.random.RandomState(5)
    pts = rng.uniform(50, 400, (6, 2)).astype(np.float32)
    prev_px = pts + rng.uniform(-3, 3, pts.shape).astype(np.float32)
    prev_un = rr.un_points(cam, prev_px)
    un = rr.un_points(cam, pts)
    assert un.dtype == np.float32 and np.array_equal(un, cam.lift(pts).astype(np.float32))
    ids = np.array([7, 3, -1, 11, 3, 5], dtype=np.int64)
    prev_ids = np.array([3, 5, 7, -1, 3], dtype=np.int64)      # 11 is missing; 3 is there twice: the first counts
    got_un, vel = rr.undistort(cam, pts, ids, prev_ids, prev_un[:5], dt=0.05)
    assert np.array_equal(got_un, un) and vel.dtype == np.float32
    for k, j in ((0, 2), (1, 0), (4, 0), (5, 1)):                # matched
        want = ((un[k].astype(np.float64) - prev_un[j].astype(np.float64)) / 0.05).astype(np.float32)
        assert np.array_equal(vel[k], want) and np.any(vel[k] != 0)
    assert np.all(vel[2] == 0) and np.all(vel[3] == 0)          # id -1 (although -1 is among prev_ids) and unmatched
    _, vel0 = rr.undistort(cam, pts, ids)                       # m == 0
    assert np.all(vel0 == 0) and vel0.shape == (6, 2)
    with pytest.raises(ValueError):
        rr.undistort(cam, pts, ids, prev_ids, prev_un[:5], dt=0.0)


def test_first_two_frames_have_no_velocity(vio):
    """A point detected in frame t has velocity zero in t and t + 1 (its id was -1 when frame t's points were stored) and a velocity
    from t + 2 on."""
    frames = fixture_frames() + [fixture_frames()[1]]
    ft = vio.FeatureTracker(Tracker(), dr.Detector(), max_cnt=40, min_dist=30, rejecter=rr.Rejecter(euroc()))
    seen = {}
    for t, img in enumerate(frames):
        out = ft.read_image(img, 0.1 * t)
        ids = ft.update_ids()
        for i, c, v in zip(ids.tolist(), out["track_cnt"].tolist(), out["velocity"]):
            seen.setdefault(i, []).append((c, v.copy()))
    old = [h for h in seen.values() if len(h) >= 3]
    assert len(old) >= 10
    moving = 0
    for h in old:
        assert [c for c, _ in h] == list(range(1, len(h) + 1))
        assert np.all(h[0][1] == 0) and np.all(h[1][1] == 0)
        moving += bool(np.any(h[2][1] != 0))
    assert moving >= 0.9 * len(old)
