"""tests/camera_reference.py against itself and against closed forms: the PINHOLE restatement is reject_reference's, MEI without a
mirror is the pinhole, npow follows the zero coefficients, KANNALA_BRANDT's lift inverts the closed-form forward model, and on the
tests' cameras and points the reference's own root selection picks the root the library solves for."""
import os
import sys

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_reference as cr  # noqa: E402
import reject_reference as rr  # noqa: E402


def grid_points(w, h, seed=3, n=400):
    rng = np.random.RandomState(seed)
    return np.concatenate([[[0, 0], [w - 1, h - 1], [w / 2.0, h / 2.0]], rng.uniform(0, 1, (n, 2)) * [w, h]]).astype(np.float32)


def test_pinhole_equals_the_reject_restatement_bit_for_bit():
    cam, ref = cr.Camera(**cr.EUROC), rr.Camera(**rr.EUROC)
    pts = grid_points(752, 480)
    rays = cam.lift(pts)["rays"]
    assert rays[:, :2].tobytes() == ref.lift(pts).tobytes() and np.all(rays[:, 2] == 1.0)
    assert cr.virtual_pixels(cam, pts).tobytes() == rr.virtual_pixels(ref, pts).tobytes()
    assert cr.un_points(cam, pts).tobytes() == rr.un_points(ref, pts).tobytes()
    ids = np.arange(len(pts), dtype=np.int64)
    prev = (rr.un_points(ref, pts) + np.float32(0.02)).astype(np.float32)
    un, vel, st = cr.undistort(cam, pts, ids, ids[::-1], prev, dt=0.05)
    un_r, vel_r = rr.undistort(ref, pts, ids, ids[::-1], prev, dt=0.05)
    assert st == cr.OK and un.tobytes() == un_r.tobytes() and vel.tobytes() == vel_r.tobytes()
    a, b, _, _ = rr.two_view_scene(ref, seed=1, n=60)
    mine, theirs = cr.reject(cam, a, b, pair=4), rr.reject(ref, a, b, pair=4)
    for k in ("status", "hyp", "n_inliers"):
        assert mine[k] == theirs[k], k
    assert mine["mask"].tobytes() == theirs["mask"].tobytes() and mine["F"].tobytes() == theirs["F"].tobytes()


def test_mei_without_mirror_and_distortion_is_the_pinhole_direction():
    """xi = 0: z = 1 - 0 * (rho2 + 1) / (0 + sqrt(1 + rho2)) = 1 analytically, and in floating point 0 * x / y is 0 exactly, so the
    ray is (mx, my, 1): within the 2 ulp the identity is held to, it is in fact equal."""
    p = dict(model=cr.MODEL_MEI, width=752, height=480, xi=0.0, gamma1=461.6, gamma2=460.3, u0=363.0, v0=248.1)
    pts = grid_points(752, 480)
    rays = cr.Camera(**p).lift(pts)["rays"]
    pin = rr.Camera(fx=461.6, fy=460.3, cx=363.0, cy=248.1).lift(pts)
    d = np.stack([pin[:, 0], pin[:, 1], np.ones(len(pts))], axis=1)
    assert np.all(np.abs(rays / rays[:, 2:3] - d) <= 2 * np.spacing(np.abs(d)))


def test_npow_follows_the_zero_coefficients():
    assert cr.kb_npow([0.0, 0.0, 0.0, 0.0]) == 1 and cr.kb_npow([0.1, 0.0, 0.0, 0.0]) == 3 and cr.kb_npow([0.1, 0.2, 0.0, 0.0]) == 5
    assert cr.kb_npow([0.1, 0.2, 0.3, 0.0]) == 7 and cr.kb_npow([0.1, 0.2, 0.3, 0.4]) == 9
    assert cr.kb_npow([0.0, 0.2, 0.0, 0.0]) == 3            # EquidistantCamera.cc:731-747 counts every zero, not only the trailing ones
    assert [cr.Camera(**cr.KB_CAMERAS[k]).npow for k in ("four", "two", "curved")] == [9, 5, 9] and cr.Camera(**cr.KB_ZERO).npow == 1
    # npow == 1: theta = rho, bit for bit
    cam = cr.Camera(**cr.KB_ZERO)
    pts = grid_points(512, 512)
    assert cam.lift(pts)["theta"].tobytes() == cam.kb_polar(pts)[0].tobytes()


@pytest.mark.parametrize("name", sorted(cr.KB_CAMERAS))
def test_kannala_brandt_lift_inverts_the_forward_model(name):
    """Rays at chosen (theta, phi) go through r(theta) = theta + k2 theta^3 + ... and u = mu r cos(phi) + u0, v = mv r sin(phi) + v0 at
    50 digits (independent of the lift), are rounded to double pixels, and are lifted again.  The pixel's rounding moves rho by at most
    2^-53 (|u| / mu + |v| / mv) and the lift's own p_u and rho add a few roundings of that size; theta moves by that over r'(theta):
    the bound below is 8 such roundings, plus the solve's own allowance (one ulp of theta)."""
    cam = cr.Camera(**cr.KB_CAMERAS[name])
    rng = np.random.RandomState(11)
    thetas = np.concatenate([[1e-3], rng.uniform(0.02, 0.98, 30) * float(cam.theta_max)])
    phis = rng.uniform(-np.pi, np.pi, len(thetas))
    mu, mv, u0, v0 = (float(cam.p[k]) for k in ("mu", "mv", "u0", "v0"))
    pix = []
    with mpmath.workdps(50):
        for t, f in zip(thetas, phis):
            t, f = mpmath.mpf(float(t)), mpmath.mpf(float(f))
            r = t + sum(mpmath.mpf(float(k)) * t ** e for k, e in zip(cam.k, (3, 5, 7, 9)))
            pix.append([float(mu * r * mpmath.cos(f) + u0), float(mv * r * mpmath.sin(f) + v0)])
    pix = np.array(pix, dtype=np.float64)
    for solver in ("fixed", "eig", "exact"):
        out = cam.lift(pix, theta=solver)
        assert not out["clamped"].any()
        slack = 8 * 2.0 ** -53 * (np.abs(pix[:, 0]) / mu + np.abs(pix[:, 1]) / mv + 1.0) / cr.kb_dr(cam.k, thetas) + 2.0 ** -52
        extra = 1e-13 if solver == "eig" else 0.0               # (the eigenvalue method's own error, measured below at 5e-15)
        assert np.all(np.abs(out["theta"] - thetas) <= slack + extra), (solver, np.abs(out["theta"] - thetas).max(), slack.min())
        assert np.all(np.abs(np.angle(np.exp(1j * (out["phi"] - phis)))) <= 1e-12)


@pytest.mark.parametrize("name", sorted(cr.KB_CAMERAS))
def test_the_reference_method_selects_the_root_the_library_solves_for(name):
    """A condition on the tests' inputs: on every point that is not clamped, the reference's eigenvalue method with its own selection
    rule (the smallest real eigenvalue above -1e-10) returns the root in [0, theta_max], i.e. the two agree to the eigenvalue method's
    accuracy.  E_ref, its largest error, is the yardstick of the device's theta bound, so it has to be an error and not a distance
    between two different roots: 1e-12 separates the two cases by many orders of magnitude."""
    cam = cr.Camera(**cr.KB_CAMERAS[name])
    pts, n_out = cr.kb_points(cam)
    assert np.all(pts >= 0) and np.all(pts[:, 0] <= cam.width) and np.all(pts[:, 1] <= cam.height)
    keep, exact, e_ref = cr.kb_theta_errors(cam, pts)
    assert len(keep) == len(pts) - n_out and cam.lift(pts)["clamped"].sum() == n_out
    assert e_ref < 1e-12, e_ref
    assert cr.kb_monotone(cam.k, cam.theta_max)
    rho, _ = cam.kb_polar(pts)
    assert rho[0] < 1e-10 and np.all(rho[1:] > 1e-3)
    # the restated fixed-work solve stays within the issue's bound, as the host build and the device must
    fixed = cam.lift(pts)["theta"]
    with mpmath.workdps(50):
        for i, t in zip(keep, exact):
            assert abs(mpmath.mpf(float(fixed[i])) - t) <= cr.theta_bound(e_ref, t)


def test_bad_lifts_and_non_finite_pixels():
    cam = cr.Camera(model=cr.MODEL_MEI, width=512, height=512, xi=1.0, gamma1=128.0, gamma2=128.0, u0=256.0, v0=256.0)
    pts = np.array([[300.0, 256.0]] * 9 + [[384.0, 256.0]], dtype=np.float32)          # the last one lifts to z = 0
    out = cr.reject(cam, pts, pts + 1)
    assert out["status"] == cr.NOT_FINITE and not out["mask"].any() and out["n_inliers"] == 0
    un, vel, st = cr.undistort(cam, pts, np.full(10, -1))
    assert st == cr.NOT_FINITE and np.isnan(un).all() and np.isnan(vel).all()
    assert cr.reject(cam, pts[:7], pts[:7])["mask"].all()                               # the size gate comes first
