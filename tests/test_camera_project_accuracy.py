"""The accuracy of spaceToPlane as the library computes it (tests/camera_project_reference.py, which the host build and the device equal
bit for bit) against the reference's formulas as written, evaluated at 50 digits (mpmath) on the same double inputs: acos for
KANNALA_BRANDT's theta, atan2 for SCARAMUZZA's, the camodocal operation order otherwise.  Inputs: rays from the axis (onto it, and
1e-12 .. 1e-3 rad beside it) to the slot's theta_max (KANNALA_BRANDT's own; for the other models the polar angle of the frame's
inscribed circle), seven azimuths each, at depths of 0.5 to 20.

The bound is VIO_CAMERA_PROJECT_C pixels, VIO_CAMERA_KB_RAY_C's procedure: the largest error measured here, doubled and rounded up.
Measured (printed by the test): pinhole 7.8e-14, mei 8.0e-14, scaramuzza 8.6e-14, kb_zero (theta_max = pi, pixels to 600) 1.38e-13,
kb_four 9.8e-14, kb_two 1.13e-13, kb_curved 5.2e-14: the largest is 1.38e-13, about one unit in the last place of a pixel coordinate of
600; doubled and rounded up, 3e-13.

The round trip project(lift(pixel)) is printed and not bounded: its error is the lift's (the eight-evaluation recursion of PINHOLE and
MEI, KANNALA_BRANDT's root) and, for SCARAMUZZA, the degree-4 fit of inv_poly to poly (about a pixel)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_project_reference as cp  # noqa: E402
import camera_reference as cr  # noqa: E402

CAMERAS = [("pinhole", cr.EUROC), ("mei", cr.MEI), ("scaramuzza", cr.SCARAMUZZA), ("kb_zero", cr.KB_ZERO), ("kb_four", cr.KB_FOUR),
           ("kb_two", cr.KB_TWO), ("kb_curved", cr.KB_CURVED)]


@pytest.mark.parametrize("name,params", CAMERAS, ids=[c[0] for c in CAMERAS])
def test_pixels_against_fifty_digits(name, params):
    cam = cr.Camera(**params)
    inv = cp.fit_inv_poly(cam) if cam.model == cr.MODEL_SCARAMUZZA else None
    theta_max = cp.theta_max_of(cam)
    P = cp.rays_to(cam, theta_max)
    polar = np.arctan2(np.hypot(P[:, 0], P[:, 1]), P[:, 2])
    assert polar.min() == 0.0 and abs(polar.max() - theta_max) < 1e-12
    pix, flags = cp.project(cam, P, inv)
    on_axis = (P[:, 0] == 0) & (P[:, 1] == 0)
    if cam.model == cr.MODEL_SCARAMUZZA:                    # norm = 0 there: no finite pixel, here and in the reference
        assert np.array_equal(flags != 0, on_axis) and np.all(flags[on_axis] == cp.NOT_FINITE)
    else:
        assert not flags.any()
    ok = flags == 0
    err = cp.max_error(pix[ok], cp.project_exact(cam, P[ok], inv))
    c = cr.centre(cam)
    px = (c + np.random.RandomState(1).uniform(-0.6, 0.6, (60, 2)) * cr.field_radius(cam)).astype(np.float32)
    back, bf = cp.project(cam, cam.lift(px)["rays"], inv)
    print("%s: theta_max %.4f, %d rays, largest pixel error %.3e (bound %.1e); round trip project(lift(pixel)) %.3e px"
          % (name, theta_max, int(ok.sum()), err, cp.PROJECT_C, float(np.max(np.abs(back - px)))))
    assert not bf.any()
    assert err <= cp.PROJECT_C


def test_inv_poly_fit_inverts_the_lift():
    """fit_inv_poly's sign: spaceToPlane of a lifted ray comes back within the fit's error, about a pixel (it would not with the
    opposite sign of theta)."""
    cam = cr.Camera(**cr.SCARAMUZZA)
    inv = cp.fit_inv_poly(cam)
    assert len(inv) == 5
    c = cr.centre(cam)
    px = (c + np.random.RandomState(2).uniform(-0.6, 0.6, (60, 2)) * cr.field_radius(cam)).astype(np.float32)
    back, _ = cp.project(cam, cam.lift(px)["rays"], inv)
    assert np.max(np.abs(back - px)) < 3.0
