"""numpy restatement of spaceToPlane (include/vio_camera_project.h, csrc/vio_camera_project_math.h) on top of
camera_reference.py, which has the library's sin, cos and atan2 and the four cameras:

  project             the pixel and the flag byte of every point through a camera_reference.Camera, in the header's operation order:
                      elementwise double arithmetic, so the device and the host build agree with it in every bit
  project_exact       the reference's formulas as written (PinholeCamera.cc:531-553, CataCamera.cc:636-659, ScaramuzzaCamera.cc:632-653,
                      EquidistantCamera.cc:451-461, with acos and atan2) at 50 digits (mpmath) on the same double inputs
  fit_inv_poly        ScaramuzzaCamera.cc:538-570: the least-squares polynomial rho(theta) of a camera's poly
  rays_to             points along rays of given polar angles, the accuracy test's inputs
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_reference as cr  # noqa: E402

D = np.float64
INV_POLY_MAX = 20
NOT_FINITE, BEHIND = 1, 2
PROJECT_C = 3e-13                 # VIO_CAMERA_PROJECT_C, pixels


def _distort(pin, x, y):
    if pin.no_distortion:
        return x, y
    dx, dy = pin.distortion(x, y)
    return x + dx, y + dy


def project(cam, points, inv_poly=None):
    """(pixels (n, 2) float64, flags (n,) uint8) of points (n, 3) through `cam`; inv_poly: SCARAMUZZA's coefficients (1 to 20)."""
    P = np.asarray(points, dtype=D).reshape(-1, 3)
    P0, P1, P2 = P[:, 0], P[:, 1], P[:, 2]
    n = len(P)
    flags = np.zeros(n, dtype=np.uint8)
    with np.errstate(all="ignore"):
        if cam.model == cr.MODEL_PINHOLE:
            x, y = _distort(cam.pin, P0 / P2, P1 / P2)
            u, v = cam.pin.fx * x + cam.pin.cx, cam.pin.fy * y + cam.pin.cy
            flags[~(P2 > 0.0)] |= BEHIND
        elif cam.model == cr.MODEL_MEI:
            a, b, c = P0 * P0, P1 * P1, P2 * P2
            z = P2 + cam.xi * np.sqrt((a + b) + c)
            x, y = _distort(cam.pin, P0 / z, P1 / z)
            u, v = cam.pin.fx * x + cam.pin.cx, cam.pin.fy * y + cam.pin.cy
            flags[~(z > 0.0)] |= BEHIND
        elif cam.model == cr.MODEL_SCARAMUZZA:
            if inv_poly is None or not 1 <= len(inv_poly) <= INV_POLY_MAX:
                raise ValueError("a SCARAMUZZA camera needs 1 to %d inv_poly coefficients" % INV_POLY_MAX)
            coef = [D(c) for c in inv_poly] + [D(0.0)] * (INV_POLY_MAX - len(inv_poly))
            a, b = P0 * P0, P1 * P1
            norm = np.sqrt(a + b)
            theta = cr.cam_atan2(-P2, norm)
            rho, theta_i = np.zeros(n), np.ones(n)
            for i in range(INV_POLY_MAX):
                rho = rho + theta_i * coef[i]
                theta_i = theta_i * theta
            inv_norm = 1.0 / norm
            xn0, xn1 = P0 * inv_norm * rho, P1 * inv_norm * rho
            u = xn0 * cam.ac + xn1 * cam.ad + cam.cx
            v = xn0 * cam.ae + xn1 + cam.cy
        else:
            a, b = P0 * P0, P1 * P1
            theta = cr.cam_atan2(np.sqrt(a + b), P2)
            phi = cr.cam_atan2(P1, P0)
            r = cr.kb_r(cam.k, theta)
            x, y = r * cr.cam_cos(phi), r * cr.cam_sin(phi)
            u, v = cam.pin.fx * x + cam.pin.cx, cam.pin.fy * y + cam.pin.cy
        bad = ~(np.isfinite(P0) & np.isfinite(P1) & np.isfinite(P2) & np.isfinite(u) & np.isfinite(v))
    flags[bad] |= NOT_FINITE
    pix = np.stack([np.where(bad, np.nan, u), np.where(bad, np.nan, v)], axis=1)
    return pix, flags


def project_exact(cam, points, inv_poly=None, dps=50):
    """The reference's spaceToPlane as written, at `dps` digits, of points (n, 3) (doubles, taken exactly): a list of (u, v) mpmath
    pairs.  KANNALA_BRANDT takes theta = acos(P2 / |P|), SCARAMUZZA atan2, as the reference does."""
    import mpmath
    P = np.asarray(points, dtype=D).reshape(-1, 3)
    out = []
    with mpmath.workdps(dps):
        m = lambda v: mpmath.mpf(float(v))
        for p in P:
            P0, P1, P2 = m(p[0]), m(p[1]), m(p[2])
            if cam.model in (cr.MODEL_PINHOLE, cr.MODEL_MEI):
                c = cam.pin
                z = P2 if cam.model == cr.MODEL_PINHOLE else P2 + m(cam.xi) * mpmath.sqrt(P0 * P0 + P1 * P1 + P2 * P2)
                x, y = P0 / z, P1 / z
                if not c.no_distortion:
                    k1, k2, p1, p2 = m(c.k1), m(c.k2), m(c.p1), m(c.p2)
                    mx2, my2, mxy = x * x, y * y, x * y
                    rho2 = mx2 + my2
                    rad = k1 * rho2 + k2 * rho2 * rho2
                    dx = x * rad + 2 * p1 * mxy + p2 * (rho2 + 2 * mx2)
                    dy = y * rad + 2 * p2 * mxy + p1 * (rho2 + 2 * my2)
                    x, y = x + dx, y + dy
                out.append((m(c.fx) * x + m(c.cx), m(c.fy) * y + m(c.cy)))
            elif cam.model == cr.MODEL_SCARAMUZZA:
                norm = mpmath.sqrt(P0 * P0 + P1 * P1)
                theta = mpmath.atan2(-P2, norm)
                rho = sum((theta ** i * m(ci) for i, ci in enumerate(inv_poly)), mpmath.mpf(0))
                xn0, xn1 = P0 / norm * rho, P1 / norm * rho
                out.append((xn0 * m(cam.ac) + xn1 * m(cam.ad) + m(cam.cx), xn0 * m(cam.ae) + xn1 + m(cam.cy)))
            else:
                theta = mpmath.acos(P2 / mpmath.sqrt(P0 * P0 + P1 * P1 + P2 * P2))
                phi = mpmath.atan2(P1, P0)
                k = [m(v) for v in cam.k]
                t = theta * theta
                r = theta * (1 + t * (k[0] + t * (k[1] + t * (k[2] + t * k[3]))))
                c = cam.pin
                out.append((m(c.fx) * r * mpmath.cos(phi) + m(c.cx), m(c.fy) * r * mpmath.sin(phi) + m(c.cy)))
    return out


def max_error(pix, exact, dps=50):
    """The largest |pix - exact| over both coordinates, in pixels, as a float."""
    import mpmath
    with mpmath.workdps(dps):
        return max(float(abs(mpmath.mpf(float(p[k])) - e[k])) for p, e in zip(np.asarray(pix, dtype=D), exact) for k in (0, 1))


def fit_inv_poly(cam, order=4):
    """ScaramuzzaCamera.cc:538-570: rho over [0, (width + height) / 2] in steps of 0.1, z = poly(rho), the angle of each sample, and
    the least-squares polynomial of degree `order` of rho in that angle.  The angle is atan2(z, rho), the one spaceToPlane computes for
    the ray liftProjective returns, (xc, -z): theta = atan2(-P2, norm) = atan2(z, rho), -pi/2 on the axis.  (The reference's fit
    writes atan2(-z, rho), the opposite sign, which its own spaceToPlane does not invert.)  Returns the order + 1 coefficients, lowest
    power first."""
    rou = np.arange(0.0, (cam.width + cam.height) / 2 + 1e-9, 0.1)
    z = sum(float(c) * rou ** k for k, c in enumerate(cam.poly))
    theta = np.arctan2(z, rou)
    V = np.vander(theta, order + 1, increasing=True)
    coef, *_ = np.linalg.lstsq(V, rou, rcond=None)
    return [float(c) for c in coef]


def theta_max_of(cam, inv_poly=None):
    """The polar angle (from the optical axis) up to which the accuracy test sends rays through `cam`: KANNALA_BRANDT's theta_max; for
    the other models the angle of the frame's inscribed circle, from the restatement's own lift."""
    if cam.model == cr.MODEL_KANNALA_BRANDT:
        return float(cam.theta_max)
    c = cr.centre(cam)
    r = 0.98 * cr.field_radius(cam)
    ray = cam.lift(np.array([[c[0] + r, c[1]]]))["rays"][0]
    return float(np.arctan2(np.hypot(ray[0], ray[1]), ray[2]))


def rays_to(cam, theta_max, n_theta=48, n_phi=7, seed=0):
    """Points (m, 3) along rays from the axis to polar angle theta_max (both included), a few azimuths each, at random depths: the
    accuracy test's inputs."""
    rng = np.random.RandomState(seed)
    th = np.concatenate([[0.0, 1e-12, 1e-9, 1e-6, 1e-3], np.linspace(0.0, theta_max, n_theta)[1:]])
    ph = np.concatenate([[0.0, np.pi / 2, np.pi, -np.pi / 2], rng.uniform(-np.pi, np.pi, n_phi - 4)])
    T, F = [a.reshape(-1) for a in np.meshgrid(th, ph, indexing="ij")]
    d = rng.uniform(0.5, 20.0, len(T))
    P = np.stack([np.sin(T) * np.cos(F), np.sin(T) * np.sin(F), np.cos(T)], axis=1) * d[:, None]
    P[T == 0.0, 0:2] = 0.0                          # onto the axis exactly
    return P
