"""numpy restatement of the camera model library (include/vio_camera.h, csrc/vio_camera_math.h): liftProjective of
the reference's four camera models, and rejectWithF / undistortedPoints on top of a ray whose z is not 1.

  Camera.lift         PINHOLE: reject_reference.Camera.lift itself.  MEI: CataCamera::liftProjective
                      (VM/src/camera_models/camera_models/CataCamera.cc:556-626, m_inv_K* of :320-323, ::distortion of :766-781).
                      SCARAMUZZA: OCAMCamera::liftProjective (ScaramuzzaCamera.cc:599-621, m_inv_scale of :200).  KANNALA_BRANDT:
                      EquidistantCamera::liftProjective (EquidistantCamera.cc:428-442) over backprojectSymmetric (:716-818)
  theta solvers       KANNALA_BRANDT's root, three ways: kb_theta_eig is the reference's own method in double (the companion matrix of
                      :779-782 through numpy.linalg.eigvals, the selection of :787-816); kb_theta_exact is the root at 50 digits
                      (mpmath); kb_theta_fixed restates the library's fixed-work solve (bisections, then safeguarded Newton steps on a
                      compensated Horner residual), in every bit
  virtual_pixels      rejectWithF's un_cur_pts (VM/src/feature_tracker.cpp:180-187): focal * P0 / P2 + COL / 2.0, as float
  un_points           undistortedPoints' cur_un_pts (feature_tracker.cpp:268): P0 / P2, P1 / P2 as float
  reject, undistort   reject_reference's, over those (the RANSAC is sfm_reference's sample8, eight_point, epipolar_error)

Everything but sin, cos and atan2 is elementwise double arithmetic in the reference's order (numpy's fma-free arithmetic is what
`fp contract(off)` gives), so the device and the host build of csrc/vio_camera_math.h agree with it in every bit for PINHOLE, MEI,
SCARAMUZZA and KANNALA_BRANDT alike: the library's sin, cos and atan2 are arithmetic of its own (fdlibm's kernels), restated here
operation for operation, so no math library's last bit enters.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reject_reference as rr  # noqa: E402
import sfm_reference as sr  # noqa: E402

OK, NOT_FINITE, FAIL_NO_MODEL = rr.OK, rr.NOT_FINITE, rr.FAIL_NO_MODEL
MAX_SLOTS, MAX_PARAMS, MAX_POINTS, MAX_ITEMS = 256, 16, 4096, 4096
KB_BISECTIONS, KB_NEWTON, KB_GRID = 12, 8, 4096
KB_DEFAULT_THETA_MAX = math.pi
KB_RAY_C = 3.6
MODEL_PINHOLE, MODEL_KANNALA_BRANDT, MODEL_MEI, MODEL_SCARAMUZZA = 0, 1, 2, 3
D = np.float64


def kb_npow(k):
    """EquidistantCamera.cc:731-747: 9 less 2 for every coefficient that is zero."""
    return 9 - 2 * sum(1 for v in k if v == 0.0)


def kb_r(k, th):
    """r(theta), Horner in theta^2 (cam_kb_r)."""
    th = np.asarray(th, dtype=D)
    t = th * th
    return th * (1.0 + t * (k[0] + t * (k[1] + t * (k[2] + t * k[3]))))


def kb_dr(k, th):
    th = np.asarray(th, dtype=D)
    t = th * th
    return 1.0 + t * (3.0 * k[0] + t * (5.0 * k[1] + t * (7.0 * k[2] + t * (9.0 * k[3]))))


def kb_monotone(k, theta_max):
    """vio_camera_set's check: r' > 0 at the KB_GRID + 1 grid points of [0, theta_max]."""
    k = [D(v) for v in k]
    i = np.arange(KB_GRID + 1, dtype=D)
    return bool(np.all(kb_dr(k, D(theta_max) * i / KB_GRID) > 0.0))


def _two_prod_err(a, b, p):
    """a * b - p exactly (what fma(a, b, -p) returns), by Dekker's splitting; a, b arrays of float64 far from overflow."""
    c = D(134217729.0)
    ah = c * a; ah = ah - (ah - a); al = a - ah
    bh = c * b; bh = bh - (bh - b); bl = b - bh
    return ((ah * bh - p) + ah * bl + al * bh) + al * bl


def kb_f(k, rho, th):
    """cam_kb_f: r(theta) - rho by the compensated Horner scheme on the degree-9 polynomial in theta."""
    rho, th = np.asarray(rho, dtype=D), np.asarray(th, dtype=D)
    a = [-rho, D(1.0), D(0.0), k[0], D(0.0), k[1], D(0.0), k[2], D(0.0), k[3]]
    s, c = np.broadcast_to(a[9], th.shape).astype(D), np.zeros(th.shape, dtype=D)
    for i in range(8, -1, -1):
        p = s * th
        pe = _two_prod_err(s, th, p)
        sn = p + a[i]
        bb = sn - p
        se = (p - (sn - bb)) + (a[i] - bb)
        c = c * th + (pe + se)
        s = sn
    return s + c


def kb_theta_fixed(k, theta_max, rho):
    """cam_kb_solve, elementwise over rho (rho <= r(theta_max))."""
    k = [D(v) for v in k]
    rho = np.asarray(rho, dtype=D).reshape(-1)
    with np.errstate(all="ignore"):
        lo, hi = np.zeros_like(rho), np.full_like(rho, D(theta_max))
        for _ in range(KB_BISECTIONS):
            mid = 0.5 * (lo + hi)
            neg = kb_f(k, rho, mid) <= 0.0
            lo, hi = np.where(neg, mid, lo), np.where(neg, hi, mid)
        th = 0.5 * (lo + hi)
        was_out = np.zeros(rho.shape, dtype=bool)
        for _ in range(KB_NEWTON):
            f = kb_f(k, rho, th)
            neg = f <= 0.0
            lo, hi = np.where(neg, th, lo), np.where(neg, hi, th)
            nx = th - f / kb_dr(k, th)
            out = ~((nx >= lo) & (nx <= hi))
            th = np.where(out, np.where(was_out, 0.5 * (lo + hi), np.where(nx > hi, hi, lo)), nx)
            was_out = out
    return th


def kb_theta_eig(k, rho):
    """backprojectSymmetric's own method for one rho (EquidistantCamera.cc:749-816): the eigenvalues of the companion matrix, the
    smallest real one above -tol, rho if there is none."""
    tol = 1e-10
    k = [float(v) for v in k]
    npow = kb_npow(k)
    coeffs = np.zeros(npow + 1)
    coeffs[0], coeffs[1] = -float(rho), 1.0
    for p, v in zip((3, 5, 7, 9), k):
        if npow >= p:
            coeffs[p] = v
    if npow == 1:
        return float(rho)
    A = np.zeros((npow, npow))
    A[1:, :npow - 1] = np.eye(npow - 1)
    A[:, npow - 1] = -coeffs[:npow] / coeffs[npow]
    thetas = []
    for e in np.linalg.eigvals(A):
        if abs(e.imag) > tol:
            continue
        t = float(e.real)
        if t < -tol:
            continue
        thetas.append(max(t, 0.0))
    return min(thetas) if thetas else float(rho)


def kb_theta_exact(k, theta_max, rho, dps=50):
    """The root of r(theta) = rho in [0, theta_max] as an mpmath number of `dps` digits: bisection in double for a start, then Newton
    at full precision (r' > 0 there)."""
    import mpmath
    with mpmath.workdps(dps):
        km = [mpmath.mpf(float(v)) for v in k]
        r = lambda t: t * (1 + t * t * (km[0] + t * t * (km[1] + t * t * (km[2] + t * t * km[3]))))
        dr = lambda t: 1 + t * t * (3 * km[0] + t * t * (5 * km[1] + t * t * (7 * km[2] + t * t * 9 * km[3])))
        rho = mpmath.mpf(float(rho))
        lo, hi = mpmath.mpf(0), mpmath.mpf(float(theta_max))
        for _ in range(60):
            mid = (lo + hi) / 2
            if r(mid) <= rho:
                lo = mid
            else:
                hi = mid
        t = (lo + hi) / 2
        for _ in range(8):
            t = t - (r(t) - rho) / dr(t)
        assert abs(r(t) - rho) < mpmath.mpf(10) ** (-(dps - 8)), "the exact root did not converge"
        return +t


def _ksin(x, y):
    """cam_ksin: sin(x + y) on |x| <= pi/4 (fdlibm's k_sin.c)."""
    S1, S2, S3 = D(-1.66666666666666324348e-01), D(8.33333333332248946124e-03), D(-1.98412698298579493134e-04)
    S4, S5, S6 = D(2.75573137070700676789e-06), D(-2.50507602534068634195e-08), D(1.58969099521155010221e-10)
    z = x * x
    v = z * x
    r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    return x - ((z * (0.5 * y - v * r) - y) - v * S1)


def _kcos(x, y):
    """cam_kcos: cos(x + y) on |x| <= pi/4 (fdlibm's k_cos.c)."""
    C1, C2, C3 = D(4.16666666666666019037e-02), D(-1.38888888888741095749e-03), D(2.48015872894767294178e-05)
    C4, C5, C6 = D(-2.75573143513906633035e-07), D(2.08757232129817482790e-09), D(-1.13596475577881948265e-11)
    z = x * x
    w = z * z
    r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6))
    hz = 0.5 * z
    t = 1.0 - hz
    return t + (((1.0 - t) - hz) + (z * r - x * y))


def _sincos(x):
    """(cam_sin, cam_cos) of an array: the two-step reduction by n pi/2, then the kernels by quadrant; NaN beyond 1e6 or not finite."""
    x = np.asarray(x, dtype=D)
    with np.errstate(all="ignore"):
        ok = (x >= -1e6) & (x <= 1e6)
        xs = np.where(ok, x, 0.0)
        fn = np.floor(xs * D(6.36619772367581382433e-01) + 0.5)
        t = xs - fn * D(1.57079632673412561417e+00)
        w = fn * D(6.07710050630396597660e-11)
        r = t - w
        w = fn * D(2.02226624879595063154e-21) - ((t - r) - w)
        y0 = r - w
        y1 = (r - y0) - w
        q = fn.astype(np.int64) & 3
        sn, cs = _ksin(y0, y1), _kcos(y0, y1)
        sin = np.where(q == 0, sn, np.where(q == 1, cs, np.where(q == 2, -sn, -cs)))
        cos = np.where(q == 0, cs, np.where(q == 1, -sn, np.where(q == 2, -cs, sn)))
    return np.where(ok, sin, np.nan), np.where(ok, cos, np.nan)


def cam_sin(x):
    return _sincos(x)[0]


def cam_cos(x):
    return _sincos(x)[1]


def _atan_pos(x):
    """cam_atan_pos: atan(x), x >= 0 (fdlibm's s_atan.c)."""
    T = [D(v) for v in (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
                        9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
                        4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)]
    with np.errstate(all="ignore"):
        c3, c2, c1, c0 = x >= 2.4375, x >= 1.1875, x >= 0.6875, x >= 0.4375
        hi = np.where(c3, D(1.57079632679489655800e+00), np.where(c2, D(9.82793723247329054082e-01), np.where(c1, D(7.85398163397448278999e-01),
                      np.where(c0, D(4.63647609000806093515e-01), 0.0))))
        lo = np.where(c3, D(6.12323399573676603587e-17), np.where(c2, D(1.39033110312309984516e-17), np.where(c1, D(3.06161699786838301793e-17),
                      np.where(c0, D(2.26987774529616870924e-17), 0.0))))
        t = np.where(c3, -1.0 / x, np.where(c2, (x - 1.5) / (1.0 + 1.5 * x), np.where(c1, (x - 1.0) / (x + 1.0),
                     np.where(c0, (2.0 * x - 1.0) / (2.0 + x), x))))
        z = t * t
        w = z * z
        s1 = z * (T[0] + w * (T[2] + w * (T[4] + w * (T[6] + w * (T[8] + w * T[10])))))
        s2 = w * (T[1] + w * (T[3] + w * (T[5] + w * (T[7] + w * T[9]))))
        return np.where(c0, hi - ((t * (s1 + s2) - lo) - t), t - t * (s1 + s2))


def cam_atan2(y, x):
    """cam_atan2 (fdlibm's e_atan2.c without its exponent shortcuts)."""
    y, x = np.asarray(y, dtype=D), np.asarray(x, dtype=D)
    PI, PI_LO, PI_O_2 = D(3.1415926535897931160e+00), D(1.2246467991473531772e-16), D(1.5707963267948965580e+00)
    with np.errstate(all="ignore"):
        q = y / x
        z = _atan_pos(np.where(q < 0.0, -q, q))
        gen = np.where(x > 0.0, np.where(y < 0.0, -z, z), np.where(y < 0.0, (z - PI_LO) - PI, PI - (z - PI_LO)))
        return np.where(y == 0.0, np.where(x < 0.0, PI, 0.0 * x), np.where(x == 0.0, np.where(y < 0.0, -PI_O_2, PI_O_2), gen))


class Camera:
    """One camera slot: model, width, height and the model's keywords (camera.PARAMS of the binding)."""

    def __init__(self, model=MODEL_PINHOLE, width=752, height=480, **p):
        self.model, self.width, self.height = int(model), int(width), int(height)
        self.p = {k: D(v) for k, v in p.items()}
        g = lambda name, default=None: self.p[name] if name in self.p else D(default)
        if model == MODEL_PINHOLE:
            self.pin = rr.Camera(p["fx"], p["fy"], p["cx"], p["cy"], p.get("k1", 0.0), p.get("k2", 0.0), p.get("p1", 0.0), p.get("p2", 0.0), width, height)
        elif model == MODEL_MEI:
            # m_inv_K11 .. m_inv_K23 from gamma1, gamma2, u0, v0 (CataCamera.cc:320-323): rr.Camera's constants on those
            self.pin = rr.Camera(p["gamma1"], p["gamma2"], p["u0"], p["v0"], p.get("k1", 0.0), p.get("k2", 0.0), p.get("p1", 0.0), p.get("p2", 0.0), width, height)
            self.xi = g("xi")
        elif model == MODEL_SCARAMUZZA:
            self.poly = [g("poly%d" % i, 0.0) for i in range(5)]
            self.ac, self.ad, self.ae, self.cx, self.cy = g("ac", 1.0), g("ad", 0.0), g("ae", 0.0), g("cx"), g("cy")
            self.inv_scale = D(1.0) / (self.ac - self.ad * self.ae)                    # ScaramuzzaCamera.cc:200
        elif model == MODEL_KANNALA_BRANDT:
            self.k = [g(n, 0.0) for n in ("k2", "k3", "k4", "k5")]
            self.pin = rr.Camera(p["mu"], p["mv"], p["u0"], p["v0"], width=width, height=height)
            self.theta_max = g("theta_max", KB_DEFAULT_THETA_MAX)
            self.r_max = D(kb_r(self.k, self.theta_max))
            self.npow = kb_npow(self.k)
        else:
            raise ValueError("unknown model %r" % (model,))

    def params(self):
        return dict(model=self.model, width=self.width, height=self.height, **{k: float(v) for k, v in self.p.items()})

    def kb_polar(self, pts):
        """(rho, phi) of backprojectSymmetric's p_u (EquidistantCamera.cc:433-435, :720-730)."""
        p = np.asarray(pts).reshape(-1, 2).astype(D)
        c = self.pin
        with np.errstate(all="ignore"):
            px, py = c.ik11 * p[:, 0] + c.ik13, c.ik22 * p[:, 1] + c.ik23
            rho = np.sqrt(px * px + py * py)
            phi = np.where(rho < 1e-10, 0.0, cam_atan2(py, px))
        return rho, phi

    def lift(self, pts, theta="fixed"):
        """A dict: rays (n, 3) float64, theta, phi (n,) float64 (0 unless KANNALA_BRANDT), clamped (n,) bool.  theta: "fixed" (the
        library's solve), "eig" (the reference's), "exact" (50 digits, rounded to double) or an (n,) array to use as it is."""
        p = np.asarray(pts).reshape(-1, 2).astype(D)
        n = len(p)
        th, ph, cl = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
        with np.errstate(all="ignore"):
            if self.model == MODEL_PINHOLE:
                l = self.pin.lift(p)
                rays = np.stack([l[:, 0], l[:, 1], np.ones(n)], axis=1)
            elif self.model == MODEL_MEI:
                l = self.pin.lift(p)                                                    # CataCamera.cc:562-606, n = 8
                mx, my = l[:, 0], l[:, 1]
                if self.xi == 1.0:                                                      # :610-613
                    z = (1.0 - mx * mx - my * my) / 2.0
                else:                                                                   # :616-619
                    rho2 = mx * mx + my * my
                    z = 1.0 - self.xi * (rho2 + 1.0) / (self.xi + np.sqrt(1.0 + (1.0 - self.xi * self.xi) * rho2))
                rays = np.stack([mx, my, z], axis=1)
            elif self.model == MODEL_SCARAMUZZA:
                xc0, xc1 = p[:, 0] - self.cx, p[:, 1] - self.cy                         # ScaramuzzaCamera.cc:602
                a0 = self.inv_scale * (xc0 - self.ad * xc1)                             # :606-609
                a1 = self.inv_scale * (-self.ae * xc0 + self.ac * xc1)
                phi = np.sqrt(a0 * a0 + a1 * a1)
                phi_i, z = np.ones(n), np.zeros(n)
                for i in range(5):                                                      # :615-619
                    z = z + phi_i * self.poly[i]
                    phi_i = phi_i * phi
                rays = np.stack([xc0, xc1, -z], axis=1)                                 # :621: xc, not xc_a
            else:
                rho, ph = self.kb_polar(p)
                if self.npow == 1:
                    th = rho.copy()                                                     # EquidistantCamera.cc:771-774
                else:
                    cl = rho > self.r_max
                    inside = ~cl & np.isfinite(rho)
                    if isinstance(theta, str):
                        th = np.full(n, float(self.theta_max))
                        if theta == "fixed":
                            th[inside] = kb_theta_fixed(self.k, self.theta_max, rho[inside])
                        elif theta == "eig":
                            th[inside] = [kb_theta_eig(self.k, r) for r in rho[inside]]
                        else:
                            th[inside] = [float(kb_theta_exact(self.k, self.theta_max, r)) for r in rho[inside]]
                        th[~cl & ~inside] = np.nan
                    else:
                        th = np.asarray(theta, dtype=D).reshape(n).copy()
                st = cam_sin(th)
                rays = np.stack([st * cam_cos(ph), st * cam_sin(ph), cam_cos(th)], axis=1)  # :438-440
        return dict(rays=rays, theta=th, phi=ph, clamped=cl)


def rays_of(cam, pts, rays=None):
    return cam.lift(pts)["rays"] if rays is None else np.asarray(rays, dtype=D).reshape(-1, 3)


def bad_rays(rays):
    """A lift the tracker cannot use: P0 / P2 or P1 / P2 is not finite."""
    with np.errstate(all="ignore"):
        return ~(np.isfinite(rays[:, 0] / rays[:, 2]) & np.isfinite(rays[:, 1] / rays[:, 2]))


def virtual_pixels(cam, pts, focal_length=rr.DEFAULT_FOCAL_LENGTH, rays=None):
    """feature_tracker.cpp:180-187, (n, 2) float32; rays: use these (n, 3) instead of lifting pts."""
    r = rays_of(cam, pts, rays)
    with np.errstate(all="ignore"):
        vx = D(focal_length) * r[:, 0] / r[:, 2] + cam.width / 2.0
        vy = D(focal_length) * r[:, 1] / r[:, 2] + cam.height / 2.0
        return np.stack([vx, vy], axis=1).astype(np.float32)


def un_points(cam, pts, rays=None):
    """feature_tracker.cpp:268, (n, 2) float32."""
    r = rays_of(cam, pts, rays)
    with np.errstate(all="ignore"):
        return np.stack([r[:, 0] / r[:, 2], r[:, 1] / r[:, 2]], axis=1).astype(np.float32)


def reject(cam, cur_pts, forw_pts, pair=0, cfg=None, rays=None):
    """reject_reference.reject through `cam`: status, hyp, n_inliers, F, mask, margin, and the virtual pixels `a`, `b` (n, 2) float32.
    rays: (cur rays, forw rays) to use instead of lifting (the device's own, to take its sin, cos and atan2 out of a comparison)."""
    cfg = dict(rr.DEFAULT_CFG, **(cfg or {}))
    cur = np.asarray(cur_pts, dtype=np.float32).reshape(-1, 2)
    forw = np.asarray(forw_pts, dtype=np.float32).reshape(-1, 2)
    n = len(cur)
    out = dict(status=OK, hyp=-1, n_inliers=n, F=np.full((3, 3), np.nan), mask=np.ones(n, dtype=bool), margin=np.inf, a=None, b=None)
    bad = dict(out, status=NOT_FINITE, n_inliers=0, mask=np.zeros(n, dtype=bool))
    if not (np.all(np.isfinite(cur)) and np.all(np.isfinite(forw))):
        return bad
    if n < rr.MIN_POINTS:
        return out
    rc, rf = (rays_of(cam, cur), rays_of(cam, forw)) if rays is None else (rays_of(cam, cur, rays[0]), rays_of(cam, forw, rays[1]))
    if bad_rays(rc).any() or bad_rays(rf).any():
        return bad
    a32, b32 = virtual_pixels(cam, cur, cfg["focal_length"], rc), virtual_pixels(cam, forw, cfg["focal_length"], rf)
    out.update(a=a32, b=b32)
    a, b = a32.astype(D), b32.astype(D)
    H = int(cfg["ransac_hypotheses"])
    thr = D(cfg["f_threshold"]) * D(cfg["f_threshold"])
    with np.errstate(all="ignore"):                              # (reject_reference.reject from here, in one block of hypotheses)
        sel = np.array([sr.sample8(cfg["seed"], pair, h, n) for h in range(H)])
        err = sr.epipolar_error(sr.eight_point(a[sel], b[sel]), a, b)
        cnt = (err <= thr).sum(axis=1)
        hyp = int(np.argmax(cnt))
        e = err[hyp]
        out.update(hyp=hyp, margin=float(np.abs(e / thr - 1.0).min()))
        if cnt[hyp] < rr.MIN_POINTS:
            return dict(out, status=FAIL_NO_MODEL)
        Fm = sr.eight_point(a[e <= thr], b[e <= thr])
        if not np.all(np.isfinite(Fm)):
            return dict(out, status=FAIL_NO_MODEL)
        e2 = sr.epipolar_error(Fm, a, b)
        mask = e2 <= thr
        out.update(F=Fm, mask=mask, n_inliers=int(mask.sum()), margin=min(out["margin"], float(np.abs(e2 / thr - 1.0).min())))
    return out


class _Unpointed:
    """un_points behind the attribute reject_reference.undistort reads of a camera: lift() / 1.0."""

    def __init__(self, un):
        self.un = un

    def lift(self, pts):
        return self.un.astype(D)


def undistort(cam, pts, ids, prev_ids=None, prev_un_pts=None, dt=None, rays=None):
    """(un_pts, velocity, status): reject_reference.undistort's matching and velocity over this camera's un_points."""
    r = rays_of(cam, pts, rays)
    n = len(r)
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    if not np.all(np.isfinite(p)) or bad_rays(r).any():
        return np.full((n, 2), np.nan, dtype=np.float32), np.full((n, 2), np.nan, dtype=np.float32), NOT_FINITE
    un = un_points(cam, pts, r)
    un2, vel = rr.undistort(_Unpointed(un), pts, ids, prev_ids, prev_un_pts, dt)        # ((float)(double)un / 1.0 is un)
    assert un2.tobytes() == un.tobytes()
    return un, vel, OK


class Rejecter:
    """The restatement behind the rejecter interface of frontend.FeatureTracker."""

    def __init__(self, cam, cfg=None):
        self.cam, self.cfg = cam, dict(rr.DEFAULT_CFG, **(cfg or {}))

    def reject(self, cur_pts, forw_pts, pair=0):
        return reject(self.cam, cur_pts, forw_pts, pair, self.cfg)["mask"]

    def undistort(self, pts, ids=None, prev_ids=None, prev_un_pts=None, dt=None):
        if ids is None:
            ids = np.full(len(np.asarray(pts).reshape(-1, 2)), -1, dtype=np.int64)
        return undistort(self.cam, pts, ids, prev_ids, prev_un_pts, dt)[:2]


# ---------------------------------------------------------------------------------------------------------
# the test cameras (on a 752 x 480 or a 512 x 512 frame) and their points
# ---------------------------------------------------------------------------------------------------------
EUROC = dict(model=MODEL_PINHOLE, **rr.EUROC)
MEI = dict(model=MODEL_MEI, width=752, height=480, xi=0.9, k1=-0.12, k2=0.03, p1=2e-4, p2=-3e-4, gamma1=830.0, gamma2=828.0, u0=371.5, v0=243.25)
MEI_PLAIN = dict(MEI, k1=0.0, k2=0.0, p1=0.0, p2=0.0)
MEI_XI1 = dict(MEI, xi=1.0)
SCARAMUZZA = dict(model=MODEL_SCARAMUZZA, width=512, height=512, poly0=-180.5, poly1=0.0, poly2=1.9e-3, poly3=-2.5e-6, poly4=1.1e-8,
                  ac=0.9995, ad=2.5e-4, ae=-1.5e-4, cx=255.25, cy=257.5)
KB_ZERO = dict(model=MODEL_KANNALA_BRANDT, width=512, height=512, mu=190.0, mv=190.5, u0=254.0, v0=256.5)
# four coefficients (a common fisheye calibration's size), k4 = k5 = 0 (npow == 5), and a strongly curved but monotone one whose
# derivative falls to 0.36 at theta_max
KB_FOUR = dict(model=MODEL_KANNALA_BRANDT, width=752, height=480, k2=-0.0125, k3=0.0045, k4=-0.0031, k5=0.00052, mu=150.0, mv=150.5, u0=376.0,
               v0=240.5, theta_max=1.6)
KB_TWO = dict(model=MODEL_KANNALA_BRANDT, width=512, height=512, k2=0.034, k3=-0.0071, mu=165.0, mv=165.0, u0=256.0, v0=256.0, theta_max=1.5)
KB_CURVED = dict(model=MODEL_KANNALA_BRANDT, width=512, height=512, k2=-0.18, k3=0.021, k4=-0.0012, k5=0.00003, mu=200.0, mv=200.0, u0=256.0,
                 v0=256.0, theta_max=1.25)
KB_CAMERAS = {"four": KB_FOUR, "two": KB_TWO, "curved": KB_CURVED}


def kb_points(cam, n_mid=40, seed=0):
    """Pixels (float32) of a KANNALA_BRANDT camera: the centre (rho < 1e-10), `n_mid` mid-field points, four just inside r(theta_max)
    and four just outside (they are clamped).  Returns (pts, n_outside)."""
    rng = np.random.RandomState(seed)
    mu, mv, u0, v0 = (float(cam.p[k]) for k in ("mu", "mv", "u0", "v0"))
    r_max = float(cam.r_max)
    ang = rng.uniform(-np.pi, np.pi, n_mid)
    rad = rng.uniform(0.02, 0.97, n_mid) * r_max
    mid = np.stack([u0 + mu * rad * np.cos(ang), v0 + mv * rad * np.sin(ang)], axis=1)
    ea = np.array([0.3, 1.9, -2.2, -0.6])
    inside = np.stack([u0 + mu * 0.9995 * r_max * np.cos(ea), v0 + mv * 0.9995 * r_max * np.sin(ea)], axis=1)
    outside = np.stack([u0 + mu * 1.0005 * r_max * np.cos(ea), v0 + mv * 1.0005 * r_max * np.sin(ea)], axis=1)
    pts = np.concatenate([[[u0, v0]], mid, inside, outside]).astype(np.float32)
    return pts, len(outside)


def kb_theta_errors(cam, pts):
    """For the points of `pts` that are not clamped: (exact thetas as mpmath numbers, E_ref): E_ref is the largest error of the
    reference's own method (kb_theta_eig) against the exact root, the yardstick of the theta bound."""
    import mpmath
    rho, _ = cam.kb_polar(pts)
    keep = np.nonzero(~(rho > cam.r_max))[0]
    exact = [kb_theta_exact(cam.k, cam.theta_max, rho[i]) for i in keep]
    with mpmath.workdps(50):
        e_ref = max(float(abs(mpmath.mpf(kb_theta_eig(cam.k, rho[i])) - t)) for i, t in zip(keep, exact))
    return keep, exact, e_ref


def theta_bound(e_ref, theta):
    """The issue's bound on the device's theta error: 2 E_ref + 2^-52 max(theta, 1)."""
    return 2.0 * e_ref + 2.0 ** -52 * max(float(theta), 1.0)


# ---------------------------------------------------------------------------------------------------------
# two views of one scene through any of the cameras (test scaffolding: the library has no spaceToPlane)
# ---------------------------------------------------------------------------------------------------------
def centre(cam):
    k = {MODEL_PINHOLE: ("cx", "cy"), MODEL_MEI: ("u0", "v0"), MODEL_SCARAMUZZA: ("cx", "cy"), MODEL_KANNALA_BRANDT: ("u0", "v0")}[cam.model]
    return np.array([float(cam.p[k[0]]), float(cam.p[k[1]])])


def field_radius(cam):
    """The radius around the centre that is inside the frame and, for KANNALA_BRANDT with coefficients, inside r(theta_max)."""
    c = centre(cam)
    r = min(c[0], c[1], cam.width - c[0], cam.height - c[1])
    if cam.model == MODEL_KANNALA_BRANDT and cam.npow > 1:
        r = min(r, 0.98 * float(cam.r_max) * min(float(cam.p["mu"]), float(cam.p["mv"])))
    return float(r)


def _polar(rays):
    return np.arctan2(np.hypot(rays[:, 0], rays[:, 1]), rays[:, 2])


def project_radially(cam, dirs, r_hi):
    """Pixels whose lifted rays point along `dirs` (n, 3): the pixel lies at the ray's azimuth from the centre, at the radius where the
    lift's polar angle is the ray's, found by 50 bisections over [0, r_hi] on the restatement's own lift.  Exact for the models that
    are symmetric about the centre; tangential distortion and the affine part enter as a small displacement, which a test scene
    takes as noise."""
    dirs = np.asarray(dirs, dtype=D)
    az, want = np.arctan2(dirs[:, 1], dirs[:, 0]), _polar(dirs)
    c = centre(cam)
    lo, hi = np.zeros(len(dirs)), np.full(len(dirs), float(r_hi))
    unit = np.stack([np.cos(az), np.sin(az)], axis=1)
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        small = _polar(cam.lift(c + mid[:, None] * unit, theta="eig" if cam.model == MODEL_KANNALA_BRANDT and cam.npow > 1 else "fixed")["rays"]) < want
        lo, hi = np.where(small, mid, lo), np.where(small, hi, mid)
    return c + (0.5 * (lo + hi))[:, None] * unit


def two_view_scene(cam, n=150, seed=0, outlier_share=0.2, noise_px=0.1, r_frac=0.8):
    """Matched pixels (cur, forw), float32 (n, 2): landmarks seen through `cam` from two poses a small motion apart, pixel noise on
    both, `outlier_share` of forw replaced by random pixels."""
    rng = np.random.RandomState(2000 + seed)
    c = centre(cam)
    r_hi = r_frac * field_radius(cam)
    rad, ang = r_hi * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(-np.pi, np.pi, n)
    cur = c + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    rays = cam.lift(cur, theta="eig" if cam.model == MODEL_KANNALA_BRANDT and cam.npow > 1 else "fixed")["rays"]
    P = rays / np.linalg.norm(rays, axis=1, keepdims=True) * rng.uniform(3.0, 9.0, (n, 1))
    w = np.array([0.01, -0.015, 0.02])
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + K + 0.5 * K @ K
    P2 = (P - np.array([0.25, 0.05, 0.1])) @ R.T
    forw = project_radially(cam, P2, r_hi / r_frac)
    cur = cur + rng.normal(0.0, noise_px, cur.shape)
    forw = forw + rng.normal(0.0, noise_px, forw.shape)
    out = rng.choice(n, int(round(outlier_share * n)), replace=False)
    forw[out] = c + rng.uniform(-r_hi, r_hi, (len(out), 2)) * 0.7
    return cur.astype(np.float32), forw.astype(np.float32)
