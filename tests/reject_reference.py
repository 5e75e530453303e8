"""numpy restatement of rejectWithF and undistortedPoints (include/vio_reject.h, csrc/vio_reject.hip).

  Camera          the reference's PINHOLE model: lift() is PinholeCamera::liftProjective with ::distortion
                  (VM/src/camera_models/camera_models/PinholeCamera.cc:461-521, :657-673), project() is ::spaceToPlane (:562-619)
  reject()        FeatureTracker::rejectWithF (VM/src/feature_tracker.cpp:169-202), cv::findFundamentalMat replaced by the RANSAC of
                  include/vio_sfm.h: sample8, eight_point, epipolar_error and the Jacobi are tests/sfm_reference.py's, not copies
  undistort()     FeatureTracker::undistortedPoints (:258-306)
  Rejecter        both behind the interface frontend.FeatureTracker takes as `rejecter`

The lift is elementwise double arithmetic in the reference's operation order, so the device and the host build of
csrc/vio_reject_math.h agree with it in every bit.  The fit's sums are sfm_reference's (numpy's summation order), which the device
follows only to rounding: reject() reports `margin`, the smallest relative distance of any winner's error to the gate before and after
the refit, and a comparison of masks is meaningful where it is well above rounding.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfm_reference as sr  # noqa: E402

OK, NOT_FINITE, FAIL_NO_MODEL = 0, -3, 1
MAX_POINTS, MAX_ITEMS, MAX_HYPOTHESES, DEFAULT_HYPOTHESES = 4096, 4096, 4096, 128
DEFAULT_F_THRESHOLD, DEFAULT_FOCAL_LENGTH = 1.0, 460.0
LIFT_EVALUATIONS, MIN_POINTS = 8, 8
ROUND, THREADS, ID_CHUNK = 64, 256, 1024
DEFAULT_CFG = dict(seed=0, ransac_hypotheses=DEFAULT_HYPOTHESES, f_threshold=DEFAULT_F_THRESHOLD, focal_length=DEFAULT_FOCAL_LENGTH)
# VM/config/euroc_config.yaml:11-22
EUROC = dict(fx=4.616e+02, fy=4.603e+02, cx=3.630e+02, cy=2.481e+02, k1=-2.917e-01, k2=8.228e-02, p1=5.333e-05, p2=-1.578e-04,
             width=752, height=480)


class Camera:
    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, width=752, height=480):
        self.fx, self.fy, self.cx, self.cy = (np.float64(v) for v in (fx, fy, cx, cy))
        self.k1, self.k2, self.p1, self.p2 = (np.float64(v) for v in (k1, k2, p1, p2))
        self.width, self.height = int(width), int(height)
        self.ik11, self.ik13 = np.float64(1.0) / self.fx, -self.cx / self.fx
        self.ik22, self.ik23 = np.float64(1.0) / self.fy, -self.cy / self.fy
        self.no_distortion = bool(self.k1 == 0.0 and self.k2 == 0.0 and self.p1 == 0.0 and self.p2 == 0.0)

    def params(self):
        return dict(fx=float(self.fx), fy=float(self.fy), cx=float(self.cx), cy=float(self.cy), k1=float(self.k1), k2=float(self.k2),
                    p1=float(self.p1), p2=float(self.p2), width=self.width, height=self.height)

    def distortion(self, x, y):
        mx2, my2, mxy = x * x, y * y, x * y
        rho2 = mx2 + my2
        rad = self.k1 * rho2 + self.k2 * rho2 * rho2
        dx = x * rad + 2.0 * self.p1 * mxy + self.p2 * (rho2 + 2.0 * mx2)
        dy = y * rad + 2.0 * self.p2 * mxy + self.p1 * (rho2 + 2.0 * my2)
        return dx, dy

    def lift(self, pts, evaluations=LIFT_EVALUATIONS):
        """(n, 2) float64 (x, y) of the rays (x, y, 1) of the pixels pts (n, 2)."""
        p = np.asarray(pts).reshape(-1, 2).astype(np.float64)
        with np.errstate(all="ignore"):
            mx_d, my_d = self.ik11 * p[:, 0] + self.ik13, self.ik22 * p[:, 1] + self.ik23
            x, y = mx_d, my_d
            if not self.no_distortion:
                dx, dy = self.distortion(mx_d, my_d)
                x, y = mx_d - dx, my_d - dy
                for _ in range(1, evaluations):
                    dx, dy = self.distortion(x, y)
                    x, y = mx_d - dx, my_d - dy
        return np.stack([x, y], axis=1)

    def project(self, xy):
        """spaceToPlane of the rays (x, y, 1): pixels (n, 2) float64."""
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        x, y = xy[:, 0], xy[:, 1]
        if not self.no_distortion:
            dx, dy = self.distortion(x, y)
            x, y = x + dx, y + dy
        return np.stack([self.fx * x + self.cx, self.fy * y + self.cy], axis=1)


def virtual_pixels(cam, pts, focal_length=DEFAULT_FOCAL_LENGTH):
    """rejectWithF's un_cur_pts / un_forw_pts (feature_tracker.cpp:179-187): cv::Point2f, here (n, 2) float32."""
    l = cam.lift(pts)
    with np.errstate(all="ignore"):
        vx = np.float64(focal_length) * l[:, 0] / 1.0 + cam.width / 2.0
        vy = np.float64(focal_length) * l[:, 1] / 1.0 + cam.height / 2.0
        return np.stack([vx, vy], axis=1).astype(np.float32)


def un_points(cam, pts):
    """undistortedPoints' cur_un_pts (feature_tracker.cpp:268): (n, 2) float32."""
    with np.errstate(all="ignore"):
        return (cam.lift(pts) / 1.0).astype(np.float32)


def reject(cam, cur_pts, forw_pts, pair=0, cfg=None, perturb=None):
    """A dict: status, hyp, n_inliers, F (3, 3), mask (n,) bool, margin, winner_round (hyp // ROUND).  perturb: a RandomState; every
    virtual pixel the fit reads moves by one ulp of its double up or down (the tests measure the restatement's own spread with it)."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    cur = np.asarray(cur_pts, dtype=np.float32).reshape(-1, 2)
    forw = np.asarray(forw_pts, dtype=np.float32).reshape(-1, 2)
    n = len(cur)
    out = dict(status=OK, hyp=-1, n_inliers=n, F=np.full((3, 3), np.nan), mask=np.ones(n, dtype=bool), margin=np.inf, winner_round=-1)
    if not (np.all(np.isfinite(cur)) and np.all(np.isfinite(forw))):
        return dict(out, status=NOT_FINITE, n_inliers=0, mask=np.zeros(n, dtype=bool))
    if n < MIN_POINTS:
        return out
    a = virtual_pixels(cam, cur, cfg["focal_length"]).astype(np.float64)
    b = virtual_pixels(cam, forw, cfg["focal_length"]).astype(np.float64)
    if perturb is not None:
        a = np.where(perturb.rand(*a.shape) < 0.5, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))
        b = np.where(perturb.rand(*b.shape) < 0.5, np.nextafter(b, np.inf), np.nextafter(b, -np.inf))
    H = int(cfg["ransac_hypotheses"])
    thr = np.float64(cfg["f_threshold"]) * np.float64(cfg["f_threshold"])
    cnt = np.zeros(H, dtype=np.int64)
    errs = {}
    with np.errstate(all="ignore"):
        for h0 in range(0, H, 512):                             # (in blocks: 4096 hypotheses x 4096 points is too much at once)
            hs = range(h0, min(H, h0 + 512))
            sel = np.array([sr.sample8(cfg["seed"], pair, h, n) for h in hs])
            err = sr.epipolar_error(sr.eight_point(a[sel], b[sel]), a, b)
            cnt[h0:h0 + len(sel)] = (err <= thr).sum(axis=1)
            best = int(np.argmax(cnt[h0:h0 + len(sel)]))
            errs[h0 + best] = err[best]
        hyp = int(np.argmax(cnt))                               # most inliers, ties to the lowest h
        err = errs[hyp]
        out.update(hyp=hyp, winner_round=hyp // ROUND, margin=float(np.abs(err / thr - 1.0).min()))
        m0 = err <= thr
        if cnt[hyp] < MIN_POINTS:
            return dict(out, status=FAIL_NO_MODEL)
        Fm = sr.eight_point(a[m0], b[m0])
        if not np.all(np.isfinite(Fm)):
            return dict(out, status=FAIL_NO_MODEL)
        e2 = sr.epipolar_error(Fm, a, b)
        mask = e2 <= thr
        out.update(F=Fm, mask=mask, n_inliers=int(mask.sum()), margin=min(out["margin"], float(np.abs(e2 / thr - 1.0).min())))
    return out


def undistort(cam, pts, ids, prev_ids=None, prev_un_pts=None, dt=None):
    """(un_pts, velocity), (n, 2) float32 each."""
    un = un_points(cam, pts)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    vel = np.zeros((len(un), 2), dtype=np.float32)
    prev_ids = np.zeros(0, dtype=np.int64) if prev_ids is None else np.asarray(prev_ids, dtype=np.int64).reshape(-1)
    if len(prev_ids) == 0:
        return un, vel
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError("dt must be finite and > 0")
    prev = np.asarray(prev_un_pts, dtype=np.float32).reshape(-1, 2)
    first = {}
    for j, i in enumerate(prev_ids.tolist()):
        first.setdefault(i, j)
    for k, i in enumerate(ids.tolist()):
        if i != -1 and i in first:
            with np.errstate(all="ignore"):
                vel[k] = ((un[k].astype(np.float64) - prev[first[i]].astype(np.float64)) / np.float64(dt)).astype(np.float32)
    return un, vel


class Rejecter:
    """The restatement behind RejectHandle's interface (frontend.FeatureTracker's `rejecter`)."""

    def __init__(self, cam, cfg=None):
        self.cam, self.cfg = cam, dict(DEFAULT_CFG, **(cfg or {}))

    def reject(self, cur_pts, forw_pts, pair=0):
        return reject(self.cam, cur_pts, forw_pts, pair, self.cfg)["mask"]

    def undistort(self, pts, ids=None, prev_ids=None, prev_un_pts=None, dt=None):
        if ids is None:
            ids = np.full(len(np.asarray(pts).reshape(-1, 2)), -1, dtype=np.int64)
        return undistort(self.cam, pts, ids, prev_ids, prev_un_pts, dt)


def two_view_scene(cam, seed=0, n=150, outlier_share=0.2, noise_px=0.1, frames=(2, 5)):
    """Matched pixels of the landmarks a stream.SyntheticStream shows in both `frames`, projected through cam, with pixel noise;
    `outlier_share` of the second frame's points replaced by uniform random pixels.  Returns cur (n, 2) float32, forw, planted (n,) bool
    and the clean forw pixels."""
    vio = sys.modules.get("vio_amd")
    if vio is None:
        import conftest
        vio = conftest.load_package()
    from vio_amd import stream as vs
    rng = np.random.RandomState(1000 + seed)
    i, j = frames
    st = vs.SyntheticStream(n_frames=j + 1, landmarks_per_frame=max(30, (n + i) // max(i, 1) + 1), track_len=j + 1, seed=seed, pixel_noise=0.0)
    both = [l for l in range(len(st.lm_obs)) if i in st.lm_obs[l] and j in st.lm_obs[l]]
    both = both[:n]
    assert len(both) == n, (len(both), n)
    a = cam.project(np.array([st.lm_obs[l][i] for l in both]))
    b = cam.project(np.array([st.lm_obs[l][j] for l in both]))
    a = a + rng.normal(0.0, noise_px, a.shape)
    clean = b + rng.normal(0.0, noise_px, b.shape)
    forw = clean.copy()
    planted = np.zeros(n, dtype=bool)
    planted[rng.choice(n, int(round(outlier_share * n)), replace=False)] = True
    forw[planted] = np.stack([rng.uniform(0, cam.width, planted.sum()), rng.uniform(0, cam.height, planted.sum())], axis=1)
    return a.astype(np.float32), forw.astype(np.float32), planted, clean.astype(np.float32)
