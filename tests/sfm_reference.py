"""numpy restatement of the batched structure-from-motion (include/vio_sfm.h, csrc/vio_sfm.hip).

The vision half of the reference's initialisation, in its call order:
  relative_pose()   Estimator::relativePose (VM/src/estimator.cpp:462-491) with MotionEstimator::solveRelativeRT
                    (VM/src/initial/solve_5pts.cpp:193-226): the first frame i with more than 20 correspondences to the newest
                    frame, mean parallax * 460 > 30 and a relative pose with more than 12 points in front of both cameras
  construct()       GlobalSFM::construct (VM/src/initial/initial_sfm.cpp:121-313): the PnP / triangulation chains in its order, then
                    the full bundle adjustment
  sfm()             both
cv::findFundamentalMat, cv::recoverPose, cv::solvePnP and the Ceres solve are replaced by the algorithms include/vio_sfm.h states
(fixed-count RANSAC with counter-based sampling over the normalised 8-point model, Levenberg-Marquardt with Ceres' trust-region
rule), written here the way the kernels evaluate them: every symmetric eigenproblem is a cyclic Jacobi iteration with a fixed sweep
count, the points are eliminated by a Schur complement, the reduced system is factorised by Cholesky.

This restatement is unpinned: neither OpenCV nor Ceres can be compiled here.  The CPU tests hold it to the ground truth of the
synthetic streams (tests/test_sfm_reference.py), and the GPU tests hold the device to it.

An item is a dict: n_frames F, start_frame (n_tracks,) int32, obs_offset (n_tracks + 1,) int64, pts (n_obs, 2): track j is seen in the
consecutive frames start_frame[j] .. with the normalised points pts[obs_offset[j] : obs_offset[j + 1]].
"""
import numpy as np

OK, NOT_FINITE = 0, -3
FAIL_RELATIVE_POSE, FAIL_PNP, FAIL_BA = 1, 2, 3
MAX_FRAMES = 16
FOCAL = 460.0
RANSAC_THRESHOLD = 0.3 / 460.0
MIN_CORRES = 20             # more than
MIN_PARALLAX_PX = 30.0      # more than
MIN_FRONT = 12              # more than
MAX_DEPTH = 50.0
JACOBI_SWEEPS = 10
PNP_MIN_POINTS = 10
PNP_MAX_ITER = 20
PNP_STEP_TOL = 1.1920929e-07
BA_MAX_ITER = 50
BA_FUNCTION_TOL = 1e-6
BA_GRADIENT_TOL = 1e-10
BA_PARAMETER_TOL = 1e-8
BA_COST_OK = 5e-3
LM_RADIUS0 = 1e4
LM_RADIUS_MAX = 1e16
LM_RADIUS_MIN = 1e-32
LM_MIN_RHO = 1e-3
LM_DIAG_MIN = 1e-6
LM_DIAG_MAX = 1e32
DEFAULT_CFG = dict(seed=0, ransac_hypotheses=128)

M32 = 0xFFFFFFFF


# ---- counter-based sampling ----------------------------------------------------------------------------
def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def hash4(seed, i, h, draw):
    a = mix32(seed + 0x9E3779B9)
    a = mix32(a + i)
    a = mix32(a + h)
    return mix32(a + draw)


def sample8(seed, i, h, n):
    """The 8 distinct indices below n of hypothesis h of candidate i: draw k picks the (hash % (n - k))-th index not taken yet."""
    taken = []                                  # ascending
    out = []
    for k in range(8):
        idx = hash4(seed, i, h, k) % (n - k)
        pos = 0
        for c in taken:
            if idx >= c:
                idx += 1
                pos += 1
            else:
                break
        taken.insert(pos, idx)
        out.append(idx)
    return out


# ---- small dense kernels -------------------------------------------------------------------------------
def jacobi_eigh(A):
    """Cyclic Jacobi on symmetric matrices A (..., n, n): JACOBI_SWEEPS sweeps over (p, q), p < q, row by row.  Returns (w, V) with
    A = V diag(w) V^T, unsorted."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[-1]
    V = np.zeros_like(A)
    V[..., np.arange(n), np.arange(n)] = 1.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for _ in range(JACOBI_SWEEPS):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[..., p, q]
                    theta = (A[..., q, q] - A[..., p, p]) / (2.0 * apq)
                    t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    t = np.where(apq == 0.0, 0.0, t)
                    t = np.where(np.isfinite(t), t, 0.0)
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    c_, s_ = c[..., None], s[..., None]
                    rp, rq = A[..., p, :].copy(), A[..., q, :].copy()
                    A[..., p, :] = c_ * rp - s_ * rq
                    A[..., q, :] = s_ * rp + c_ * rq
                    cp, cq = A[..., :, p].copy(), A[..., :, q].copy()
                    A[..., :, p] = c_ * cp - s_ * cq
                    A[..., :, q] = s_ * cp + c_ * cq
                    vp, vq = V[..., :, p].copy(), V[..., :, q].copy()
                    V[..., :, p] = c_ * vp - s_ * vq
                    V[..., :, q] = s_ * vp + c_ * vq
    return A[..., np.arange(n), np.arange(n)], V


def smallest_eigvec(A):
    w, V = jacobi_eigh(A)
    k = np.argmin(w, axis=-1)
    return np.take_along_axis(V, k[..., None, None], axis=-1)[..., 0]


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = np.sqrt(th2)
    K = skew(w)
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    return np.eye(3) + a * K + b * (K @ K)


def rot_to_quat(R):
    """(w, x, y, z) of a rotation matrix: Eigen's Quaternion(Matrix3d) branches."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def triangulate_point(P0, P1, p0, p1):
    """GlobalSFM::triangulatePoint (initial_sfm.cpp:5-20): the smallest right singular vector of the 4 x 4 design matrix (here the
    smallest eigenvector of its normal matrix), dehomogenised; no cheirality test.  Batched over leading axes of p0 / p1."""
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    D = np.stack([p0[..., 0, None] * P0[2] - P0[0], p0[..., 1, None] * P0[2] - P0[1],
                  p1[..., 0, None] * P1[2] - P1[0], p1[..., 1, None] * P1[2] - P1[1]], axis=-2)
    v = smallest_eigvec(np.swapaxes(D, -1, -2) @ D)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v[..., 0:3] / v[..., 3:4]


# ---- stage 1 -------------------------------------------------------------------------------------------
def correspondences(item, i):
    """FeatureManager::getCorresponding(i, F - 1) (feature_manager.cpp:120-139), in track order: (n, 4) = (x_i, y_i, x_last, y_last)
    and the tracks' indices."""
    F = item["n_frames"]
    sf, off = np.asarray(item["start_frame"]), np.asarray(item["obs_offset"])
    n = off[1:] - off[:-1]
    m = (sf <= i) & (sf + n - 1 >= F - 1)
    idx = np.nonzero(m)[0]
    pts = np.asarray(item["pts"], dtype=np.float64).reshape(-1, 2)
    a = pts[off[idx] + (i - sf[idx])]
    b = pts[off[idx] + (F - 1 - sf[idx])]
    return np.concatenate([a, b], axis=1).reshape(-1, 4), idx


def hartley(p):
    """Hartley's scaling of points p (..., n, 2): (centroid (..., 2), scale (...,)) with mean distance sqrt(2) after it."""
    c = p.sum(axis=-2) / p.shape[-2]
    d = p - c[..., None, :]
    md = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).sum(axis=-1) / p.shape[-2]
    return c, np.sqrt(2.0) / md


def eight_point(a, b):
    """The normalised 8-point model of x_b^T F x_a = 0 over n >= 8 correspondences a, b (..., n, 2): F (..., 3, 3), rank 2."""
    ca, sa = hartley(a)
    cb, sb = hartley(b)
    x1 = (a - ca[..., None, :]) * sa[..., None, None]
    x2 = (b - cb[..., None, :]) * sb[..., None, None]
    one = np.ones(x1.shape[:-1])
    rows = np.stack([x2[..., 0] * x1[..., 0], x2[..., 0] * x1[..., 1], x2[..., 0],
                     x2[..., 1] * x1[..., 0], x2[..., 1] * x1[..., 1], x2[..., 1],
                     x1[..., 0], x1[..., 1], one], axis=-1)                        # (..., n, 9)
    N = np.zeros(rows.shape[:-2] + (9, 9))
    for k in range(rows.shape[-2]):                                                # in correspondence order
        r = rows[..., k, :]
        N = N + r[..., :, None] * r[..., None, :]
    f = smallest_eigvec(N)
    Fh = f.reshape(f.shape[:-1] + (3, 3))
    v = smallest_eigvec(np.swapaxes(Fh, -1, -2) @ Fh)                             # rank 2: F - (F v) v^T, v the smallest right
    Fv = (Fh @ v[..., None])[..., 0]                                               # singular vector
    Fh = Fh - Fv[..., :, None] * v[..., None, :]
    z = np.zeros_like(sa)
    T1 = np.stack([np.stack([sa, z, -sa * ca[..., 0]], -1), np.stack([z, sa, -sa * ca[..., 1]], -1), np.stack([z, z, z + 1], -1)], -2)
    T2 = np.stack([np.stack([sb, z, -sb * cb[..., 0]], -1), np.stack([z, sb, -sb * cb[..., 1]], -1), np.stack([z, z, z + 1], -1)], -2)
    return np.swapaxes(T2, -1, -2) @ Fh @ T1


def epipolar_error(Fm, a, b):
    """OpenCV's fundamental-matrix error: the larger of the two squared point-to-epipolar-line distances.  Fm (..., 3, 3), a / b (n, 2):
    (..., n)."""
    ax, ay, bx, by = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    F_ = Fm[..., None, :, :]
    A = F_[..., 0, 0] * ax + F_[..., 0, 1] * ay + F_[..., 0, 2]
    B = F_[..., 1, 0] * ax + F_[..., 1, 1] * ay + F_[..., 1, 2]
    Cc = F_[..., 2, 0] * ax + F_[..., 2, 1] * ay + F_[..., 2, 2]
    d2 = bx * A + by * B + Cc
    s2 = 1.0 / (A * A + B * B)
    A1 = F_[..., 0, 0] * bx + F_[..., 1, 0] * by + F_[..., 2, 0]
    B1 = F_[..., 0, 1] * bx + F_[..., 1, 1] * by + F_[..., 2, 1]
    C1 = F_[..., 0, 2] * bx + F_[..., 1, 2] * by + F_[..., 2, 2]
    d1 = ax * A1 + ay * B1 + C1
    s1 = 1.0 / (A1 * A1 + B1 * B1)
    return np.maximum(d1 * d1 * s1, d2 * d2 * s2)


def recover_pose(E, a, b, mask):
    """cv::recoverPose with K = I on the inliers: (count, R, t, mask of the points in front)."""
    w, V = jacobi_eigh(E.T @ E)
    order = sorted(range(3), key=lambda k: -w[k])
    V = V[:, order]
    w = w[order]
    u0 = E @ V[:, 0] / np.sqrt(w[0])
    u1 = E @ V[:, 1] / np.sqrt(w[1])
    u1 = u1 - (u0 @ u1) * u0
    u1 = u1 / np.sqrt(u1 @ u1)
    u2 = np.cross(u0, u1)
    U = np.stack([u0, u1, u2], axis=1)
    if np.linalg.det(V) < 0:
        V = V * np.array([1.0, 1.0, -1.0])
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2 = U @ W @ V.T, U @ W.T @ V.T
    idx = np.nonzero(mask)[0]
    best = (-1, None, None, None)
    P0 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    for R, t in ((R1, u2), (R2, u2), (R1, -u2), (R2, -u2)):
        P1 = np.concatenate([R, t[:, None]], axis=1)
        X = triangulate_point(P0, P1, a[idx], b[idx])
        z1 = X[:, 2]
        z2 = (X @ R.T + t)[:, 2]
        good = (z1 > 0) & (z1 < MAX_DEPTH) & (z2 > 0) & (z2 < MAX_DEPTH)
        cnt = int(good.sum())
        if cnt > best[0]:
            m = np.zeros(len(mask), dtype=bool)
            m[idx[good]] = True
            best = (cnt, R, t, m)
    return best


def solve_relative_rt(corres, i, cfg):
    """solveRelativeRT on the correspondences of candidate i.  Returns a dict: ok, R (relative_R), T (relative_T), hyp, n_inliers,
    mask (RANSAC's final mask), front (recoverPose's count), margin (smallest relative distance of a final error to the gate)."""
    a, b = corres[:, 0:2], corres[:, 2:4]
    n = len(a)
    H = int(cfg["ransac_hypotheses"])
    sel = np.array([sample8(cfg["seed"], i, h, n) for h in range(H)])
    Fs = eight_point(a[sel], b[sel])
    thr = RANSAC_THRESHOLD * RANSAC_THRESHOLD
    err = epipolar_error(Fs, a, b)
    with np.errstate(invalid="ignore"):
        cnt = (err <= thr).sum(axis=1)
    hyp = int(np.argmax(cnt))                              # most inliers, ties to the lowest h
    out = dict(ok=False, hyp=hyp, n_inliers=int(cnt[hyp]), mask=np.zeros(n, dtype=bool), front=0, R=np.full((3, 3), np.nan),
               T=np.full(3, np.nan), margin=np.inf, margin_all=float(np.abs(err / thr - 1.0).min()))
    m0 = err[hyp] <= thr
    out["margin"] = float(np.abs(err[hyp] / thr - 1.0).min())
    if cnt[hyp] < 8:
        return out
    Fm = eight_point(a[m0], b[m0])                         # one refit on the winner's inliers, then the final mask
    e2 = epipolar_error(Fm, a, b)
    out["margin"] = min(out["margin"], float(np.abs(e2 / thr - 1.0).min()))
    mask = e2 <= thr
    out["mask"] = mask
    out["n_inliers"] = int(mask.sum())
    if not np.all(np.isfinite(Fm)) or mask.sum() == 0:
        return out
    front, R, t, _ = recover_pose(Fm, a, b, mask)
    out["front"] = front
    if R is None or not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return out
    out["R"] = R.T.copy()                                  # solve_5pts.cpp:218-219
    out["T"] = -(R.T @ t)
    out["ok"] = front > MIN_FRONT
    return out


def finite_item(item):
    return bool(np.all(np.isfinite(np.asarray(item["pts"], dtype=np.float64))))


def relative_pose(item, cfg=None):
    """Estimator::relativePose.  Returns a dict: status, l, R, T, hyp, n_inliers, mask (over candidate l's correspondences),
    corres (F - 1 counts), parallax (F - 1 mean parallaxes in pixels), margin."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    F = item["n_frames"]
    out = dict(status=FAIL_RELATIVE_POSE, l=-1, R=np.full((3, 3), np.nan), T=np.full(3, np.nan), hyp=-1, n_inliers=0,
               mask=np.zeros(0, dtype=bool), corres=np.zeros(F - 1, dtype=np.int32), parallax=np.zeros(F - 1), margin=np.inf,
               front=0)
    if not finite_item(item):
        out["status"] = NOT_FINITE
        return out
    cs = []
    for i in range(F - 1):
        c, _ = correspondences(item, i)
        cs.append(c)
        out["corres"][i] = len(c)
        if len(c):
            d = c[:, 0:2] - c[:, 2:4]
            s = 0.0
            for v in np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]):       # in track order
                s = s + v
            out["parallax"][i] = s / len(c) * FOCAL
    for i in range(F - 1):
        if out["corres"][i] > MIN_CORRES and out["parallax"][i] > MIN_PARALLAX_PX:
            r = solve_relative_rt(cs[i], i, cfg)
            if r["ok"]:
                out.update(status=OK, l=i, R=r["R"], T=r["T"], hyp=r["hyp"], n_inliers=r["n_inliers"], mask=r["mask"],
                           margin=r["margin"], front=r["front"])
                return out
    return out


# ---- stage 2 -------------------------------------------------------------------------------------------
def _obs_arrays(item):
    sf = np.asarray(item["start_frame"], dtype=np.int64)
    off = np.asarray(item["obs_offset"], dtype=np.int64)
    pts = np.asarray(item["pts"], dtype=np.float64).reshape(-1, 2)
    track = np.repeat(np.arange(len(sf)), off[1:] - off[:-1])
    frame = np.arange(len(pts)) - off[track] + sf[track]
    return sf, off, pts, track, frame


def _residuals(Rc, tc, X, pts, track, frame):
    """Normalised reprojection residuals of every observation, (n_obs, 2), the camera points and R X."""
    RX = np.einsum("oij,oj->oi", Rc[frame], X[track])
    Xc = RX + tc[frame]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = Xc[:, 0:2] / Xc[:, 2:3] - pts
    return r, Xc, RX


def _jacobians(Rc, Xc, RX, frame):
    """Per observation: Jc (2 x 6) over (left rotation increment, translation) and Jp (2 x 3) over the point."""
    n = len(Xc)
    iz = 1.0 / Xc[:, 2]
    Jp_ = np.zeros((n, 2, 3))
    Jp_[:, 0, 0] = iz
    Jp_[:, 1, 1] = iz
    Jp_[:, 0, 2] = -Xc[:, 0] * iz * iz
    Jp_[:, 1, 2] = -Xc[:, 1] * iz * iz
    S = np.zeros((n, 3, 3))                     # -[R X]x
    S[:, 0, 1], S[:, 0, 2] = RX[:, 2], -RX[:, 1]
    S[:, 1, 0], S[:, 1, 2] = -RX[:, 2], RX[:, 0]
    S[:, 2, 0], S[:, 2, 1] = RX[:, 1], -RX[:, 0]
    Jc = np.concatenate([Jp_ @ S, Jp_], axis=2)
    Jp = Jp_ @ Rc[frame]
    return Jc, Jp


def _seq_sum(v):
    s = 0.0
    for x in v:
        s = s + x
    return s


def _lm_radius(radius, rho):
    return min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), LM_RADIUS_MAX)


def solve_frame_by_pnp(R0, t0, X, obs):
    """GlobalSFM::solveFrameByPnP's solve: Levenberg-Marquardt on (left rotation increment, t) from the guess.  Returns (ok, R, t,
    iterations)."""
    n = len(X)
    R, t = R0.copy(), t0.copy()
    fr = np.zeros(n, dtype=np.int64)
    trk = np.arange(n)

    def lin(R, t):
        r, Xc, RX = _residuals(R[None], t[None], X, obs, trk, fr)
        Jc, _ = _jacobians(R[None], Xc, RX, fr)
        cost = 0.5 * _seq_sum(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
        H = np.zeros((6, 6))
        g = np.zeros(6)
        for k in range(n):
            H = H + Jc[k].T @ Jc[k]
            g = g + Jc[k].T @ r[k]
        return cost, H, g

    cost, H, g = lin(R, t)
    radius, v, it = LM_RADIUS0, 2.0, 0
    if not np.isfinite(cost):
        return False, R, t, it
    if np.abs(g).max() <= BA_GRADIENT_TOL:
        return True, R, t, it
    while it < PNP_MAX_ITER:
        it += 1
        lam = 1.0 / radius
        D = np.clip(np.diag(H), LM_DIAG_MIN, LM_DIAG_MAX)
        A = H + lam * np.diag(D)
        L = _cholesky(A)
        ok = L is not None
        if ok:
            d = _chol_solve(L, -g)
            if np.sqrt(d @ d) <= PNP_STEP_TOL:
                break
            R2, t2 = exp_so3(d[0:3]) @ R, t + d[3:6]
            r2, _, _ = _residuals(R2[None], t2[None], X, obs, trk, fr)
            c2 = 0.5 * _seq_sum(r2[:, 0] * r2[:, 0] + r2[:, 1] * r2[:, 1])
            model = 0.5 * (lam * (d * D) @ d - d @ g)
            rho = (cost - c2) / model if np.isfinite(c2) and model > 0 else -1.0
        if ok and rho > LM_MIN_RHO:
            R, t = R2, t2
            cost, H, g = lin(R, t)
            if np.abs(g).max() <= BA_GRADIENT_TOL:
                break
            radius, v = _lm_radius(radius, rho), 2.0
        else:
            radius, v = radius / v, v * 2.0
            if radius < LM_RADIUS_MIN:
                break
    return bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t))), R, t, it


def _cholesky(A):
    """Lower Cholesky factor, column by column; None when a pivot is not positive."""
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _chol_solve(L, b):
    n = len(b)
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def bundle_adjust(F, l, Rc, tc, X, state, item):
    """The full BA of initial_sfm.cpp:233-281 with the points eliminated.  Rc / tc: camera-from-world rotations and translations (F),
    X (n_tracks, 3), state (n_tracks,) bool.  Returns (converged, iterations, initial cost, final cost, Rc, tc, X)."""
    sf, off, pts, track, frame = _obs_arrays(item)
    use = state[track]
    pts, track, frame = pts[use], track[use], frame[use]
    nt = len(sf)
    n_obs = len(pts)
    const = np.zeros(6 * F, dtype=bool)
    const[6 * l:6 * l + 6] = True
    const[6 * (F - 1) + 3:6 * (F - 1) + 6] = True
    tid = np.nonzero(state)[0]

    def cost_of(Rc, tc, X):
        r, Xc, RX = _residuals(Rc, tc, X, pts, track, frame)
        per = np.zeros(nt)
        np.add.at(per, track, r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
        return 0.5 * _seq_sum(per[tid]), r, Xc, RX

    def lin(Rc, tc, X):
        cost, r, Xc, RX = cost_of(Rc, tc, X)
        Jc, Jp = _jacobians(Rc, Xc, RX, frame)
        Hcc = np.zeros((F, 6, 6))
        gc = np.zeros((F, 6))
        Hpp = np.zeros((nt, 3, 3))
        gp = np.zeros((nt, 3))
        for o in range(n_obs):                              # in observation order: by track, then by frame
            Hcc[frame[o]] += Jc[o].T @ Jc[o]
            gc[frame[o]] += Jc[o].T @ r[o]
            Hpp[track[o]] += Jp[o].T @ Jp[o]
            gp[track[o]] += Jp[o].T @ r[o]
        W = np.einsum("oki,okj->oij", Jc, Jp)               # (n_obs, 6, 3)
        return dict(cost=cost, Hcc=Hcc, gc=gc, Hpp=Hpp, gp=gp, W=W)

    def gmax(s):
        g = np.abs(s["gc"].reshape(-1)[~const])
        gp = np.abs(s["gp"][tid])
        return max(g.max() if g.size else 0.0, gp.max() if gp.size else 0.0)

    Rc, tc, X = Rc.copy(), tc.copy(), X.copy()
    s = lin(Rc, tc, X)
    cost0 = s["cost"]
    radius, v, it = LM_RADIUS0, 2.0, 0
    converged = False
    if not np.isfinite(cost0):
        return False, 0, cost0, cost0, Rc, tc, X
    if gmax(s) <= BA_GRADIENT_TOL:
        return True, 0, cost0, cost0, Rc, tc, X
    while it < BA_MAX_ITER:
        it += 1
        lam = 1.0 / radius
        Dc = np.clip(np.stack([np.diag(h) for h in s["Hcc"]]).reshape(-1), LM_DIAG_MIN, LM_DIAG_MAX)
        Dp = np.clip(np.stack([np.diag(h) for h in s["Hpp"]]), LM_DIAG_MIN, LM_DIAG_MAX)
        Hpp = s["Hpp"] + lam * np.stack([np.diag(d) for d in Dp])
        Hinv = np.zeros_like(Hpp)
        Hinv[tid] = _inv3_sym(Hpp[tid])
        Y = s["W"] @ Hinv[track]                            # (n_obs, 6, 3)
        S = np.zeros((6 * F, 6 * F))
        rhs = np.zeros(6 * F)
        for f in range(F):
            S[6 * f:6 * f + 6, 6 * f:6 * f + 6] = s["Hcc"][f]
            rhs[6 * f:6 * f + 6] = -s["gc"][f]
        S[np.arange(6 * F), np.arange(6 * F)] += lam * Dc
        for j in tid:                                        # in track order
            oo = np.nonzero(track == j)[0]
            for o1 in oo:
                f1 = frame[o1]
                rhs[6 * f1:6 * f1 + 6] += Y[o1] @ s["gp"][j]
                for o2 in oo:
                    f2 = frame[o2]
                    S[6 * f1:6 * f1 + 6, 6 * f2:6 * f2 + 6] -= Y[o1] @ s["W"][o2].T
        S[const, :] = 0.0
        S[:, const] = 0.0
        S[const, const] = 1.0
        rhs[const] = 0.0
        L = _cholesky(S)
        ok = L is not None
        if ok:
            dc = _chol_solve(L, rhs)
            wd = np.einsum("oij,oi->oj", s["W"], dc.reshape(F, 6)[frame])      # W^T dc per observation
            acc = np.zeros((nt, 3))
            for o in range(n_obs):
                acc[track[o]] += wd[o]
            dp = np.einsum("jab,jb->ja", Hinv, -s["gp"] - acc)
            dp[~state] = 0.0
            x2 = _seq_sum([(q * q).sum() for q in [rot_to_quat(R) for R in Rc]]) + _seq_sum((tc * tc).sum(axis=1)) + \
                _seq_sum((X[tid] * X[tid]).sum(axis=1))
            d2 = dc @ dc + _seq_sum((dp[tid] * dp[tid]).sum(axis=1))
            if np.sqrt(d2) <= BA_PARAMETER_TOL * (np.sqrt(x2) + BA_PARAMETER_TOL):
                converged = True
                break
            R2 = np.stack([exp_so3(dc[6 * f:6 * f + 3]) @ Rc[f] for f in range(F)])
            t2 = tc + dc.reshape(F, 6)[:, 3:6]
            X2 = X + dp
            c2 = cost_of(R2, t2, X2)[0]
            gdot = dc @ s["gc"].reshape(-1) + _seq_sum((dp[tid] * s["gp"][tid]).sum(axis=1))
            ddd = (dc * Dc) @ dc + _seq_sum((dp[tid] * Dp[tid] * dp[tid]).sum(axis=1))
            model = 0.5 * (lam * ddd - gdot)
            rho = (s["cost"] - c2) / model if np.isfinite(c2) and model > 0 else -1.0
        if ok and rho > LM_MIN_RHO:
            old = s["cost"]
            Rc, tc, X = R2, t2, X2
            s = lin(Rc, tc, X)
            if gmax(s) <= BA_GRADIENT_TOL:
                converged = True
                break
            if abs(old - s["cost"]) <= BA_FUNCTION_TOL * old:
                converged = True
                break
            radius, v = _lm_radius(radius, rho), 2.0
        else:
            radius, v = radius / v, v * 2.0
            if radius < LM_RADIUS_MIN:
                break
    return converged, it, cost0, s["cost"], Rc, tc, X


def _inv3_sym(A):
    """Inverse of symmetric 3 x 3 matrices (n, 3, 3) by cofactors."""
    a, b, c, d, e, f = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        idet = 1.0 / (a * c00 + b * c01 + c * c02)
    out = np.stack([np.stack([c00, c01, c02], -1), np.stack([c01, c11, c12], -1), np.stack([c02, c12, c22], -1)], -2)
    return out * idet[:, None, None]


def construct(item, l, relative_R, relative_T):
    """GlobalSFM::construct.  Returns a dict: status, fail_frame, Q (F, 4) wxyz, T (F, 3) (camera poses in frame l), points
    (n_tracks, 3), state (n_tracks,), pnp_iterations (F,), ba_iterations, ba_converged, initial_cost, final_cost, n_remaining
    (the tracks left for the last step, initial_sfm.cpp:196-210)."""
    F = item["n_frames"]
    sf, off, pts, track, frame = _obs_arrays(item)
    nt = len(sf)
    nobs = off[1:] - off[:-1]
    out = dict(status=OK, fail_frame=-1, Q=np.full((F, 4), np.nan), T=np.full((F, 3), np.nan), points=np.full((nt, 3), np.nan),
               state=np.zeros(nt, dtype=bool), pnp_iterations=np.zeros(F, dtype=np.int32), ba_iterations=0, ba_converged=False,
               initial_cost=np.nan, final_cost=np.nan, n_remaining=0)
    if not (finite_item(item) and np.all(np.isfinite(relative_R)) and np.all(np.isfinite(relative_T))):
        out["status"] = NOT_FINITE
        return out
    Rc = np.zeros((F, 3, 3))
    tc = np.zeros((F, 3))
    X = np.zeros((nt, 3))
    state = np.zeros(nt, dtype=bool)
    Rc[l] = np.eye(3)
    Rc[F - 1] = quat_to_rot(rot_to_quat(relative_R)).T                    # q[F-1] = Quaterniond(relative_R); c_Quat = inverse
    tc[F - 1] = -(Rc[F - 1] @ relative_T)

    def pose(i):
        return np.concatenate([Rc[i], tc[i][:, None]], axis=1)

    def has(i):
        return (sf <= i) & (sf + nobs - 1 >= i)

    def tri2(f0, f1):
        m = ~state & has(f0) & has(f1)
        idx = np.nonzero(m)[0]
        if len(idx):
            X[idx] = triangulate_point(pose(f0), pose(f1), pts[off[idx] + f0 - sf[idx]], pts[off[idx] + f1 - sf[idx]])
            state[idx] = True

    def pnp(i, guess):
        idx = np.nonzero(state & has(i))[0]
        if len(idx) < PNP_MIN_POINTS:
            return False
        ok, R, t, it = solve_frame_by_pnp(Rc[guess], tc[guess], X[idx], pts[off[idx] + i - sf[idx]])
        out["pnp_iterations"][i] = it
        if ok:
            Rc[i], tc[i] = R, t
        return ok

    def failed(i):
        out.update(status=FAIL_PNP, fail_frame=i)
        return out

    for i in range(l, F - 1):
        if i > l and not pnp(i, i - 1):
            return failed(i)
        tri2(i, F - 1)
    for i in range(l + 1, F - 1):
        tri2(l, i)
    for i in range(l - 1, -1, -1):
        if not pnp(i, i + 1):
            return failed(i)
        tri2(i, l)
    idx = np.nonzero(~state & (nobs >= 2))[0]
    out["n_remaining"] = len(idx)                    # tracks no chain step saw: triangulated from their first and last observation
    for j in idx:
        X[j] = triangulate_point(pose(sf[j]), pose(sf[j] + nobs[j] - 1), pts[off[j]], pts[off[j + 1] - 1])
        state[j] = True
    # c_Quat = c_Rotation: the BA starts from the quaternions' rotations
    Rc = np.stack([quat_to_rot(_normalized(rot_to_quat(R))) for R in Rc])
    conv, it, c0, c1, Rc, tc, X = bundle_adjust(F, l, Rc, tc, X, state, item)
    out.update(ba_iterations=it, ba_converged=bool(conv), initial_cost=c0, final_cost=c1, state=state.copy())
    if not (np.isfinite(c1) and np.all(np.isfinite(Rc)) and np.all(np.isfinite(tc))):
        out["status"] = NOT_FINITE
        return out
    if not (conv or c1 < BA_COST_OK):
        out["status"] = FAIL_BA
        return out
    for i in range(F):
        out["Q"][i] = rot_to_quat(Rc[i].T)
        out["T"][i] = -(Rc[i].T @ tc[i])
    out["points"] = np.where(state[:, None], X, np.nan)
    return out


def _normalized(q):
    return q / np.sqrt(q @ q)


def sfm(item, cfg=None):
    """relativePose + construct: construct's dict with stage 1's entries under `rel`."""
    rel = relative_pose(item, cfg)
    if rel["status"] != OK:
        F = item["n_frames"]
        nt = len(item["start_frame"])
        return dict(status=rel["status"], fail_frame=-1, Q=np.full((F, 4), np.nan), T=np.full((F, 3), np.nan),
                    points=np.full((nt, 3), np.nan), state=np.zeros(nt, dtype=bool), pnp_iterations=np.zeros(F, dtype=np.int32),
                    ba_iterations=0, ba_converged=False, initial_cost=np.nan, final_cost=np.nan, n_remaining=0, rel=rel)
    out = construct(item, rel["l"], rel["R"], rel["T"])
    out["rel"] = rel
    return out


# ---- items and ground truth ----------------------------------------------------------------------------
def item_from_tracks(tracks, frames):
    """The SfM item of a StreamDriver's tracks (landmark -> [(global frame, point)], consecutive window frames) over the window
    `frames`, in the dict's order (sfm_f, estimator.cpp:275-289).  Returns (item, landmark ids)."""
    sf, off, pts, ids = [], [0], [], []
    for lm, tr in tracks.items():
        sf.append(frames.index(tr[0][0]))
        pts.extend(p for _, p in tr)
        off.append(off[-1] + len(tr))
        ids.append(lm)
    return dict(n_frames=len(frames), start_frame=np.array(sf, dtype=np.int32), obs_offset=np.array(off, dtype=np.int64),
                pts=np.array(pts, dtype=np.float64).reshape(-1, 2)), ids


def window_item(stream, frames):
    """The item of the window `frames` (consecutive global frames) of a stream, as StreamDriver's bookkeeping would hold it: a landmark
    hosted in frame h is seen in h (lm_px) and in lm_obs's frames; only the part inside the window counts.  Returns (item, ids)."""
    tracks = {}
    for f in frames:
        for lm, h in enumerate(stream.lm_host):
            if h == f:
                tracks[lm] = [(f, np.asarray(stream.lm_px[lm], dtype=np.float64))]
            elif lm in tracks and f in stream.lm_obs[lm] and tracks[lm][-1][0] == f - 1:
                tracks[lm].append((f, np.asarray(stream.lm_obs[lm][f], dtype=np.float64)))
    return item_from_tracks(tracks, list(frames))


def ground_truth(stream, frames, l, ids):
    """Camera poses (R (F, 3, 3) camera-to-l, T (F, 3)) and the landmarks `ids` in camera frame frames[l], scaled to |T[F-1]| = 1."""
    ric = np.asarray(getattr(stream, "ric", None) if hasattr(stream, "ric") else _synth().R_IC, dtype=np.float64)
    tic = np.asarray(getattr(stream, "tic", None) if hasattr(stream, "tic") else _synth().T_IC, dtype=np.float64)
    fl = frames[l]
    Rcl = stream.R[fl] @ ric
    pcl = stream.P[fl] + stream.R[fl] @ tic
    R = np.stack([Rcl.T @ stream.R[f] @ ric for f in frames])
    T = np.stack([Rcl.T @ (stream.P[f] + stream.R[f] @ tic - pcl) for f in frames])
    X = []
    for lm in ids:
        h = stream.lm_host[lm]
        px = stream.lm_px[lm]
        pw = stream.R[h] @ (ric @ (np.array([px[0], px[1], 1.0]) * stream.lm_depth[lm]) + tic) + stream.P[h]
        X.append(Rcl.T @ (pw - pcl))
    s = np.linalg.norm(T[-1])
    return R, T / s, np.array(X).reshape(-1, 3) / s, s


def _synth():
    import sys
    return sys.modules["vio_amd"].synth


def perturb_ulp(item, rng):
    """The item with every point moved by one ulp in a random direction (the bar of the device comparisons, as init_reference's)."""
    a = np.asarray(item["pts"], dtype=np.float64)
    return dict(item, pts=np.where(rng.rand(*a.shape) < 0.5, np.nextafter(a, np.inf), np.nextafter(a, -np.inf)))
