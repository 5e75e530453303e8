"""numpy restatement of the batched extrinsic rotation calibration (include/vio_exrot.h, csrc/vio_exrot.hip).

InitialEXRotation::CalibrationExRotation (VM/src/initial/initial_ex_rotation.cpp:11-141) over a window of F frames: the history after
F - 1 calls, every call's outcome ("step" k = 1 .. F - 1, the reference's frame_count) reported:
  relative_rotations()   solveRelativeR of every consecutive frame pair
  calibrate()            the recursion over the pairs: Rc_g with the ric of the step before, the Huber weights, the 4 x 4 problem, the gate
  exrot()                both
cv::findFundamentalMat with its defaults is replaced by what include/vio_exrot.h states: the threshold of 3.0 on normalised image
coordinates makes every correspondence an inlier, so the result is the normalised 8-point fit over all correspondences in track order
(sfm_reference.eight_point); decomposeE's SVD is built as sfm_reference.recover_pose builds it, without the sign fix of V; the four
triangulation tests use sfm_reference.triangulate_point.  This restatement is unpinned: OpenCV is not a dependency, and nothing here is
compared against it.  The CPU tests hold it to the ground truth of directly built windows (tests/test_exrot_reference.py), and the GPU
tests hold the device to it.

An item is sfm_reference's dict plus delta_q (F - 1, 4) as (w, x, y, z): the pre-integrated rotation from frame k to frame k + 1.
"""
import numpy as np

import sfm_reference as sr
from sfm_reference import eight_point, jacobi_eigh, quat_to_rot, rot_to_quat, triangulate_point

OK, NOT_FINITE = 0, -3
FAIL_NOT_OBSERVABLE = 1
MAX_FRAMES = 32
MIN_CORRES = 9
DEFAULT_CFG = dict(min_frames=10, min_sigma=0.25, huber_deg=5.0)


# ---- step 1: solveRelativeR ----------------------------------------------------------------------------
def pair_correspondences(item, k):
    """FeatureManager::getCorresponding(k, k + 1), in track order: (n, 4) = (x_k, y_k, x_k+1, y_k+1)."""
    sf, off = np.asarray(item["start_frame"]), np.asarray(item["obs_offset"])
    n = off[1:] - off[:-1]
    idx = np.nonzero((sf <= k) & (sf + n - 1 >= k + 1))[0]
    pts = np.asarray(item["pts"], dtype=np.float64).reshape(-1, 2)
    a = pts[off[idx] + (k - sf[idx])]
    b = pts[off[idx] + (k + 1 - sf[idx])]
    return np.concatenate([a, b], axis=1).reshape(-1, 4)


def decompose_e(E):
    """decomposeE and the det R1 = -1 case: (R1, R2, t1, det_flip); t2 = -t1.  V and the singular values from the eigenvectors of
    E^T E in descending order (no sign fix), u0 = E v0 / s0, u1 = E v1 / s1 made orthonormal to u0, u2 = u0 x u1.  With
    det R1 + 1 < 1e-9 the reference decomposes -E, whose SVD is (-U, S, V): R1, R2 and t1 change sign."""
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
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2 = U @ W @ V.T, U @ W.T @ V.T
    flip = bool(np.linalg.det(R1) + 1.0 < 1e-9)
    if flip:
        R1, R2, u2 = -R1, -R2, -u2
    return R1, R2, u2, flip


def solve_relative_r(corres):
    """solveRelativeR.  Returns a dict: Rc (3, 3), n_corres, front (4,) counts for (R1, t1), (R1, t2), (R2, t1), (R2, t2), choice
    (1: R1, 2: R2, 0: the identity), det_flip, finite."""
    n = len(corres)
    out = dict(Rc=np.eye(3), n_corres=n, front=np.zeros(4, dtype=np.int32), choice=0, det_flip=False, finite=True)
    if n < MIN_CORRES:
        return out
    a, b = corres[:, 0:2], corres[:, 2:4]
    with np.errstate(all="ignore"):
        E = eight_point(a, b)
        R1, R2, t1, flip = decompose_e(E)
    if not (np.all(np.isfinite(R1)) and np.all(np.isfinite(R2)) and np.all(np.isfinite(t1))):
        return dict(out, Rc=np.full((3, 3), np.nan), finite=False)
    P0 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    front = []
    for R, t in ((R1, t1), (R1, -t1), (R2, t1), (R2, -t1)):
        X = triangulate_point(P0, np.concatenate([R, t[:, None]], axis=1), a, b)
        with np.errstate(invalid="ignore"):
            front.append(int(((X[:, 2] > 0) & ((X @ R.T + t)[:, 2] > 0)).sum()))
    # the ratios front / n share their denominator: compared as integers
    choice = 1 if max(front[0], front[1]) > max(front[2], front[3]) else 2
    return dict(out, Rc=(R1 if choice == 1 else R2).T.copy(), front=np.array(front, dtype=np.int32), choice=choice, det_flip=flip)


def finite_item(item):
    return bool(np.all(np.isfinite(np.asarray(item["pts"], dtype=np.float64))))


def relative_rotations(item):
    """Step 1 of every consecutive pair: a dict of arrays over the F - 1 pairs (status, Rc, n_corres, front, choice, det_flip)."""
    P = item["n_frames"] - 1
    if not finite_item(item):
        return dict(status=NOT_FINITE, Rc=np.full((P, 3, 3), np.nan), n_corres=np.zeros(P, dtype=np.int32),
                    front=np.zeros((P, 4), dtype=np.int32), choice=np.zeros(P, dtype=np.int32), det_flip=np.zeros(P, dtype=bool))
    rs = [solve_relative_r(pair_correspondences(item, k)) for k in range(P)]
    return dict(status=OK if all(r["finite"] for r in rs) else NOT_FINITE, Rc=np.array([r["Rc"] for r in rs]).reshape(P, 3, 3),
                n_corres=np.array([r["n_corres"] for r in rs], dtype=np.int32), front=np.array([r["front"] for r in rs]).reshape(P, 4),
                choice=np.array([r["choice"] for r in rs], dtype=np.int32), det_flip=np.array([r["det_flip"] for r in rs], dtype=bool))


# ---- steps 2-5 -----------------------------------------------------------------------------------------
def quat_left(q):
    """L(q) over (x, y, z, w) for q = (w, x, y, z) (initial_ex_rotation.cpp:33-38)."""
    w, x, y, z = q
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def quat_right(q):
    w, x, y, z = q
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])


def angular_distance_deg(a, b):
    """Eigen's Quaternion::angularDistance of (w, x, y, z) quaternions, in degrees: d = a * conj(b), 2 atan2(|vec d|, |d.w|)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b[0], -b[1], -b[2], -b[3]
    dw = aw * bw - ax * bx - ay * by - az * bz
    dx = aw * bx + ax * bw + ay * bz - az * by
    dy = aw * by + ay * bw + az * bx - ax * bz
    dz = aw * bz + az * bw + ax * by - ay * bx
    return 180.0 / np.pi * (2.0 * np.arctan2(np.sqrt(dx * dx + dy * dy + dz * dz), abs(dw)))


def calibrate(Rc, delta_q, cfg=None):
    """The recursion over the pairs.  Returns a dict: status, step (the first step that passed the gate, 1-based, or -1), q (w, x, y, z)
    and ric at that step, and per step step_q, step_ric, sigma (the three smallest singular values, descending), huber."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    Rc = np.asarray(Rc, dtype=np.float64).reshape(-1, 3, 3)
    dq = np.asarray(delta_q, dtype=np.float64).reshape(-1, 4)
    P = len(Rc)
    out = dict(status=NOT_FINITE, step=-1, q=np.full(4, np.nan), ric=np.full((3, 3), np.nan), step_q=np.full((P, 4), np.nan),
               step_ric=np.full((P, 3, 3), np.nan), sigma=np.full((P, 3), np.nan), huber=np.full(P, np.nan))
    if not (np.all(np.isfinite(Rc)) and np.all(np.isfinite(dq))):
        return out
    ric = np.eye(3)
    N = np.zeros((4, 4))
    step_q, step_ric, sigma, huber = [], [], [], []
    first = -1
    for k in range(P):
        Rimu = quat_to_rot(dq[k])
        D = quat_left(rot_to_quat(Rc[k])) - quat_right(rot_to_quat(Rimu))
        Rg = (ric.T @ Rimu) @ ric                                  # with the ric of the step before; kept as stored
        deg = angular_distance_deg(rot_to_quat(Rc[k]), rot_to_quat(Rg))
        h = cfg["huber_deg"] / deg if deg > cfg["huber_deg"] else 1.0
        M = ((D[0][:, None] * D[0][None, :] + D[1][:, None] * D[1][None, :]) + D[2][:, None] * D[2][None, :]) + D[3][:, None] * D[3][None, :]
        N = N + (h * h) * M                                        # = the sum over pairs 1 .. k in pair order: old weights never change
        w, V = jacobi_eigh(N)
        mi = int(np.argmin(w))
        order = sorted(range(4), key=lambda i: -w[i])
        x = V[:, mi]                                               # (x, y, z, w) of Quaterniond(x)
        ric = quat_to_rot(np.array([x[3], x[0], x[1], x[2]])).T
        step_q.append(rot_to_quat(ric))
        step_ric.append(ric)
        sigma.append(np.sqrt(np.maximum(w[order[1:]], 0.0)))
        huber.append(h)
        if first < 0 and k + 1 >= cfg["min_frames"] and sigma[-1][1] > cfg["min_sigma"]:
            first = k
    if not (np.all(np.isfinite(step_q)) and np.all(np.isfinite(step_ric)) and np.all(np.isfinite(sigma))):
        return out
    out.update(status=OK if first >= 0 else FAIL_NOT_OBSERVABLE, step=first + 1 if first >= 0 else -1, step_q=np.array(step_q).reshape(P, 4),
               step_ric=np.array(step_ric).reshape(P, 3, 3), sigma=np.array(sigma).reshape(P, 3), huber=np.array(huber))
    if first >= 0:
        out.update(q=out["step_q"][first].copy(), ric=out["step_ric"][first].copy())
    return out


def exrot(item, cfg=None):
    """Both stages: calibrate()'s dict with relative_rotations()'s under "pairs"."""
    pairs = relative_rotations(item)
    out = calibrate(pairs["Rc"], item["delta_q"], cfg)
    out["pairs"] = pairs
    return out


def make_calibrator(cfg=None):
    """The `calibrate_ric=` hook of StreamDriver(initialize=...): a callable(items) returning what ExrotHandle.exrot_batch returns."""
    return lambda items: [exrot(it, cfg) for it in items]


# ---- directly built windows ----------------------------------------------------------------------------
def rot_error_deg(A, B):
    """The angle of A^T B in degrees, from its skew part and its trace (atan2: exact down to rounding for small angles)."""
    M = A.T @ B
    s = 0.5 * np.sqrt((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2)
    return float(np.degrees(np.arctan2(s, (np.trace(M) - 1.0) / 2.0)))


def _rand_rot(rng, angle):
    ax = rng.normal(size=3)
    return sr.exp_so3(ax / np.linalg.norm(ax) * angle)


def make_window(seed, deg, F=11, noise=0.0, n_points=400, ric_angle=0.6, step=0.3):
    """A window with enough rotation for the reference's gate (the project's streams rotate too little between frames): a random ric of
    ric_angle rad, a body rotation of `deg` degrees per frame about a fresh random axis, random steps of `step` m, n_points points on a
    shell of radius 4 .. 12 m around the start, observed where they fall inside a +-1 normalised field of view; every maximal run of
    at least two consecutive frames a point is seen in is a track.  Returns (item, ric)."""
    rng = np.random.RandomState(seed)
    ric = _rand_rot(rng, ric_angle)
    Rb, pb = [np.eye(3)], [np.zeros(3)]
    for _ in range(F - 1):
        Rb.append(Rb[-1] @ _rand_rot(rng, np.radians(deg)))
        d = rng.normal(size=3)
        pb.append(pb[-1] + d / np.linalg.norm(d) * step)
    d = rng.normal(size=(n_points, 3))
    X = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(4.0, 12.0, size=(n_points, 1))
    obs = np.full((F, n_points, 2), np.nan)
    for f in range(F):
        Xc = (X - pb[f]) @ (Rb[f] @ ric)                           # rows: R_wc^T (X - p)
        z = Xc[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            uv = Xc[:, 0:2] / z[:, None]
        vis = (z > 0) & (np.abs(uv[:, 0]) <= 1.0) & (np.abs(uv[:, 1]) <= 1.0)
        obs[f, vis] = uv[vis] + noise * rng.normal(size=(int(vis.sum()), 2))
    sf, off, pts = [], [0], []
    for j in range(n_points):
        f = 0
        while f < F:
            if np.isnan(obs[f, j, 0]):
                f += 1
                continue
            g = f
            while g + 1 < F and not np.isnan(obs[g + 1, j, 0]):
                g += 1
            if g > f:
                sf.append(f)
                pts.extend(obs[f:g + 1, j])
                off.append(off[-1] + g - f + 1)
            f = g + 1
    dq = np.array([rot_to_quat(Rb[k].T @ Rb[k + 1]) for k in range(F - 1)])
    return dict(n_frames=F, start_frame=np.array(sf, dtype=np.int32), obs_offset=np.array(off, dtype=np.int64),
                pts=np.array(pts, dtype=np.float64).reshape(-1, 2), delta_q=dq), ric


def perturb_ulp(item, rng):
    """The item with every point moved by one ulp in a random direction (sfm_reference.perturb_ulp; delta_q stays)."""
    return sr.perturb_ulp(item, rng)
