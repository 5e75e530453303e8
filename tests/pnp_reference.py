"""The non-keyframe PnP of include/vio_pnp.h restated in numpy: what k_pnp_frames computes, sum by sum.

solve() is sfm_reference.solve_frame_by_pnp with the order of the sums as a parameter: "sequential" is that function bit for bit (one
accumulator per sum, the points in order); "wave64" is the kernel's: usable point m belongs to lane m mod 64, every lane sums its
points' terms in ascending order from 0.0, and the 64 lane sums are reduced by the butterfly v[i] += v[i ^ s], s = 1, 2, 4, 8, 16, 32
(every lane ends with the same bits; lane 0's are taken).  frames() is the whole call for one window: the usable points of every
frame (validity, in the observations' order), min_points, the statuses and fail_frame.

make_all_frames_window() cuts an all_image_frame window out of a stream: every stride-th frame a keyframe, the others not.
"""
import numpy as np

import sfm_reference as sr
from sfm_reference import (BA_GRADIENT_TOL, LM_DIAG_MAX, LM_DIAG_MIN, LM_MIN_RHO, LM_RADIUS0, LM_RADIUS_MIN, PNP_MAX_ITER, PNP_STEP_TOL,
                           _chol_solve, _cholesky, _jacobians, _lm_radius, _residuals, exp_so3)

MIN_POINTS = 6
MAX_FRAMES = 32
MAX_POINTS = 4096
WAVE = 64
OK, NOT_FINITE = 0, -3
FAIL_FEW_POINTS, FAIL_NO_POSE = 1, 2
DEFAULT_CFG = dict(min_points=MIN_POINTS)


def _wave_sum(terms):
    """terms (n, k): the k sums over the n points in the kernel's order."""
    n, k = terms.shape
    rows = (n + WAVE - 1) // WAVE
    pad = np.zeros((rows * WAVE, k))
    pad[:n] = terms
    pad = pad.reshape(rows, WAVE, k)
    v = np.zeros((WAVE, k))
    for r in range(rows):               # lane j: points j, j + 64, ... in ascending order (x + 0.0 is x for the lanes that ran out)
        v = v + pad[r]
    lanes = np.arange(WAVE)
    s = 1
    while s < WAVE:
        v = v + v[lanes ^ s]
        s *= 2
    assert np.all((v == v[0]) | np.isnan(v))
    return v[0]


def _linearize(R, t, X, obs, order, full=True):
    n = len(X)
    fr = np.zeros(n, dtype=np.int64)
    trk = np.arange(n)
    r, Xc, RX = _residuals(R[None], t[None], X, obs, trk, fr)
    r2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    if order == "sequential":
        cost = 0.5 * sr._seq_sum(r2)
        if not full:
            return cost, None, None
        Jc, _ = _jacobians(R[None], Xc, RX, fr)
        H = np.zeros((6, 6))
        g = np.zeros(6)
        for k in range(n):
            H = H + Jc[k].T @ Jc[k]
            g = g + Jc[k].T @ r[k]
        return cost, H, g
    assert order == "wave64", order
    if not full:
        return 0.5 * _wave_sum(r2[:, None])[0], None, None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Jc, _ = _jacobians(R[None], Xc, RX, fr)
        cols = [Jc[:, 0, x] * Jc[:, 0, y] + Jc[:, 1, x] * Jc[:, 1, y] for x in range(6) for y in range(x, 6)]
        cols += [Jc[:, 0, x] * r[:, 0] + Jc[:, 1, x] * r[:, 1] for x in range(6)]
        v = _wave_sum(np.stack(cols + [r2], axis=1))
    H = np.zeros((6, 6))
    e = 0
    for x in range(6):
        for y in range(x, 6):
            H[x, y] = H[y, x] = v[e]
            e += 1
    return 0.5 * v[27], H, v[21:27].copy()


def solve(R0, t0, X, obs, order="sequential"):
    """The Levenberg-Marquardt solve from the guess (R0, t0) over the points X (n, 3) seen at obs (n, 2).  Returns (ok, R, t,
    iterations, cost): ok is False when the cost at the guess is not finite or the result is not."""
    R, t = R0.copy(), t0.copy()
    cost, H, g = _linearize(R, t, X, obs, order)
    radius, v, it = LM_RADIUS0, 2.0, 0
    if not np.isfinite(cost):
        return False, R, t, it, cost
    if np.abs(g).max() <= BA_GRADIENT_TOL:
        return True, R, t, it, cost
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
            c2, _, _ = _linearize(R2, t2, X, obs, order, full=False)
            model = 0.5 * (lam * (d * D) @ d - d @ g)
            rho = (cost - c2) / model if np.isfinite(c2) and model > 0 else -1.0
        if ok and rho > LM_MIN_RHO:
            R, t = R2, t2
            cost, H, g = _linearize(R, t, X, obs, order)
            if np.abs(g).max() <= BA_GRADIENT_TOL:
                break
            radius, v = _lm_radius(radius, rho), 2.0
        else:
            radius, v = radius / v, v * 2.0
            if radius < LM_RADIUS_MIN:
                break
    return bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t))), R, t, it, cost


def guess_pose(q, T):
    """R = Q^-1 (the quaternion's rotation matrix, transposed), t = -R T."""
    R = sr.quat_to_rot(np.asarray(q, dtype=np.float64)).T
    t = np.array([-((R[k, 0] * T[0] + R[k, 1] * T[1]) + R[k, 2] * T[2]) for k in range(3)])
    return R, t


def frames(item, cfg=None, order="wave64"):
    """vio_pnp_frames_batch for one window: a dict with status, fail_frame, Q (n, 4) wxyz, T (n, 3), frame_status, iterations,
    n_used and cost (n,)."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    gk = np.asarray(item["guess_key"], dtype=np.int64).reshape(-1)
    n = len(gk)
    off = np.asarray(item["obs_offset"], dtype=np.int64)
    op = np.asarray(item["obs_point"], dtype=np.int64).reshape(-1)
    ob = np.asarray(item["obs_pts"], dtype=np.float64).reshape(-1, 2)
    pts = np.asarray(item["points"], dtype=np.float64).reshape(-1, 3)
    valid = np.ones(len(pts), dtype=bool) if item.get("valid") is None else np.asarray(item["valid"]) != 0
    kq = np.asarray(item["key_Q"], dtype=np.float64).reshape(-1, 4)
    kt = np.asarray(item["key_T"], dtype=np.float64).reshape(-1, 3)
    out = dict(status=OK, fail_frame=-1, Q=np.full((n, 4), np.nan), T=np.full((n, 3), np.nan), frame_status=np.zeros(n, dtype=np.int32),
               iterations=np.zeros(n, dtype=np.int32), n_used=np.zeros(n, dtype=np.int32), cost=np.full(n, np.nan))
    for k in range(n):
        o, p = ob[off[k]:off[k + 1]], op[off[k]:off[k + 1]]
        use = valid[p]
        X = pts[p[use]]
        out["n_used"][k] = len(X)
        if not (np.all(np.isfinite(o)) and np.all(np.isfinite(X)) and np.all(np.isfinite(kq[gk[k]])) and np.all(np.isfinite(kt[gk[k]]))):
            out["frame_status"][k] = NOT_FINITE
            continue
        if len(X) < cfg["min_points"]:
            out["frame_status"][k] = FAIL_FEW_POINTS
            continue
        R0, t0 = guess_pose(kq[gk[k]], kt[gk[k]])
        ok, R, t, it, cost = solve(R0, t0, X, o[use], order)
        out["iterations"][k] = it
        if not np.isfinite(cost) and it == 0:
            out["frame_status"][k] = FAIL_NO_POSE
            continue
        Rt = R.T
        Q = sr.rot_to_quat(Rt)
        T = np.array([-((Rt[r, 0] * t[0] + Rt[r, 1] * t[1]) + Rt[r, 2] * t[2]) for r in range(3)])
        if not (ok and np.isfinite(cost) and np.all(np.isfinite(Q)) and np.all(np.isfinite(T))):
            out["frame_status"][k] = NOT_FINITE
            continue
        out["Q"][k], out["T"][k], out["cost"][k] = Q, T, cost
    st = out["frame_status"]
    if np.any(st == NOT_FINITE):
        out.update(status=NOT_FINITE, Q=np.full((n, 4), np.nan), T=np.full((n, 3), np.nan), cost=np.full(n, np.nan))
        out["frame_status"][:] = NOT_FINITE
        out["iterations"][:] = 0
        out["n_used"][:] = 0
    elif np.any(st != OK):
        k = int(np.nonzero(st != OK)[0][0])
        out.update(status=int(st[k]), fail_frame=k)
    return out


def perturb_ulp(item, rng):
    """The item with every image point of the non-keyframes moved by one ulp (sfm_reference.perturb_ulp on obs_pts)."""
    return dict(item, obs_pts=sr.perturb_ulp(dict(pts=item["obs_pts"]), rng)["pts"])


# ---- windows of all_image_frame --------------------------------------------------------------------------
def _seen(stream, lm, f):
    if stream.lm_host[lm] == f:
        return np.asarray(stream.lm_px[lm], dtype=np.float64)
    p = stream.lm_obs[lm].get(f)
    return None if p is None else np.asarray(p, dtype=np.float64)


def make_all_frames_window(stream, first, stride=2, n_key=11):
    """An all_image_frame window of a stream: the global frames first, first + stride, ... (n_key of them) are the keyframes, the
    frames in between are not.  Returns a dict: frames (global, time order), is_key, key_frames, sfm_item and ids (the keyframes'
    tracks, restricted to the keyframes, through item_from_tracks), all_frames (what pnp_items_from_sfm takes: per frame is_key and,
    for a non-keyframe, obs_point / obs_pts over the SfM item's tracks in landmark order, from the stream's lm_obs), pres and
    intervals (the stream's own, between consecutive frames)."""
    key_frames = [first + stride * k for k in range(n_key)]
    frames_ = list(range(first, key_frames[-1] + 1))
    tracks = {}
    for ki, f in enumerate(key_frames):
        for lm in range(len(stream.lm_host)):
            p = _seen(stream, lm, f)
            if p is None:
                continue
            if lm not in tracks:
                tracks[lm] = [(f, p)]
            elif tracks[lm][-1][0] == key_frames[ki - 1]:
                tracks[lm].append((f, p))
    item, ids = sr.item_from_tracks(tracks, key_frames)
    col = {lm: j for j, lm in enumerate(ids)}
    all_frames = []
    for f in frames_:
        if f in key_frames:
            all_frames.append(dict(is_key=True))
            continue
        op, ob = [], []
        for lm in sorted(col):
            p = _seen(stream, lm, f)
            if p is not None:
                op.append(col[lm])
                ob.append(p)
        all_frames.append(dict(is_key=False, obs_point=np.array(op, dtype=np.int32), obs_pts=np.array(ob, dtype=np.float64).reshape(-1, 2)))
    return dict(frames=frames_, is_key=[f in key_frames for f in frames_], key_frames=key_frames, sfm_item=item, ids=ids,
                all_frames=all_frames, pres=list(stream.preint[first:frames_[-1]]), intervals=list(stream.imu[first:frames_[-1]]))


def ground_truth_frames(stream, win, l):
    """The poses (Q (n, 4) wxyz, T (n, 3)) of the window's non-keyframes in camera frame key_frames[l] at the SfM's scale
    (sfm_reference.ground_truth over all the frames, scaled by the keyframes' |T[last]|)."""
    Rk, Tk, _, s = sr.ground_truth(stream, win["key_frames"], l, [])
    non = [f for f, k in zip(win["frames"], win["is_key"]) if not k]
    # ground_truth scales by the last frame's |T|: put the last keyframe last, take the others' rows
    R, T, _, s2 = sr.ground_truth(stream, [win["key_frames"][l]] + non + [win["key_frames"][-1]], 0, [])
    assert s2 == s
    return np.stack([sr.rot_to_quat(r) for r in R[1:-1]]), T[1:-1]


# ---- the committed fixtures -------------------------------------------------------------------------------
PX = 1.0 / 460.0
_FIXTURES = {}


def fixture(which, noisy=True):
    """The 21-frame window (first = 0, stride 2, 11 keyframes, 10 non-keyframes) of the synthetic stream ("syn", seed 3) or of the
    MH_05 stream ("mh", seed 7), 30 landmarks per frame tracked over 20 frames, at 0.1 px (noisy) or noise-free; computed once.
    Returns a dict: stream, win (make_all_frames_window's), sfm (sfm_reference.sfm of the keyframes), item (the PnP item)."""
    import os
    key = (which, bool(noisy))
    if key not in _FIXTURES:
        from conftest import load_package
        vio = load_package()
        noise = 0.1 * PX if noisy else 0.0
        if which == "syn":
            st = vio.stream.SyntheticStream(n_frames=22, landmarks_per_frame=30, track_len=20, seed=3, pixel_noise=noise)
        else:
            mh = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mh05_imu_stretch.npz")))
            st = vio.stream.RealImuStream(mh, n_frames=22, landmarks_per_frame=30, track_len=20, seed=7, pixel_noise=noise)
        win = make_all_frames_window(st, 0)
        res = sr.sfm(win["sfm_item"])
        assert res["status"] == sr.OK, (which, noisy, res["status"])
        item = vio.pnp_items_from_sfm([res], [win["sfm_item"]], [win["all_frames"]])[0]
        _FIXTURES[key] = dict(stream=st, win=win, sfm=res, item=item)
    return _FIXTURES[key]


def frame_item(item, k, keep=None):
    """Frame k of an item as a one-frame item; keep: the indices (into the frame's observations) that stay."""
    off = np.asarray(item["obs_offset"], dtype=np.int64)
    op, ob = np.asarray(item["obs_point"])[off[k]:off[k + 1]], np.asarray(item["obs_pts"]).reshape(-1, 2)[off[k]:off[k + 1]]
    if keep is not None:
        op, ob = op[keep], ob[keep]
    return dict(item, guess_key=np.asarray(item["guess_key"])[k:k + 1], obs_offset=np.array([0, len(op)], dtype=np.int64),
                obs_point=np.ascontiguousarray(op), obs_pts=np.ascontiguousarray(ob))


def synthetic_frame(n, seed):
    """A flat one-frame problem of n points in front of a camera a few centimetres and degrees off its guess; every point valid."""
    rng = np.random.RandomState(seed)
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(4, 10, n)], axis=1)
    R = exp_so3(rng.normal(0, 0.02, 3))
    t = rng.normal(0, 0.05, 3)
    Xc = X @ R.T + t
    obs = Xc[:, 0:2] / Xc[:, 2:3] + rng.normal(0, 0.1 * PX, (n, 2))
    return dict(points=X, valid=None, key_Q=np.array([[1.0, 0, 0, 0]]), key_T=np.zeros((1, 3)), guess_key=np.zeros(1, dtype=np.int32),
                obs_offset=np.array([0, n], dtype=np.int64), obs_point=np.arange(n, dtype=np.int32), obs_pts=obs)
