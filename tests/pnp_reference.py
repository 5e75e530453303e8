"""The non-keyframe PnP of include/vio_pnp.h restated in numpy: what k_pnp_frames computes, sum by sum.

solve() is sfm_reference.solve_frame_by_pnp with the order of the sums as a parameter: "sequential" is that function bit for bit (one
accumulator per sum, the points in order, every small product numpy's `@`); "wave64" is the kernel's: usable point m belongs to lane
m mod 64, every lane sums its points' terms in ascending order from 0.0, and the 64 lane sums are reduced by the butterfly
v[i] += v[i ^ s], s = 1, 2, 4, 8, 16, 32 (every lane ends with the same bits; lane 0's are taken).  Under "wave64" the operations per
point and per iteration are the kernel's too, one by one: the residual, the Jacobian and the 28 products (_wave_terms), the 6 x 6
factorisation and substitutions (_factor_solve), the step's rotation (_step_rotation), the three sums over the six unknowns (_dot) and
the cube of the radius rule as x * x * x (_lm_radius_wave).  numpy's `@` and einsum take those sums in another order or fused, which
is a last-bit difference that nothing showed while every frame ran three or four accepted steps; with a point at depth 1e-120 in the
guess camera the pivots of the factorisation are differences of numbers of 1e240 and their sign hangs on that bit.  Measured on the
CPU over LIMIT_CASES, the restatement as it was (`@` everywhere) against this one: z1e-120_seed13 20 iterations for 15,
z1e-120_seed31 8 for 17, z1e-120_seed172 10 for 18, z1e-150_seed192 8 for 16, z1e-150_seed328 another pose (Q by 1.6e-2) at the same
count; no other case moves by a third of its bar, and the 20 fixture frames of test_gpu_pnp.py move by at most 1.1e-16 (Q), 3.0e-15
(T).  One at a time: the factorisation's and the linearisation's order each move such counts; the step's rotation, the dots and the
cube move no count and no result by more than 4e-16.  On the device every one of those frames has this restatement's count and bits
(tests/test_gpu_pnp_limits.py).  What is left to differ from the device is sin and cos in the step's rotation.
solve() reports the branches it takes (trace); frames() is the whole call for one window: the usable points of every frame (validity,
in the observations' order), min_points, the statuses and fail_frame.

make_all_frames_window() cuts an all_image_frame window out of a stream: every stride-th frame a keyframe, the others not.
far_frame(), near_frame() and LIMIT_CASES are the problems of tests/test_gpu_pnp_limits.py, off the loop's easy path.
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


def _wave_terms(R, t, X, obs, full):
    """Per point, in the kernel's operations (residual and jac_cam of csrc/vio_sfm_math.h, wave_sums of csrc/vio_pnp.hip): the 27
    products of J^T J and J^T r (with full) and r^2, one column each.  Every three-term sum is (a + b) + c, the products with the
    zeros of the projection's Jacobian included."""
    RX = [(R[k, 0] * X[:, 0] + R[k, 1] * X[:, 1]) + R[k, 2] * X[:, 2] for k in range(3)]
    Xc = [RX[k] + t[k] for k in range(3)]
    r = [Xc[0] / Xc[2] - obs[:, 0], Xc[1] / Xc[2] - obs[:, 1]]
    r2 = r[0] * r[0] + r[1] * r[1]
    if not full:
        return r2[:, None]
    iz = 1.0 / Xc[2]
    zero = np.zeros(len(X))
    Jpr = [[iz, zero, -Xc[0] * iz * iz], [zero, iz, -Xc[1] * iz * iz]]
    S = [[zero, RX[2], -RX[1]], [-RX[2], zero, RX[0]], [RX[1], -RX[0], zero]]
    Jc = [[(Jpr[a][0] * S[0][c] + Jpr[a][1] * S[1][c]) + Jpr[a][2] * S[2][c] for c in range(3)] + Jpr[a] for a in range(2)]
    cols = [Jc[0][x] * Jc[0][y] + Jc[1][x] * Jc[1][y] for x in range(6) for y in range(x, 6)]
    cols += [Jc[0][x] * r[0] + Jc[1][x] * r[1] for x in range(6)]
    return np.stack(cols + [r2], axis=1)


def _linearize(R, t, X, obs, order, full=True):
    if order == "sequential":
        n = len(X)
        fr = np.zeros(n, dtype=np.int64)
        trk = np.arange(n)
        r, Xc, RX = _residuals(R[None], t[None], X, obs, trk, fr)
        r2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
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
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = _wave_sum(_wave_terms(R, t, X, obs, full))
    if not full:
        return 0.5 * v[0], None, None
    H = np.zeros((6, 6))
    e = 0
    for x in range(6):
        for y in range(x, 6):
            H[x, y] = H[y, x] = v[e]
            e += 1
    return 0.5 * v[27], H, v[21:27].copy()


def _factor_solve(A, b, order):
    """x with A x = b through the lower Cholesky factor of A, or None when a pivot is not positive.  "sequential" is
    sfm_reference's pair, whose sums are numpy's `@`; "wave64" is the kernel's cholesky_solve6 sum by sum: every sum starts at 0.0
    and takes its terms in ascending k.  The two orders round differently, which decides a pivot's sign where H holds entries of
    1e240 and more (a point at depth 1e-120 in the guess camera): there, and nowhere else in the suites, the iteration counts differ."""
    if order == "sequential":
        L = _cholesky(A)
        return None if L is None else _chol_solve(L, b)
    n = len(b)
    L = A.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            d = 0.0
            for k in range(j):
                d = d + L[j, k] * L[j, k]
            d = L[j, j] - d
            if not d > 0.0:
                return None
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, n):
                s = 0.0
                for k in range(j):
                    s = s + L[i, k] * L[j, k]
                L[i, j] = (L[i, j] - s) / L[j, j]
        y, x = np.zeros(n), np.zeros(n)
        for i in range(n):
            s = 0.0
            for k in range(i):
                s = s + L[i, k] * y[k]
            y[i] = (b[i] - s) / L[i, i]
        for i in range(n - 1, -1, -1):
            s = 0.0
            for k in range(i + 1, n):
                s = s + L[k, i] * x[k]
            x[i] = (y[i] - s) / L[i, i]
    return x


def _lm_radius_wave(radius, rho):
    """sfm_reference._lm_radius with the cube as the kernel's product x * x * x (`** 3` is pow, which may round otherwise)."""
    x = 2.0 * rho - 1.0
    return min(radius / max(1.0 / 3.0, 1.0 - x * x * x), sr.LM_RADIUS_MAX)


def _dot(a, b):
    """sum a[k] b[k] from 0.0 in ascending k, as the kernel's loops over the six unknowns take it."""
    s = 0.0
    for x, y in zip(a, b):
        s = s + x * y
    return s


def _step_rotation(w, R):
    """exp_so3(w) R in the operations of csrc/vio_sfm_math.h's exp_so3 and mm3: every three-term sum is (a + b) + c."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = np.sqrt(th2)
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = sr.skew(w)
    E = np.array([[((1.0 if r == c else 0.0) + a * K[r, c]) + b * (K[r, 0] * K[0, c] + K[r, 1] * K[1, c] + K[r, 2] * K[2, c]) for c in range(3)]
                  for r in range(3)])
    return np.array([[E[r, 0] * R[0, c] + E[r, 1] * R[1, c] + E[r, 2] * R[2, c] for c in range(3)] for r in range(3)])


EVENTS = ("nocost", "grad0", "diagmin", "cholfail", "steptol", "c2_not_finite", "model_not_positive", "accept", "reject", "gradtol", "radmin",
          "maxiter")


def solve(R0, t0, X, obs, order="sequential", trace=None):
    """The Levenberg-Marquardt solve from the guess (R0, t0) over the points X (n, 3) seen at obs (n, 2).  Returns (ok, R, t,
    iterations, cost): ok is False when the cost at the guess is not finite or the result is not.

    trace: a list that receives the names (EVENTS) of the branches the solve takes, in order.  Before the loop: nocost (the cost at
    the guess is not finite), grad0 (the gradient test holds at the guess).  Per iteration: diagmin (an entry of diag H below
    LM_DIAG_MIN when D is formed), then one of cholfail (no factorisation: the radius shrinks), steptol, accept, reject (a factorised
    step with rho <= LM_MIN_RHO: the radius shrinks), the last two after c2_not_finite / model_not_positive where those force
    rho = -1; gradtol after the accept it follows, radmin after the cholfail or reject it follows.  maxiter: the loop ran out.
    Tracing adds no arithmetic."""
    ev = (lambda name: None) if trace is None else trace.append
    wave = order == "wave64"
    R, t = R0.copy(), t0.copy()
    cost, H, g = _linearize(R, t, X, obs, order)
    radius, v, it = LM_RADIUS0, 2.0, 0
    if not np.isfinite(cost):
        ev("nocost")
        return False, R, t, it, cost
    if np.abs(g).max() <= BA_GRADIENT_TOL:
        ev("grad0")
        return True, R, t, it, cost
    while it < PNP_MAX_ITER:
        it += 1
        lam = 1.0 / radius
        if trace is not None and np.any(np.diag(H) < LM_DIAG_MIN):
            ev("diagmin")
        D = np.clip(np.diag(H), LM_DIAG_MIN, LM_DIAG_MAX)
        A = H + lam * np.diag(D)
        d = _factor_solve(A, -g, order)
        ok = d is not None
        if ok:
            if np.sqrt(_dot(d, d) if wave else d @ d) <= PNP_STEP_TOL:
                ev("steptol")
                break
            R2, t2 = _step_rotation(d[0:3], R) if wave else exp_so3(d[0:3]) @ R, t + d[3:6]
            c2, _, _ = _linearize(R2, t2, X, obs, order, full=False)
            model = 0.5 * (lam * _dot(d * D, d) - _dot(d, g)) if wave else 0.5 * (lam * (d * D) @ d - d @ g)
            if trace is not None and not np.isfinite(c2):
                ev("c2_not_finite")
            if trace is not None and not model > 0:
                ev("model_not_positive")
            rho = (cost - c2) / model if np.isfinite(c2) and model > 0 else -1.0
        else:
            ev("cholfail")
        if ok and rho > LM_MIN_RHO:
            ev("accept")
            R, t = R2, t2
            cost, H, g = _linearize(R, t, X, obs, order)
            if np.abs(g).max() <= BA_GRADIENT_TOL:
                ev("gradtol")
                break
            radius, v = _lm_radius_wave(radius, rho) if wave else _lm_radius(radius, rho), 2.0
        else:
            if ok:
                ev("reject")
            radius, v = radius / v, v * 2.0
            if radius < LM_RADIUS_MIN:
                ev("radmin")
                break
    else:
        ev("maxiter")
    return bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t))), R, t, it, cost


def guess_pose(q, T):
    """R = Q^-1 (the quaternion's rotation matrix, transposed), t = -R T."""
    R = sr.quat_to_rot(np.asarray(q, dtype=np.float64)).T
    t = np.array([-((R[k, 0] * T[0] + R[k, 1] * T[1]) + R[k, 2] * T[2]) for k in range(3)])
    return R, t


def frames(item, cfg=None, order="wave64", traces=None):
    """vio_pnp_frames_batch for one window: a dict with status, fail_frame, Q (n, 4) wxyz, T (n, 3), frame_status, iterations,
    n_used and cost (n,).  traces: a list that receives one list of solve()'s events per frame (empty for a frame that is not solved)."""
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
        tr = None
        if traces is not None:
            tr = []
            traces.append(tr)
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
        ok, R, t, it, cost = solve(R0, t0, X, o[use], order, tr)
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


# ---- one-frame problems off the easy path (tests/test_gpu_pnp_limits.py) ----------------------------------
def _one_frame(X, obs, Rg, tg, R, t):
    """The one-frame item of points X seen at obs with the guess camera (Rg, tg); true_Q / true_T: the pose (R, t) the observations
    were made from, in the output's convention (Q = Quaternion(R^T), T = -R^T t).  The library reads neither of the two."""
    n = len(X)
    return dict(points=X, valid=None, key_Q=sr.rot_to_quat(Rg.T)[None], key_T=-(Rg.T @ tg)[None], guess_key=np.zeros(1, dtype=np.int32),
                obs_offset=np.array([0, n], dtype=np.int64), obs_point=np.arange(n, dtype=np.int32), obs_pts=obs,
                true_Q=sr.rot_to_quat(R.T), true_T=-(R.T @ t))


def far_frame(n, seed, rot, tr, noise=0.1 * PX, depth=(4.0, 10.0), lateral=3.0):
    """synthetic_frame's points (x, y within +-lateral, z within depth) and identity guess, seen by a camera rot radians about a
    random axis and tr metres (in a random direction) off that guess, at `noise` of image noise."""
    rng = np.random.RandomState(seed)
    X = np.stack([rng.uniform(-lateral, lateral, n), rng.uniform(-lateral, lateral, n), rng.uniform(depth[0], depth[1], n)], axis=1)
    axis, way = rng.normal(size=3), rng.normal(size=3)
    R = exp_so3(rot * axis / np.linalg.norm(axis))
    t = tr * way / np.linalg.norm(way)
    Xc = X @ R.T + t
    obs = Xc[:, 0:2] / Xc[:, 2:3] + rng.normal(0, 1.0, (n, 2)) * noise
    item = _one_frame(X, obs, np.eye(3), np.zeros(3), R, t)
    return dict(item, key_Q=np.array([[1.0, 0, 0, 0]]), key_T=np.zeros((1, 3)))


def near_frame(n, seed, axis, angle, noise=0.1 * PX):
    """A camera rotated `angle` about coordinate axis `axis`, times a small random rotation, with the points in front of that camera
    and a guess about 0.02 rad and 5 cm off it: an easy solve whose output rotation is large."""
    rng = np.random.RandomState(seed)
    e = np.zeros(3)
    e[axis] = angle
    R = exp_so3(e) @ exp_so3(rng.normal(0, 0.01, 3))
    t = rng.normal(0, 0.05, 3)
    Xc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(4, 10, n)], axis=1)
    X = (Xc - t) @ R
    obs = Xc[:, 0:2] / Xc[:, 2:3] + rng.normal(0, 1.0, (n, 2)) * noise
    Rg = exp_so3(rng.normal(0, 0.02 / np.sqrt(3.0), 3)) @ R
    tg = t + rng.normal(0, 0.05 / np.sqrt(3.0), 3)
    return _one_frame(X, obs, Rg, tg, R, t)


def exact_guess(item):
    """The one-frame item with the pose its observations were made from as the guess."""
    return dict(item, key_Q=item["true_Q"][None].copy(), key_T=item["true_T"][None].copy())


def join_frames(items):
    """One window of one-frame items: every frame keeps its own slice of points and its own key pose."""
    base = np.concatenate([[0], np.cumsum([len(it["points"]) for it in items])])
    off = np.concatenate([[0], np.cumsum([len(it["obs_point"]) for it in items])]).astype(np.int64)
    valid = None
    if any(it.get("valid") is not None for it in items):
        valid = np.concatenate([np.ones(len(it["points"]), dtype=bool) if it.get("valid") is None else np.asarray(it["valid"]) != 0 for it in items])
    return dict(points=np.concatenate([np.asarray(it["points"], dtype=np.float64).reshape(-1, 3) for it in items]), valid=valid,
                key_Q=np.concatenate([np.asarray(it["key_Q"])[np.asarray(it["guess_key"])] for it in items]),
                key_T=np.concatenate([np.asarray(it["key_T"])[np.asarray(it["guess_key"])] for it in items]),
                guess_key=np.arange(len(items), dtype=np.int32), obs_offset=off,
                obs_point=np.concatenate([np.asarray(it["obs_point"]) + b for it, b in zip(items, base)]).astype(np.int32),
                obs_pts=np.concatenate([np.asarray(it["obs_pts"], dtype=np.float64).reshape(-1, 2) for it in items]))


# ---- the cases of tests/test_gpu_pnp_limits.py, and what the restatement must show on each ------------------
def shape(trace):
    """A solve's trace as one letter per iteration: A accept, R reject, C failed factorisation, S step tolerance."""
    return "".join(dict(accept="A", reject="R", cholfail="C", steptol="S").get(e, "") for e in trace)


def quat_branch(R):
    """The branch rot_to_quat takes on R: -1 where the trace is positive, else the index i of the largest diagonal entry as it finds it."""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return -1
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 2 if R[2, 2] > R[i, i] else i


def _scaled(item, points=1.0, obs=1.0, quat=1.0):
    return dict(item, points=item["points"] * points, obs_pts=item["obs_pts"] * obs, key_Q=item["key_Q"] * quat)


def _point_at(item, k, z):
    """The item with point k at (z, z, z): in the identity guess camera, at depth z on the ray (1, 1)."""
    P = item["points"].copy()
    P[k] = z
    return dict(item, points=P)


def _twice(item, a, b):
    """The item with observation b naming observation a's point: that point is seen twice, b's own not at all."""
    op = item["obs_point"].copy()
    op[b] = op[a]
    return dict(item, obs_point=op)


def _case(group, make, shape, ends, iters, cfg=None, status=OK, quat=None, **more):
    return dict(group=group, make=make, shape=shape, ends=ends, iters=iters, cfg=cfg, status=status, quat=quat, **more)


# name -> group, make() (a one-frame item), and what the restatement's solve of it must show: shape (a regular expression the whole
# of shape(trace) matches), ends (the event the solve leaves by), iters (lowest, highest count), status, quat (quat_branch of the
# result), every (an event that occurs in every iteration), cfg (min_points).  The figures were measured on the CPU; test_pnp_reference.py holds them.
LIMIT_CASES = {}
# rejected steps and the cap: five or six rejects in a row at the start (vv reaches 64), and where an R follows a later A the radius
# is divided by 2 again, not by the vv the earlier run left
for _rot, _seed, _shape, _ends, _it in ((0.8, 1, "R{4}A{8}S", "steptol", 13), (0.8, 2, "R{5}A{12}S", "steptol", 18), (0.8, 3, "R{6}A{14}", "maxiter", 20),
                                        (1.5, 2, "R{5}ARA+RAR+A+R+A", "maxiter", 20), (1.5, 5, "R{5}ARA{12}R", "maxiter", 20),
                                        (2.5, 1, "R{4}AR{3}A{6}RAR{3}A", "maxiter", 20), (2.5, 3, "A{4}R{5}A{11}", "maxiter", 20),
                                        (3.1, 1, "R{6}A{7}R{3}A{4}", "maxiter", 20), (3.1, 5, "AR{4}AR{2}A{12}", "maxiter", 20)):
    LIMIT_CASES["far_rot%.1f_seed%d" % (_rot, _seed)] = _case("reject", lambda r=_rot, s=_seed: far_frame(40, s, r, 1.0), _shape, _ends, (_it, _it))
# shallow points: steps that carry points through z = 0
LIMIT_CASES["shallow_seed1"] = _case("shallow", lambda: far_frame(20, 1, 0.2, 0.2, depth=(0.05, 0.3), lateral=0.05), "R{6}A{3}RA{8}R{2}", "maxiter", (20, 20))
LIMIT_CASES["shallow_seed2"] = _case("shallow", lambda: far_frame(20, 2, 0.2, 0.2, depth=(0.05, 0.3), lateral=0.1), "AR{5}ARA{10}RA", "maxiter", (20, 20))
# zero iterations with a pose
LIMIT_CASES["exact_guess"] = _case("zero", lambda: exact_guess(far_frame(24, 5, 0.5, 0.5, noise=0.0)), "", "grad0", (0, 0))
LIMIT_CASES["identity"] = _case("zero", lambda: far_frame(24, 5, 0.0, 0.0, noise=0.0), "", "grad0", (0, 0))
# the diagonal clamp: the translation block of H lies below LM_DIAG_MIN in every iteration
for _s, _shape, _ends, _it in ((1e6, "A{13}", "gradtol", 13), (1e12, "A{5}", "gradtol", 5), (1e150, "A{3}S", "steptol", 4)):
    LIMIT_CASES["points_x%g" % _s] = _case("diagmin", lambda s=_s: _scaled(synthetic_frame(24, 8), points=s), _shape, _ends, (_it, _it), every="diagmin")
# failed factorisations and the radius floor
for _z, _seed, _k, _shape, _ends, _it in ((1e-120, 13, 5, "C{7}AC{6}S", "steptol", 15), (1e-120, 31, 0, "AC{16}", "radmin", 17), (1e-120, 172, 8, "C{2}AC{15}", "radmin", 18),
                                         (1e-150, 192, 8, "C{6}AC{8}S", "steptol", 16), (1e-150, 328, 5, "C{5}AC{14}", "radmin", 20),
                                         (1e-154, 5, 5, "C{15}", "radmin", 15)):
    LIMIT_CASES["z%g_seed%d" % (_z, _seed)] = _case("cholfail", lambda z=_z, s=_seed, k=_k: _point_at(synthetic_frame(12, s), k, z), _shape, _ends, (_it, _it))
LIMIT_CASES["obs_x1e100"] = _case("cholfail", lambda: _scaled(synthetic_frame(12, 5), obs=1e100), "R{15}", "radmin", (15, 15))
LIMIT_CASES["obs_x1e160"] = _case("cholfail", lambda: _scaled(synthetic_frame(12, 5), obs=1e160), "", "nocost", (0, 0), status=FAIL_NO_POSE)
# output rotations above 120 degrees: rot_to_quat's else branch, i = axis
for _axis in range(3):
    for _angle in (2.2, 3.0, np.pi):
        LIMIT_CASES["near_axis%d_%.2f" % (_axis, _angle)] = _case("quat", lambda a=_axis, g=_angle: near_frame(24, 5, a, g), "A{3,4}S?", None, (3, 4),
                                                                  quat=_axis)
# guess quaternions that are not unit
LIMIT_CASES["guess_q_x3"] = _case("guess", lambda: _scaled(synthetic_frame(24, 5), quat=3.0), "A{3}S", "steptol", (4, 4))
LIMIT_CASES["guess_q_x0"] = _case("guess", lambda: _scaled(synthetic_frame(24, 5), quat=0.0), "A{3}S", "steptol", (4, 4))
# ... and one with a rotation in it: quat_to_rot gives a matrix that is no rotation, and the left-multiplied steps leave it so
LIMIT_CASES["guess_q_near_x3"] = _case("guess", lambda: _scaled(near_frame(24, 5, 0, 0.1), quat=3.0), "A{11}S", "steptol", (12, 12))
LIMIT_CASES["guess_q_near_x0.9"] = _case("guess", lambda: _scaled(near_frame(24, 5, 0, 0.1), quat=0.9), "A{3}S", "steptol", (4, 4))
# noise-free: the pose is also held to the one the frame was made from
for _rot, _seed in ((0.3, 1), (0.3, 7), (0.8, 1), (0.8, 7)):
    LIMIT_CASES["truth_rot%.1f_seed%d" % (_rot, _seed)] = _case("truth", lambda r=_rot, s=_seed: far_frame(40, s, r, 1.0, noise=0.0), "R*A+S", "steptol",
                                                                 (5, 16))
# accepted sizes at the edge
LIMIT_CASES["three_points"] = _case("sizes", lambda: synthetic_frame(3, 5), "A{3}", "gradtol", (3, 3), cfg=dict(min_points=3))
LIMIT_CASES["max_points"] = _case("sizes", lambda: synthetic_frame(MAX_POINTS, 3), "A+S?", None, (3, 4), cfg=dict(min_points=MAX_POINTS))
LIMIT_CASES["point_twice"] = _case("sizes", lambda: _twice(synthetic_frame(24, 5), 3, 7), "A{12}S", "steptol", (13, 13))
# the four fates of one workgroup (test_one_workgroup_four_fates): 0 iterations, an easy solve, the cap, the radius floor
FOUR_FATES = ("exact_guess", "guess_q_x3", "far_rot1.5_seed5", "z1e-120_seed31")
_LIMIT = {}


def limit_case(name):
    """(item, cfg, the restatement's window, the frame's trace) of a case of LIMIT_CASES, computed once."""
    if name not in _LIMIT:
        c = LIMIT_CASES[name]
        item, traces = c["make"](), []
        with np.errstate(all="ignore"):
            ref = frames(item, c["cfg"], traces=traces)
        _LIMIT[name] = (item, c["cfg"], ref, traces[0])
    return _LIMIT[name]


def check_limit_case(name):
    """Asserts that the restatement takes, on the case, the branches the case is there for; returns limit_case(name)."""
    import re
    c = LIMIT_CASES[name]
    item, cfg, ref, trace = limit_case(name)
    what = (name, shape(trace), [e for e in trace if e not in ("accept", "reject", "cholfail")], int(ref["iterations"][0]))
    assert ref["frame_status"][0] == c["status"], what
    assert re.fullmatch(c["shape"], shape(trace)), what
    assert c["iters"][0] <= ref["iterations"][0] <= c["iters"][1], what
    assert c["ends"] is None or trace[-1] == c["ends"], what
    if c.get("every"):
        assert trace.count(c["every"]) == ref["iterations"][0] > 0, what
    if c["quat"] is not None:
        assert quat_branch(sr.quat_to_rot(ref["Q"][0])) == c["quat"], what
    return item, cfg, ref, trace


def undecidable(item, cfg=None, seed=5):
    """The number of frames whose iteration count changes in the restatement when every image point moves by one ulp (two such
    perturbations, test_gpu_pnp._compare's): the device comparison skips those."""
    with np.errstate(all="ignore"):
        ref = frames(item, cfg)
        rng = np.random.RandomState(seed)
        runs = [frames(perturb_ulp(item, rng), cfg) for _ in range(2)]
    return int(np.sum(np.any([r["iterations"] != ref["iterations"] for r in runs], axis=0)))


def no_observations():
    """A one-frame item whose frame observes nothing."""
    return dict(points=np.zeros((0, 3)), valid=None, key_Q=np.array([[1.0, 0, 0, 0]]), key_T=np.zeros((1, 3)), guess_key=np.zeros(1, dtype=np.int32),
                obs_offset=np.zeros(2, dtype=np.int64), obs_point=np.zeros(0, dtype=np.int32), obs_pts=np.zeros((0, 2)))


def cycled(item, n):
    """A window of n frames: the item's frames 0, 1, ... over and over."""
    off = np.asarray(item["obs_offset"], dtype=np.int64)
    ks = [k % len(item["guess_key"]) for k in range(n)]
    return dict(item, guess_key=np.asarray(item["guess_key"])[ks],
                obs_offset=np.concatenate([[0], np.cumsum([off[k + 1] - off[k] for k in ks])]).astype(np.int64),
                obs_point=np.concatenate([np.asarray(item["obs_point"])[off[k]:off[k + 1]] for k in ks]),
                obs_pts=np.concatenate([np.asarray(item["obs_pts"]).reshape(-1, 2)[off[k]:off[k + 1]] for k in ks]))


FATES_PERMUTED = (2, 0, 3, 1)


def limit_windows():
    """The windows of more than one frame of tests/test_gpu_pnp_limits.py, by name: the four fates as one workgroup, permuted, and as
    frames 3 to 6 of seven (behind three easy frames, so they straddle two workgroups); a frame without observations between two
    solvable ones; VIO_PNP_MAX_FRAMES frames, the synthetic fixture's ten cycled."""
    fates = [limit_case(n)[0] for n in FOUR_FATES]
    return dict(four_fates=join_frames(fates), four_fates_permuted=join_frames([fates[k] for k in FATES_PERMUTED]),
                four_fates_straddling=join_frames([synthetic_frame(24, s) for s in (1, 2, 3)] + fates),
                empty_between=join_frames([fates[1], no_observations(), fates[2]]), full_window=cycled(fixture("syn")["item"], MAX_FRAMES))
