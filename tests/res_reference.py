"""numpy reference of the residual query (include/vio_residuals.h), built from the oracle's own pieces:
vioo_reproj_edge / vioo_reproj_xyz_edge for the residuals, vioo_loss for rho0, vioo_imu_edge and vioo_inverse15 for the IMU chi2.
Shared by test_residuals_reference.py (CPU) and test_gpu_residuals.py."""
import ctypes as C

import numpy as np

NF, NW = 11, 10
FOCAL = 460.0


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _rot(q):
    """Eigen toRotationMatrix of (x, y, z, w)."""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _depth(poses, ext, w, e, vals, xyz):
    """The point's depth in the observing camera (the sign is all the flags use)."""
    ric, tic = _rot(ext[3:7]), ext[0:3]
    fj = int(w.frame[e] if xyz else w.target[e])
    Rj, Pj = _rot(poses[fj, 3:7]), poses[fj, 0:3]
    if xyz:
        pw = np.asarray(vals[int(w.lm[e])], dtype=np.float64)
    else:
        fi = int(w.host[e])
        Ri, Pi = _rot(poses[fi, 3:7]), poses[fi, 0:3]
        lam = vals[int(w.lm[e])]
        pi = np.array([w.pts_i[e][0], w.pts_i[e][1], 1.0]) / lam
        pw = Ri @ (ric @ pi + tic) + Pi
    return (ric.T @ (Rj.T @ (pw - Pj) - tic))[2]


def reference(oracle_lib, vio, cfg, w, poses, sb, ext, vals, err_prior, focal=FOCAL, outlier_px=3.0, imu=True):
    """(obs (m, 4), lm (n, 3), flags (n,) uint8, summary dict) at the state (poses, sb, ext, vals, err_prior), under the rules of
    include/vio_residuals.h.  imu=False: the IMU fields and chi2 are NaN (pre == NULL)."""
    xyz = getattr(w, "xyz", None) is not None
    d = oracle_lib.dll
    fe, fx, fl, fi, finv = d.vioo_reproj_edge, d.vioo_reproj_xyz_edge, d.vioo_loss, d.vioo_imu_edge, d.vioo_inverse15
    for f in (fe, fx, fl, fi, finv):
        f.restype = None
    poses, sb, ext = _c(poses), _c(sb), _c(ext)
    n = len(vals)
    lm = np.asarray(w.lm)
    m = lm.size
    s2 = cfg.reproj_sqrt_info ** 2
    obs = np.zeros((m, 4))
    dneg = np.zeros(m, dtype=bool)
    r, rho = np.zeros(2), np.zeros(3)
    fr = np.asarray(w.frame if xyz else w.target)
    for e in range(m):
        l = int(lm[e])
        if xyz:
            fx(_dp(_c(poses[fr[e]])), _dp(ext), _dp(_c(vals[l])), _dp(_c(w.pts[e])), _dp(r), None, None)
        else:
            fe(_dp(_c(poses[int(w.host[e])])), _dp(_c(poses[fr[e]])), _dp(ext), C.c_double(vals[l]), _dp(_c(w.pts_i[e])),
               _dp(_c(w.pts_j[e])), _dp(r), None, None, None, None)
        e2 = r[0] * (s2 * r[0]) + r[1] * (s2 * r[1])                 # Edge::Chi2
        fl(C.c_int(cfg.loss_type), C.c_double(cfg.loss_delta), C.c_double(e2), _dp(rho))
        obs[e] = (r[0], r[1], e2, rho[0])
        dneg[e] = _depth(poses, ext, w, e, vals, xyz) <= 0.0
    px = focal * np.sqrt(obs[:, 0] ** 2 + obs[:, 1] ** 2)
    cnt = np.bincount(lm, minlength=n)
    lmo = np.zeros((n, 3))
    flags = np.zeros(n, dtype=np.uint8)
    for e in range(m):                                              # (a landmark's edges in the caller's order)
        l = lm[e]
        lmo[l, 0] += px[e]
        lmo[l, 1] = px[e] if np.isnan(px[e]) or np.isnan(lmo[l, 1]) else max(lmo[l, 1], px[e])
        lmo[l, 2] += obs[e, 3]
        if dneg[e]:
            flags[l] |= 2
    has = cnt > 0
    lmo[has, 0] /= cnt[has]
    flags[has & ~(lmo[:, 0] <= outlier_px)] |= 1
    vals = np.asarray(vals, dtype=np.float64)
    bad_state = ~np.all(np.isfinite(vals.reshape(n, -1)), axis=1) if xyz else ~((vals > 0) & np.isfinite(vals))
    flags[bad_state] |= 4

    imu_edge = np.full(NW, np.nan)
    if imu:
        for k, p in enumerate(w.preint):
            if p is None:
                imu_edge[k] = 0.0
                continue
            pre = p if isinstance(p, vio.VioPreint) else vio.VioPreint.from_dict(p)
            rr, info = np.zeros(15), np.zeros(225)
            fi(C.byref(pre), _dp(_c(cfg.gravity[:])), _dp(_c(poses[k])), _dp(_c(sb[k])), _dp(_c(poses[k + 1])), _dp(_c(sb[k + 1])),
               _dp(rr), None, None, None, None)
            finv(_dp(_c(np.frombuffer(pre.covariance, dtype=np.float64))), _dp(info))
            imu_edge[k] = float(rr @ (info.reshape(15, 15) @ rr))
    prior = float(np.sqrt(np.sum(np.asarray(err_prior, dtype=np.float64) ** 2)))
    vr, vp = float(obs[:, 3].sum()), float(obs[:, 2].sum())
    summary = {
        "visual_robust": vr, "visual_plain": vp, "imu_edge": imu_edge, "imu": float(imu_edge.sum()), "prior": prior,
        "chi2": 0.5 * (vr + float(imu_edge.sum()) + prior),
        "frame_robust": np.bincount(fr, weights=obs[:, 3], minlength=NF)[:NF],
        "frame_edges": np.bincount(fr, minlength=NF)[:NF],
        "n_flagged": np.array([np.count_nonzero(flags & b) for b in (1, 2, 4)]),
    }
    return obs, lmo, flags, summary


def reference_of(oracle_lib, vio, ctx, w, **kw):
    """reference() at the state a context (HIP or oracle) holds now."""
    poses, sb, ext = ctx.get_window()
    xyz = getattr(w, "xyz", None) is not None
    vals = ctx.get_landmarks_xyz() if xyz else ctx.get_landmarks()
    _, err = ctx.get_prior()
    return reference(oracle_lib, vio, ctx.cfg, w, poses, sb, ext, vals, err, **kw)


# (name, landmarks, loss, ext_fixed, marginalisation prior, xyz, missing IMU edge)
CASES = [
    ("trivial", 80, 0, 0, False, False, None),
    ("huber", 80, 1, 0, False, False, None),
    ("cauchy", 80, 2, 0, False, False, None),
    ("tukey", 80, 3, 0, False, False, None),
    ("cauchy_extfixed", 80, 2, 1, False, False, None),
    ("xyz_cauchy", 60, 2, 0, False, True, None),
    ("prior_cauchy", 100, 2, 0, True, False, None),
    ("missing_imu_edge", 60, 0, 0, False, False, 4),
]


def make_case(vio, oracle_lib, case):
    """(window, context overrides) of one of CASES.  The prior is MargOldFrame of a neighbouring window, made with the oracle."""
    name, n, loss, ext_fixed, marg, xyz, missing = case
    make = vio.synth.make_window_xyz if xyz else vio.synth.make_window
    w = make(n, seed=6 if missing is not None else 3, t0=1.1)
    kw = dict(ext_fixed=ext_fixed, loss_type=loss)
    if loss in (1, 3):              # (at delta = 1 every edge of these windows lies beyond delta; Tukey gives such an edge zero weight,
        kw["loss_delta"] = 5.0 if loss == 1 else 50.0      # and a landmark whose edges all have it leaves the solve singular)
    if missing is not None:
        w.preint = list(w.preint)
        w.preint[missing] = None
    if marg:
        w0 = vio.synth.make_window(n, seed=4)
        c0 = oracle_lib.context(**kw)
        c0.load(w0)
        c0.solve(5)
        w.prior = c0.marginalize(vio.MARG_OLD)
    return w, kw


def corrupt(vio, w, fraction=0.05, seed=11, lo_px=15.0, hi_px=30.0):
    """Shift every target observation of a seeded `fraction` of the landmarks by lo_px .. hi_px pixels in a random direction; returns
    the corrupted landmarks (bool, n)."""
    rng = np.random.RandomState(seed)
    n = w.n_landmarks
    bad = np.zeros(n, dtype=bool)
    bad[rng.choice(n, int(round(fraction * n)), replace=False)] = True
    w.pts_j = np.array(w.pts_j, dtype=np.float64)
    for e in np.nonzero(bad[np.asarray(w.lm)])[0]:
        a = rng.uniform(0, 2 * np.pi)
        w.pts_j[e] += rng.uniform(lo_px, hi_px) / vio.synth.FOCAL * np.array([np.cos(a), np.sin(a)])
    return bad


def recall_precision(flags, truth):
    hit = (flags & 1).astype(bool)
    tp = np.count_nonzero(hit & truth)
    return tp / max(1, np.count_nonzero(truth)), tp / max(1, np.count_nonzero(hit))


# the seeded outlier case: make_window(2000, seed=OUTLIER_SEED), 5 % of the landmarks shifted by 15 - 30 px, solve(10) under Cauchy,
# bit 0 at 3 px.  On the oracle's solve the reference flags exactly the 100 corrupted landmarks: recall and precision 1.0, with the
# clean landmarks' mean error at most 2.32 px and the corrupted ones' at least 9.68 px (seeds 22 and 23 give the same).  Those margins
# are far beyond what separates two solvers' states, so the thresholds are the measured values.
OUTLIER_SEED = 21
RECALL_MIN = 1.0
PRECISION_MIN = 1.0


def outlier_window(vio):
    w = vio.synth.make_window(2000, seed=OUTLIER_SEED)
    truth = corrupt(vio, w)
    return w, truth
