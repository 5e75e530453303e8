"""numpy restatement of the batched marginalisation's device algorithm (include/vio_marg.h, csrc/vio_marg.hip).

build(): k_marg_build — H_marg / b_marg of Problem::Marginalize's graph (problem.cc:617-713) from the oracle's edge pieces (vioo_reproj_edge,
vioo_robust_info2, vioo_imu_edge, vioo_inverse15), landmark by landmark in ascending order.
tail(): k_marg_tail — problem.cc:717-779 with the same parallel cyclic Jacobi eigen-solver (round-robin schedule, rotation test, stopping
rule), the same live-row rules and the same output layout.
tight_check(): a prior against the Schur complement in 50-digit arithmetic, with bars computed from the host references' own distance
from it; spectrum_check(): the invariants of jt_inv and err.  limit_cases(): the well-conditioned windows both are applied to.

Shared by test_marg_reference.py (CPU: build, tail and tight_check against the oracle), test_gpu_marg_batch.py (dense_input and
exact_schur behind the entry-wise bars of check_prior, and tail where vio_marginalize refuses a window) and test_gpu_marg_limits.py
(the device held to tight_check and spectrum_check, with tail and the oracle's prior as the references)."""
import ctypes as C
import math

import numpy as np

from conftest import load_package

PD, PRD, NF, M2 = 171, 156, 11, 15
EPS = 1e-8
JAC_EPS = 2.220446049250313e-16
JAC_MAX_SWEEPS = 40


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def build(oracle_lib, vio, cfg, kind, w, prior):
    """(H_marg (171 x 171), b_marg (171)) as k_marg_build forms them.  cfg: a VioConfig (loss, edge information, gravity)."""
    H, b = np.zeros((PD, PD)), np.zeros(PD)
    if kind == vio.MARG_OLD:
        dll = oracle_lib.dll
        fe, fr, fi, finv = dll.vioo_reproj_edge, dll.vioo_robust_info2, dll.vioo_imu_edge, dll.vioo_inverse15
        fe.restype = fr.restype = fi.restype = finv.restype = None
        poses, sb, ext = _c(w.poses).reshape(11, 7), _c(w.speed_bias).reshape(11, 9), _c(w.ext)
        s = cfg.reproj_sqrt_info
        lm, host, target = np.asarray(w.lm), np.asarray(w.host), np.asarray(w.target)
        r, Jl, Ji, Jj, Je = np.zeros(2), np.zeros(2), np.zeros(12), np.zeros(12), np.zeros(12)
        W, drho = np.zeros(4), C.c_double()
        for l in range(len(w.inv_depth)):
            es = np.nonzero(lm == l)[0]
            if len(es) == 0 or host[es[0]] != 0:
                continue
            hl, bl, wl = 0.0, 0.0, np.zeros(PD)
            for e in es:
                t = int(target[e])
                fe(_dp(_c(poses[0])), _dp(_c(poses[t])), _dp(ext), C.c_double(float(w.inv_depth[l])), _dp(_c(w.pts_i[e])),
                   _dp(_c(w.pts_j[e])), _dp(r), _dp(Jl), _dp(Ji), _dp(Jj), _dp(Je))
                fr(C.c_int(cfg.loss_type), C.c_double(cfg.loss_delta), C.c_double(s), _dp(r), C.byref(drho), _dp(W))
                Wm = W.reshape(2, 2)
                cols = list(range(6)) + list(range(6, 12)) + list(range(6 + 15 * t, 12 + 15 * t))
                Jc = np.hstack([Je.reshape(2, 6), Ji.reshape(2, 6), Jj.reshape(2, 6)])
                cvec = drho.value * (s * s) * r
                H[np.ix_(cols, cols)] += Jc.T @ Wm @ Jc
                b[cols] -= Jc.T @ cvec
                hl += Jl @ Wm @ Jl
                bl -= Jl @ cvec
                wl[cols] += Jc.T @ (Wm @ Jl)
            H -= np.outer(wl, wl) / hl
            b -= wl * (bl / hl)
        pre = w.preint[0] if w.preint is not None and len(w.preint) else None
        if pre is not None:
            p = pre if isinstance(pre, vio.VioPreint) else vio.VioPreint.from_dict(pre)
            res, Jpi, Jsi, Jpj, Jsj = np.zeros(15), np.zeros(90), np.zeros(135), np.zeros(90), np.zeros(135)
            g = _c(list(cfg.gravity))
            fi(C.byref(p), _dp(g), _dp(_c(poses[0])), _dp(_c(sb[0])), _dp(_c(poses[1])), _dp(_c(sb[1])), _dp(res), _dp(Jpi), _dp(Jsi),
               _dp(Jpj), _dp(Jsj))
            info = np.zeros(225)
            finv(_dp(_c(np.asarray(p.covariance))), _dp(info))
            J = np.hstack([Jpi.reshape(15, 6), Jsi.reshape(15, 9), Jpj.reshape(15, 6), Jsj.reshape(15, 9)])
            I = info.reshape(15, 15)
            H[6:36, 6:36] += J.T @ I @ J
            b[6:36] -= J.T @ (I @ res)
    if prior is not None:
        H[:PRD, :PRD] += np.asarray(prior["H"])
        b[:PRD] += np.asarray(prior["b"])[:PRD]
    return H, b


def marg_order(frame):
    """The index map of problem.cc:721-745: the frame's speed-bias to the bottom, then its pose."""
    def move(idx, dim, src):
        return [i for i in src if not (idx <= i < idx + dim)] + list(range(idx, idx + dim))
    o1 = move(12 + 15 * frame, 9, list(range(PD)))
    o2 = move(6 + 15 * frame, 6, list(range(PD)))
    return np.array([o1[o2[i]] for i in range(PD)])


def jacobi(A):
    """Eigenvalues (unsorted, the diagonal the sweeps leave) and V^T of a symmetric A (np even: the caller pads) by k_marg_tail's
    parallel cyclic Jacobi: only the lower triangle is read and updated, as the device's packed triangle."""
    A = np.tril(np.array(A, dtype=np.float64))
    n = A.shape[0]
    Vt = np.eye(n)
    if n == 0:
        return np.zeros(0), Vt
    npairs = n // 2

    def player(pos, r):
        return 0 if pos == 0 else 1 + (pos - 1 + r) % (n - 1)
    for _ in range(JAC_MAX_SWEEPS):
        any_rot = False
        for r in range(n - 1):
            P, Q, Cs, Ss = [], [], [], []
            for k in range(npairs):
                p, q = sorted((player(k, r), player(n - 1 - k, r)))
                app, aqq, apq = A[p, p], A[q, q], A[q, p]
                c, s = 1.0, 0.0
                if apq != 0.0 and not (abs(apq) <= JAC_EPS * np.sqrt(abs(app) * abs(aqq))):
                    th = (aqq - app) / (2.0 * apq)
                    t = 0.5 / th if abs(th) > 1e150 else (1.0 if th >= 0 else -1.0) / (abs(th) + np.sqrt(1.0 + th * th))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = t * c
                    any_rot = True
                P.append(p); Q.append(q); Cs.append(c); Ss.append(s)
            P, Q, Cs, Ss = np.array(P), np.array(Q), np.array(Cs), np.array(Ss)
            if not any(Ss != 0.0):
                continue
            S = A + np.tril(A, -1).T                      # the symmetric matrix the lower triangle stands for
            app, aqq, apq = S[P, P].copy(), S[Q, Q].copy(), S[Q, P].copy()
            X = S.copy()
            Xp, Xq = X[:, P].copy(), X[:, Q].copy()
            X[:, P] = Cs * Xp - Ss * Xq
            X[:, Q] = Ss * Xp + Cs * Xq
            Yp, Yq = X[P, :].copy(), X[Q, :].copy()
            X[P, :] = Cs[:, None] * Yp - Ss[:, None] * Yq
            X[Q, :] = Ss[:, None] * Yp + Cs[:, None] * Yq
            rot = Ss != 0.0
            tt = np.where(rot, Ss / np.where(rot, Cs, 1.0), 0.0)
            X[P[rot], P[rot]] = (app - tt * apq)[rot]
            X[Q[rot], Q[rot]] = (aqq + tt * apq)[rot]
            X[Q[rot], P[rot]] = 0.0
            X[P[rot], Q[rot]] = 0.0
            A = np.tril(X)
            Vp, Vq = Vt[P, :].copy(), Vt[Q, :].copy()
            Vt[P, :] = Cs[:, None] * Vp - Ss[:, None] * Vq
            Vt[Q, :] = Ss[:, None] * Vp + Cs[:, None] * Vq
        if not any_rot:
            break
    return np.diag(A).copy(), Vt


def tail(Hin, bin_, frame):
    """k_marg_tail: (prior dict, live-row count); see tail_full."""
    m, nl, _, _ = tail_full(Hin, bin_, frame)
    return m, nl


def tail_full(Hin, bin_, frame):
    """tail() and, besides, the live rows (indices into the 156) and the live block's eigenvalues as the Jacobi sweeps leave them.
    k_marg_tail on a 171 x 171 H_marg / 171 b_marg: the prior dict (H, b, err, jt_inv) and the live-row count.  A non-finite input
    gives the reference's outcome for it (H 0, the rest NaN) and live = 0."""
    Hin, bin_ = np.asarray(Hin, dtype=np.float64), np.asarray(bin_, dtype=np.float64)
    if not (np.isfinite(Hin).all() and np.isfinite(bin_).all()):
        nan = np.full(PRD, np.nan)
        return {"H": np.zeros((PRD, PRD)), "b": nan.copy(), "err": nan.copy(), "jt_inv": np.full((PRD, PRD), np.nan)}, 0, np.zeros(0, dtype=int), np.zeros(0)
    o = marg_order(frame)
    Hp = Hin[np.ix_(o, o)]
    n2 = PRD
    Amm = 0.5 * (Hp[n2:, n2:] + Hp[n2:, n2:].T)
    ev16, V16t = jacobi(np.pad(Amm, ((0, 1), (0, 1))))
    inv = np.where(ev16 > EPS, 1.0 / np.where(ev16 > EPS, ev16, 1.0), 0.0)
    Ainv = (V16t.T * inv) @ V16t
    Ainv = Ainv[:M2, :M2]
    rowlive = [i for i in range(n2) if (Hin[o[i], :] != 0).any() or (Hp[n2:, i] != 0).any()]
    rowlive = np.array(rowlive, dtype=int)
    bp = bin_[o[:n2]].copy()
    tempB = Hp[np.ix_(rowlive, range(n2, PD))] @ Ainv
    bp[rowlive] = bin_[o[rowlive]] - tempB @ bin_[o[n2:]]
    Hpc = Hp[np.ix_(rowlive, rowlive)] - tempB @ Hp[np.ix_(range(n2, PD), rowlive)]
    alive = ((Hpc != 0).any(1) | (Hpc != 0).any(0)) if len(rowlive) else np.zeros(0, dtype=bool)
    lpos = np.nonzero(alive)[0]
    live = rowlive[lpos]
    nl = len(live)
    A = Hpc[np.ix_(lpos, lpos)]
    A = np.tril(A) + np.tril(A, -1).T                # the lower triangle, as Eigen and the device read it
    npad = nl + (nl & 1)
    ev, Vt = jacobi(np.pad(A, ((0, npad - nl), (0, npad - nl))))
    ev, Vt = ev[:nl], Vt[:nl, :nl]
    order = np.lexsort((np.arange(nl), ev))         # ascending, ties by index
    nz = n2 - nl
    H, Jt, err = np.zeros((n2, n2)), np.zeros((n2, n2)), np.zeros(n2)
    kept = [a for a in order if ev[a] > EPS]
    for rank, a in enumerate(order):
        if ev[a] > EPS:
            row = np.zeros(n2)
            row[live] = np.sqrt(1.0 / ev[a]) * Vt[a]
            Jt[nz + rank] = row
            err[nz + rank] = -math.fsum(row[live] * bp[live])      # (the device sums these compensated: close to exact rounding)
    if kept:
        K = np.array(kept)
        Hl = (Vt[K].T * ev[K]) @ Vt[K]
        Hl[np.abs(Hl) <= 1e-9] = 0.0
        H[np.ix_(live, live)] = Hl
    return {"H": H, "b": bp, "err": err, "jt_inv": Jt}, nl, live, ev


def marginalize(oracle_lib, vio, cfg, kind, w, prior):
    """build + tail: the restated device result, and the live-row count."""
    H, b = build(oracle_lib, vio, cfg, kind, w, prior)
    return tail(H, b, 0 if kind == vio.MARG_OLD else vio.WINDOW_SIZE - 1)


def dense_input(oracle_lib, ctx, kind):
    """The oracle's own H_marg / b_marg (vioo_marg_dense_input) of the window `ctx` (an oracle context) holds."""
    f = oracle_lib.dll.vioo_marg_dense_input
    f.restype = C.c_int
    H, b = np.zeros((PD, PD)), np.zeros(PD)
    assert f(ctx.h, C.c_int32(kind), _dp(H), _dp(b)) == 0
    return H, b


def exact_schur(Hin, bin_, frame, rows, digits=50):
    """Arr - Arm Amm^-1 Amr and brr - Arm Amm^-1 bmm on the given rows of the kept block, in `digits`-digit arithmetic (mpmath) from the
    fp64 input: what both fp64 tails approximate.  Amm^-1 is the eigen pseudo-inverse with the 1e-8 cut of problem.cc:750-756, also in
    `digits`-digit arithmetic."""
    import mpmath as mp
    with mp.workdps(digits):
        o = marg_order(frame)
        Hp = np.asarray(Hin)[np.ix_(o, o)]
        bo = np.asarray(bin_)[o]
        Amm = 0.5 * (Hp[PRD:, PRD:] + Hp[PRD:, PRD:].T)
        E, Q = mp.eigsy(mp.matrix(Amm.tolist()))
        Ai = Q * mp.diag([1 / e if e > EPS else 0 for e in E]) * Q.T
        Arm = mp.matrix(Hp[np.ix_(rows, range(PRD, PD))].tolist())
        Amr = mp.matrix(Hp[np.ix_(range(PRD, PD), rows)].tolist())
        T, tb = Arm * Ai * Amr, Arm * Ai * mp.matrix(bo[PRD:].tolist())
        n = len(rows)
        S = np.array([[float(mp.mpf(Hp[rows[i], rows[j]]) - T[i, j]) for j in range(n)] for i in range(n)])
        bs = np.array([float(mp.mpf(bo[rows[i]]) - tb[i]) for i in range(n)])
    return S, bs


# ---------------------------------------------------------------------------------------------------------
# well-conditioned windows and the tight bar (test_marg_reference.py on the CPU, test_gpu_marg_limits.py on the device)
# ---------------------------------------------------------------------------------------------------------
GRAVITY_OTHER = (0.3, -0.2, 9.6)
_MEMO = {}


def _memo(tag, fn, Hin, bin_, frame, *key):
    """fn() once per (input bits, frame, key): the references of a window are computed once and shared by the tests that need them."""
    k = (tag, np.asarray(Hin).tobytes(), np.asarray(bin_).tobytes(), int(frame)) + key
    if k not in _MEMO:
        _MEMO[k] = fn()
    return _MEMO[k]


def frame_of(kind):
    return 0 if kind == 0 else 9          # VIO_MARG_OLD: frame 0; VIO_MARG_SECOND_NEW: frame WINDOW_SIZE - 1


def soft_imu(w, seed, scale):
    """w with a well-conditioned IMU edge 0: its own preint[0] with the covariance replaced by (A A^T / 15 + I) * scale (A a 15 x 15
    normal draw), the speeds jittered by N(0, 0.05) and the biases by N(0, 0.02), so that the bias Jacobians and the linearized_*
    corrections carry weight.  cond(Amm) is then 7e2 .. 7e6 (scale 1e-4 .. 1) instead of the synthesised edge's 1e11."""
    rng = np.random.RandomState(seed)
    A = rng.normal(size=(15, 15))
    s = w.copy()
    p0 = dict(w.preint[0])
    p0["covariance"] = (A @ A.T / 15 + np.eye(15)) * scale
    s.preint = [p0] + list(w.preint[1:])
    s.speed_bias = np.array(w.speed_bias, dtype=np.float64)
    s.speed_bias[:, 0:3] += rng.normal(0.0, 0.05, size=(NF, 3))
    s.speed_bias[:, 3:9] += rng.normal(0.0, 0.02, size=(NF, 6))
    return s


def take(w, obs, landmarks=None):
    """w with the observations `obs` (mask or indices, in that order) and, when `landmarks` (ascending indices) is given, with those
    landmarks only, re-indexed."""
    s = w.copy()
    lm = np.asarray(w.lm)[obs]
    if landmarks is not None:
        new = -np.ones(len(w.inv_depth), dtype=np.int64)
        new[landmarks] = np.arange(len(landmarks))
        lm = new[lm]
        assert (lm >= 0).all()
        s.inv_depth = np.asarray(w.inv_depth)[landmarks]
    s.lm = lm.astype(np.int32)
    for k in ("host", "target", "pts_i", "pts_j"):
        setattr(s, k, np.asarray(getattr(w, k))[obs])
    s.n_landmarks, s.n_observations = len(s.inv_depth), len(s.lm)
    return s


def hosted0(n, seed):
    """n landmarks, every one hosted in frame 0, with ragged tracks: make_window(n, obs_per_landmark=10) with each landmark cut to
    its first k targets, k drawn from 1 .. 10."""
    w = load_package().synth.make_window(n, seed=seed, obs_per_landmark=10)
    assert (np.asarray(w.host) == 0).all()
    k = np.random.RandomState(seed).randint(1, 11, size=n)
    return take(w, np.asarray(w.target) <= k[np.asarray(w.lm)])


def live_set(H):
    return np.nonzero((np.asarray(H) != 0).any(1))[0]


def tight_check(m, Hin, bin_, frame, refs, factor=10.0, ceiling=None, name="", dead_rows_exact=True):
    """The prior m of the dense input (Hin, bin_) against the Schur complement (S, bs) in 50-digit arithmetic on m's live rows, which
    must be the restatement's: |H - S| <= bar_H, |b - bs| <= bar_b with bar_H = factor * max over refs of |ref H - S| + 1e-13 max|S|,
    bar_b the same with max(|bs|, 1).  refs: priors of the same input computed on the host (the restatement's tail, the oracle's),
    never the code under test.  The factor 10 and the floor are the rule of test_gpu_pnp.py and test_gpu_sfm.py: the device contracts
    products and sums in another order than either reference.  ceiling: an absolute cap on both bars, relative to max|S| and
    max(|bs|, 1).  dead_rows_exact=False is for the oracle's prior alone: its QL tail runs over all 156 rows and leaves entries of
    1.5e-9 (3e-16 of max|S|, just above the 1e-9 zeroing) in rows the restatement and the device drop as dead; those entries are then
    held to bar_H and the comparison is made on the restatement's live rows.  Prints and returns the distances and bars, absolute
    (dH, db, bar_H, bar_b) with their scales (Ss = max|S|, bsc = max(|bs|, 1))."""
    live = _memo("tail", lambda: tail_full(Hin, bin_, frame), Hin, bin_, frame)[2]
    if dead_rows_exact:
        assert np.array_equal(live_set(m["H"]), live), (name, len(live_set(m["H"])), len(live))
    assert all(np.isfinite(m[k]).all() for k in ("H", "b", "err", "jt_inv")), name
    if len(live) == 0:
        assert not m["H"].any()
        return dict(dH=0.0, db=0.0, bar_H=0.0, bar_b=0.0, Ss=1.0, bsc=1.0, live=0)
    S, bs = _memo("exact", lambda: exact_schur(Hin, bin_, frame, live), Hin, bin_, frame, tuple(live))
    Ss, bsc = np.abs(S).max(), max(np.abs(bs).max(), 1.0)
    lv = np.ix_(live, live)
    bar_H = factor * max(np.abs(r["H"][lv] - S).max() for r in refs) + 1e-13 * Ss
    bar_b = factor * max(np.abs(r["b"][live] - bs).max() for r in refs) + 1e-13 * bsc
    if ceiling is not None:
        bar_H, bar_b = min(bar_H, ceiling * Ss), min(bar_b, ceiling * bsc)
    dH, db = np.abs(m["H"][lv] - S).max(), np.abs(m["b"][live] - bs).max()
    if not dead_rows_exact:
        dead = np.ones(PRD, dtype=bool)
        dead[live] = False
        dH = max(dH, np.abs(m["H"][dead]).max(initial=0.0))
    print("tight_check %-28s live %3d max|S| %.2e  H %.2e (bar %.2e)  b %.2e (bar %.2e)" % (name, len(live), Ss, dH / Ss, bar_H / Ss,
                                                                                          db / bsc, bar_b / bsc))
    assert dH <= bar_H, (name, "H", dH / Ss, bar_H / Ss)
    assert db <= bar_b, (name, "b", db / bsc, bar_b / bsc)
    return dict(dH=dH, db=db, bar_H=bar_H, bar_b=bar_b, Ss=Ss, bsc=bsc, live=len(live))


def band_is_empty(ev):
    """No eigenvalue of the live block within a decade of the 1e-8 cut: |lambda| in [1e-9, 1e-7]."""
    a = np.abs(np.asarray(ev))
    return not ((a >= 1e-9) & (a <= 1e-7)).any()


def kept_rows(m):
    return int((np.asarray(m["jt_inv"]) != 0).any(1).sum())


def spectrum_check(m, Hin, bin_, frame, oracle_prior=None, name=""):
    """What jt_inv and err must satisfy whatever the 1e-8 cut does: err = -jt_inv b (in long double) and H P H = H with
    P = jt_inv^T jt_inv.  H = V L V^T and P = V L^-1 V^T over the kept eigenpairs, so H P H - H = V L (V^T V - I) (2 + ...) L V^T / L:
    of size |H|^2 |P| times V's loss of orthogonality, which for the Jacobi and QL solvers after ~10 sweeps over <= 156 rows is a few
    hundred eps at most; the bar is 1024 eps |H|^2 |P|.
    Where the restatement's live-block spectrum has no eigenvalue with |lambda| in [1e-9, 1e-7] (returns True then, and oracle_prior
    must be given), the kept count — the rows of jt_inv that are not all zero — must be the restatement's and P within
    10 |P_restatement - P_oracle| + 1e-13 max|P| of the restatement's."""
    r = m["err"].astype(np.longdouble) + m["jt_inv"].astype(np.longdouble) @ m["b"].astype(np.longdouble)
    assert float(np.abs(r).max()) <= 1e-9 * max(np.abs(m["err"]).max(), 1e-12), name
    P = m["jt_inv"].T @ m["jt_inv"]
    Hm = np.abs(m["H"]).max()
    assert np.abs(m["H"] @ P @ m["H"] - m["H"]).max() <= 1024 * np.finfo(float).eps * Hm * Hm * np.abs(P).max(), name
    rest, _, _, ev = _memo("tail", lambda: tail_full(Hin, bin_, frame), Hin, bin_, frame)
    if not band_is_empty(ev):
        return False
    assert kept_rows(m) == kept_rows(rest) == int((ev > EPS).sum()), (name, kept_rows(m), kept_rows(rest))
    Pr, Po = rest["jt_inv"].T @ rest["jt_inv"], oracle_prior["jt_inv"].T @ oracle_prior["jt_inv"]
    bar = 10.0 * np.abs(Pr - Po).max() + 1e-13 * np.abs(Pr).max()
    d = np.abs(P - Pr).max()
    print("spectrum_check %-25s kept %3d  |P - P_rest| %.2e (bar %.2e, max|P| %.2e)" % (name, kept_rows(m), d, bar, np.abs(Pr).max()))
    assert d <= bar, (name, d, bar)
    return True


def dense_spd_prior(scale=1.0, with_b=True):
    """The dense SPD prior of test_gpu_marg_batch.test_all_156_rows_live (every one of the 156 rows live), times `scale`."""
    rng = np.random.RandomState(3)
    A = rng.normal(size=(PRD, PRD))
    H = (A @ A.T + PRD * np.eye(PRD)) * scale
    b = rng.normal(size=PRD) if with_b else np.zeros(PRD)
    return dict(H=H, b=b, err=np.zeros(PRD), jt_inv=np.zeros((PRD, PRD)))


def frame9_only_prior():
    """A prior that is non-zero only inside frame 9's 15 x 15 block (and its b only there): MARG_SECOND_NEW leaves nothing live."""
    rng = np.random.RandomState(9)
    A = rng.normal(size=(M2, M2))
    H, b = np.zeros((PRD, PRD)), np.zeros(PRD)
    s = slice(6 + 15 * 9, 6 + 15 * 10)
    H[s, s] = A @ A.T + M2 * np.eye(M2)
    b[s] = rng.normal(size=M2)
    return dict(H=H, b=b, err=np.zeros(PRD), jt_inv=np.zeros((PRD, PRD)))


def outlier_window():
    """40 landmarks, every one hosted in frame 0 and seen in all 10 targets, 20 % outliers, no IMU edge 0: 66 live rows."""
    w = load_package().synth.make_window(40, seed=7, obs_per_landmark=10, outlier_fraction=0.2)
    w.preint = [None] + list(w.preint[1:])
    return w


def soft_window(scale):
    """outlier_window() with a soft IMU edge 0: 75 live rows."""
    w = load_package().synth.make_window(40, seed=7, obs_per_landmark=10, outlier_fraction=0.2)
    return soft_imu(w, 11, scale)


def nothing_live_window():
    """MARG_OLD without prior, IMU edge 0 or a landmark hosted in frame 0: H_marg = 0."""
    w = load_package().synth.make_window(60, seed=21)
    w.preint = [None] + list(w.preint[1:])
    e = np.asarray(w.host) != 0
    return take(w, e, np.unique(np.asarray(w.lm)[e]))


LIMIT_NAMES = ["noimu_trivial", "noimu_huber1_halfinfo", "noimu_huber10_halfinfo", "noimu_cauchy1", "noimu_tukey60", "soft_1e-4", "soft_1e-2",
               "soft_1", "soft_1e-4_gravity", "hosted0_1", "hosted0_255", "hosted0_256", "hosted0_257", "hosted0_513", "ragged300",
               "soft_dense_prior_147", "second_new_dense_prior"]
# the windows whose live-block spectrum (the restatement's) has no eigenvalue within a decade of the 1e-8 cut: spectrum_check compares the
# kept count and P there.  On the others a rounding-noise eigenvalue of the rank-deficient live block (the gauge directions: exactly 0)
# reaches 1e-9 in magnitude, max|S| being 1e6 or more.  (noimu_huber1_halfinfo has no live row: it is on the list and checks nothing.)  test_marg_reference.py asserts this list against the restatement.
SPECTRUM_CASES = ["noimu_huber1_halfinfo", "noimu_cauchy1", "soft_1e-4", "soft_1e-2", "soft_1", "soft_1e-4_gravity", "hosted0_1", "hosted0_257", "ragged300",
                  "soft_dense_prior_147", "second_new_dense_prior"]
# live rows: 6 (extrinsic) + 15 (frame 1 behind the IMU edge) + 6 per further target pose; 66 = 6 + 6 x 10 without the IMU edge; 147 = the
# dense prior's 141 kept rows + frame 10's pose (its speed-bias is touched by nothing), odd: the Jacobi solver pads it to 148
EXPECT_LIVE = {"hosted0_1": 33, "noimu_cauchy1": 66, "soft_1e-4": 75, "soft_dense_prior_147": 147, "second_new_dense_prior": 141,
               "noimu_huber1_halfinfo": 0}


def limit_case(name):
    """One of limit_cases(), made once."""
    if "cases" not in _MEMO:
        _MEMO["cases"] = limit_cases()
    kind, w, kw, amb = _MEMO["cases"][name]
    return kind, w.copy(), dict(kw), amb


def limit_cases():
    """name -> (kind, window, config overrides, drop Huber-ambiguous landmarks): the well-conditioned windows of the tight accuracy tests,
    without the second stage of ragged300 (whose prior is the first stage's result: second_stage())."""
    synth = load_package().synth
    half = 0.5 * (synth.FOCAL / 1.5)
    c = {
        "noimu_trivial": (0, outlier_window(), dict(loss_type=0), False),
        # (every landmark of this window has an edge beyond delta = 1 — 92 % of the edges are — so huber_ambiguous drops all 40 and the
        #  window is a third nothing-live system; with delta = 10, 15 landmarks stay, every edge of theirs inside delta)
        "noimu_huber1_halfinfo": (0, outlier_window(), dict(loss_type=1, loss_delta=1.0, reproj_sqrt_info=half), True),
        "noimu_huber10_halfinfo": (0, outlier_window(), dict(loss_type=1, loss_delta=10.0, reproj_sqrt_info=half), True),
        "noimu_cauchy1": (0, outlier_window(), {}, False),
        "noimu_tukey60": (0, outlier_window(), dict(loss_type=3, loss_delta=60.0), False),
        "soft_1e-4": (0, soft_window(1e-4), {}, False),
        "soft_1e-2": (0, soft_window(1e-2), {}, False),
        "soft_1": (0, soft_window(1.0), {}, False),
        "soft_1e-4_gravity": (0, soft_window(1e-4), dict(gravity=GRAVITY_OTHER), False),
    }
    for n in (1, 255, 256, 257, 513):
        c["hosted0_%d" % n] = (0, soft_imu(hosted0(n, 30 + n), 12, 1e-4), {}, False)
    c["ragged300"] = (0, soft_imu(synth.make_window(300, ragged=True), 13, 1e-4), {}, False)
    w = soft_window(1e-4)
    w.prior = dense_spd_prior(1e3)
    c["soft_dense_prior_147"] = (0, w, {}, False)
    w = synth.make_window(8, seed=3)
    w.prior = dense_spd_prior(1e3)
    c["second_new_dense_prior"] = (1, w, {}, False)
    return c


def second_stage(prior):
    """The second stage of ragged300: make_window(120, ragged=True, seed=10) with a soft IMU edge and `prior` (the first stage's)."""
    w = soft_imu(load_package().synth.make_window(120, ragged=True, seed=10), 14, 1e-4)
    w.prior = dict(prior)
    return w


def drop_huber_ambiguous(oracle_lib, w, kw):
    """w without the landmarks whose Huber weight test is decided by rounding (cov_reference.huber_ambiguous), as
    test_gpu_marg_batch.without_huber_ambiguous."""
    import cov_reference as cr
    c = oracle_lib.context(**kw)
    amb = cr.huber_ambiguous(oracle_lib, c.cfg, w, np.asarray(w.poses), np.asarray(w.ext), np.asarray(w.inv_depth))
    if not amb.any():
        return w
    return take(w, ~amb[np.asarray(w.lm)], np.nonzero(~amb)[0])


def references(oracle_lib, kind, w, kw):
    """(Hin, bin_, restatement's prior, oracle's prior) of one window: the oracle's dense input, the restatement's tail of it and the
    oracle's own prior (its QL tail), all on the host."""
    c = oracle_lib.context(**kw)
    c.load(w)
    Hin, bin_ = dense_input(oracle_lib, c, kind)
    orc = c.marginalize(kind, allow_nonfinite=True)
    rest = _memo("tail", lambda: tail_full(Hin, bin_, frame_of(kind)), Hin, bin_, frame_of(kind))[0]
    return Hin, bin_, rest, orc


# the packer's rules (vio_marg.h): the result depends on each landmark's own observation order alone, and on nothing outside the graph
def packer_window():
    """60 landmarks with hosts 0 .. 6 (4 observations each), a soft IMU edge: 9 landmarks hosted in frame 0, 3 in frame 3."""
    return soft_imu(load_package().synth.make_window(60, seed=21), 15, 1e-4)


def interleaved(w):
    """The observations reordered round-robin over the landmarks: the landmarks interleave, each keeps its own order."""
    lm = np.asarray(w.lm)
    first = np.concatenate([[0], np.cumsum(np.bincount(lm, minlength=len(w.inv_depth)))[:-1]])
    within = np.arange(len(lm)) - first[lm]
    assert (np.diff(lm) >= 0).all()                 # (landmark-major, as synth emits them)
    return take(w, np.argsort(within, kind="stable"))


def only_frame0(w):
    """Without every landmark that is not hosted in frame 0, re-indexed."""
    e = np.asarray(w.host) == 0
    return take(w, e, np.unique(np.asarray(w.lm)[e]))


def with_unobserved_landmark(w):
    s = w.copy()
    s.inv_depth = np.concatenate([np.asarray(w.inv_depth), [0.2]])
    s.n_landmarks = len(s.inv_depth)
    return s


def nan_outside_graph(w):
    """NaN in pts_j of an observation whose landmark is hosted in frame 3: not an edge of MargOldFrame's graph."""
    s = w.copy()
    s.pts_j = np.array(w.pts_j, dtype=np.float64)
    s.pts_j[np.nonzero(np.asarray(w.host) == 3)[0][1], 0] = np.nan
    return s


def tukey3_window():
    """outlier_window() under Tukey delta = 3: every edge of one frame-0 landmark lies beyond delta, rho' = 0 on all of them, h = 0."""
    return outlier_window(), dict(loss_type=3, loss_delta=3.0)


def quiet_window(n, seed):
    """A window at nearly the true state (no edge beyond a Tukey delta of 3): an ordinary neighbour under any loss."""
    return load_package().synth.make_window(n, seed=seed, pos_noise=1e-3, rot_noise=1e-4, depth_noise=0.01)
