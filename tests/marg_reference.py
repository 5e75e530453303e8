"""numpy restatement of the batched marginalisation's device algorithm (include/vio_marg.h, csrc/vio_marg.hip).

build(): k_marg_build — H_marg / b_marg of Problem::Marginalize's graph (problem.cc:617-713) from the oracle's edge pieces (vioo_reproj_edge,
vioo_robust_info2, vioo_imu_edge, vioo_inverse15), landmark by landmark in ascending order.
tail(): k_marg_tail — problem.cc:717-779 with the same parallel cyclic Jacobi eigen-solver (round-robin schedule, rotation test, stopping
rule), the same live-row rules and the same output layout.
Shared by test_marg_reference.py (CPU, against the oracle) and test_gpu_marg_batch.py (the device against this restatement)."""
import ctypes as C
import math

import numpy as np

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
    """k_marg_tail on a 171 x 171 H_marg / 171 b_marg: the prior dict (H, b, err, jt_inv) and the live-row count.  A non-finite input
    gives the reference's outcome for it (H 0, the rest NaN) and live = 0."""
    Hin, bin_ = np.asarray(Hin, dtype=np.float64), np.asarray(bin_, dtype=np.float64)
    if not (np.isfinite(Hin).all() and np.isfinite(bin_).all()):
        nan = np.full(PRD, np.nan)
        return {"H": np.zeros((PRD, PRD)), "b": nan.copy(), "err": nan.copy(), "jt_inv": np.full((PRD, PRD), np.nan)}, 0
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
    return {"H": H, "b": bp, "err": err, "jt_inv": Jt}, nl


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
