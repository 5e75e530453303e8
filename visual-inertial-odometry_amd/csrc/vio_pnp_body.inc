// vio_pnp_body.inc — k_pnp_frames, its helpers, its constants and the three structs of its descriptor tables: the one text of the
// non-keyframes' PnP on the device.  vio_pnp.hip (libvio_pnp_hip) and vio_aif.hip (libvio_aif_hip) include it after
// <hip/hip_runtime.h>, include/vio_pnp.h and csrc/vio_sfm_math.h, with contraction off; the comment at the head of vio_pnp.hip
// describes the kernel (DESIGN.md sections 18 and 31).
constexpr int WAVE = 64;
constexpr int WAVES = 4;                // frames per workgroup
constexpr int NT = WAVE * WAVES;
constexpr int FO = 11;                  // per frame: status, iterations, n_used, cost, Q (4), T (3)
constexpr int PD = 5;                   // per usable point in the scratch: X (3), p (2), one array per component

struct PnpWin {
    int32_t np, has_valid;
    int64_t o_valid;    // staged int32: valid [np] as 0 / 1 (absent without has_valid)
    int64_t o_pts;      // staged doubles: points [np][3]
    int64_t o_key;      // staged doubles: key_Q [n_key][4] | key_T [n_key][3]
    int64_t o_keyT;
};

struct PnpFrame {
    int32_t win, guess;
    int32_t nobs, pad;
    int64_t o_op;       // staged int32: obs_point [nobs]
    int64_t o_obs;      // staged doubles: obs_pts [nobs][2]
    int64_t o_scr;      // double scratch: PD arrays of nobs
};

struct PnpArgs {
    const PnpWin *wins;
    const PnpFrame *frames;
    const int32_t *ints;
    const double *dd;
    double *scr;
    double *out;        // [frames][FO]
    int32_t nframes, min_points;
};

// the 28 sums over the wavefront's listed points at (R, t); without full, r^2 alone (v[27])
__device__ __forceinline__ void wave_sums(const double *pd, int cap, int n, int lane, const double *R, const double *t, bool full,
                                          double *v) {
#pragma unroll
    for (int e = 0; e < 28; ++e) v[e] = 0.0;
    for (int m = lane; m < n; m += WAVE) {
        const double X[3] = {pd[m], pd[cap + m], pd[2 * (int64_t)cap + m]}, p[2] = {pd[3 * (int64_t)cap + m], pd[4 * (int64_t)cap + m]};
        double r[2], Xc[3], RX[3];
        residual(R, t, X, p, r, Xc, RX);
        if (full) {
            double Jc[12], Jp[6];
            jac_cam(Xc, RX, Jc, Jp);
            int e = 0;
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int y = x; y < 6; ++y) { v[e] = v[e] + (Jc[x] * Jc[y] + Jc[6 + x] * Jc[6 + y]); ++e; }
#pragma unroll
            for (int x = 0; x < 6; ++x) v[21 + x] = v[21 + x] + (Jc[x] * r[0] + Jc[6 + x] * r[1]);
        }
        v[27] = v[27] + (r[0] * r[0] + r[1] * r[1]);
    }
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
        if (full) {
#pragma unroll
            for (int e = 0; e < 27; ++e) v[e] = v[e] + __shfl_xor(v[e], s, WAVE);
        }
        v[27] = v[27] + __shfl_xor(v[27], s, WAVE);
    }
}

__device__ __forceinline__ double grad_max(const double *v) {
    double gm = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) gm = fmax(gm, fabs(v[21 + k]));
    return gm;
}

__global__ __launch_bounds__(NT) void k_pnp_frames(PnpArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int f = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (f >= a.nframes) return;                     // (whole wavefronts: no barrier follows)
    const PnpFrame F = a.frames[f];
    const PnpWin W = a.wins[F.win];
    const int32_t *op = a.ints + F.o_op, *valid = a.ints + W.o_valid;
    const double *obs = a.dd + F.o_obs, *pts = a.dd + W.o_pts;
    const double *q = a.dd + W.o_key + 4 * (int64_t)F.guess, *T = a.dd + W.o_keyT + 3 * (int64_t)F.guess;
    double *pd = a.scr + F.o_scr, *o = a.out + (int64_t)FO * f;
    const int cap = F.nobs;

    // the usable points in the observations' order: a prefix count over 64 observations at a time
    int n = 0, bad = 0;
    for (int base = 0; base < cap; base += WAVE) {
        const int k = base + lane;
        bool use = false;
        double X0 = 0.0, X1 = 0.0, X2 = 0.0, p0 = 0.0, p1 = 0.0;
        if (k < cap) {
            const int j = op[k];
            p0 = obs[2 * k]; p1 = obs[2 * k + 1];
            bad |= !isfinite(p0) || !isfinite(p1);
            use = !W.has_valid || valid[j] != 0;
            if (use) {
                X0 = pts[3 * (int64_t)j]; X1 = pts[3 * (int64_t)j + 1]; X2 = pts[3 * (int64_t)j + 2];
                bad |= !isfinite(X0) || !isfinite(X1) || !isfinite(X2);
            }
        }
        const unsigned long long mask = __ballot(use);
        if (use) {
            const int m = n + __popcll(mask & ((1ull << lane) - 1ull));        // m < cap: at most one per observation
            pd[m] = X0; pd[cap + m] = X1; pd[2 * (int64_t)cap + m] = X2; pd[3 * (int64_t)cap + m] = p0; pd[4 * (int64_t)cap + m] = p1;
        }
        n += __popcll(mask);
    }
    for (int k = 0; k < 4; ++k) bad |= !isfinite(q[k]);
    for (int k = 0; k < 3; ++k) bad |= !isfinite(T[k]);
    bad = __any(bad);
    __threadfence_block();                          // the list is read by other lanes of this wavefront than wrote it

    int status = VIO_OK, it = 0;
    double R[9], t[3], cost = NAN;
    if (bad) status = VIO_ERR_NOT_FINITE;
    else if (n < a.min_points) status = VIO_PNP_FAIL_FEW_POINTS;
    else {
        // R = Q[g]^-1, t = -R T[g]
        double Rq[9];
        quat_to_rot(q, Rq);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[3 * r + c] = Rq[3 * c + r];
        for (int k = 0; k < 3; ++k) t[k] = -((R[3 * k] * T[0] + R[3 * k + 1] * T[1]) + R[3 * k + 2] * T[2]);
        double v[28];
        wave_sums(pd, cap, n, lane, R, t, true, v);
        cost = 0.5 * v[27];
        double radius = VIO_SFM_LM_INITIAL_RADIUS, vv = 2.0;
        bool go = true;
        if (!isfinite(cost)) { status = VIO_PNP_FAIL_NO_POSE; go = false; }
        else if (grad_max(v) <= VIO_SFM_BA_GRADIENT_TOL) go = false;
        while (go && it < VIO_SFM_PNP_MAX_ITER) {
            it += 1;
            const double lam = 1.0 / radius;
            double A[36], g[6], D[6], d[6];
            {
                int e = 0;
#pragma unroll
                for (int x = 0; x < 6; ++x)
#pragma unroll
                    for (int y = x; y < 6; ++y) { A[6 * x + y] = v[e]; A[6 * y + x] = v[e]; ++e; }
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                g[k] = -v[21 + k];
                D[k] = fmin(fmax(A[7 * k], LM_DIAG_MIN), LM_DIAG_MAX);
                A[7 * k] = A[7 * k] + lam * D[k];
            }
            bool take = false;
            double rho = -1.0, R2[9], t2[3];
            if (cholesky_solve6(A, g, d)) {
                double d2 = 0.0;
                for (int k = 0; k < 6; ++k) d2 += d[k] * d[k];
                if (sqrt(d2) <= VIO_SFM_PNP_STEP_TOL) break;
                double E[9];
                exp_so3(d, E);
                mm3(E, R, R2);
                for (int k = 0; k < 3; ++k) t2[k] = t[k] + d[3 + k];
                double ddd = 0.0, gd = 0.0;
                for (int k = 0; k < 6; ++k) { ddd += (d[k] * D[k]) * d[k]; gd += d[k] * v[21 + k]; }
                const double model = 0.5 * (lam * ddd - gd);
                double v2[28];
                wave_sums(pd, cap, n, lane, R2, t2, false, v2);
                const double cost2 = 0.5 * v2[27];
                rho = (isfinite(cost2) && model > 0) ? (cost - cost2) / model : -1.0;
                take = rho > LM_MIN_RHO;
            }
            if (take) {
                for (int k = 0; k < 9; ++k) R[k] = R2[k];
                for (int k = 0; k < 3; ++k) t[k] = t2[k];
                wave_sums(pd, cap, n, lane, R, t, true, v);
                cost = 0.5 * v[27];
                if (grad_max(v) <= VIO_SFM_BA_GRADIENT_TOL) break;
                radius = lm_radius(radius, rho);
                vv = 2.0;
            } else {
                radius = radius / vv;
                vv = vv * 2.0;
                if (radius < LM_RADIUS_MIN) break;
            }
        }
    }
    // Q = Quaternion(R^T), T = -R^T t
    double Qo[4] = {NAN, NAN, NAN, NAN}, To[3] = {NAN, NAN, NAN};
    if (status == VIO_OK) {
        double Rt[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Rt[3 * r + c] = R[3 * c + r];
        rot_to_quat(Rt, Qo);
        for (int k = 0; k < 3; ++k) To[k] = -((Rt[3 * k] * t[0] + Rt[3 * k + 1] * t[1]) + Rt[3 * k + 2] * t[2]);
        int fin = isfinite(cost) != 0;
        for (int k = 0; k < 4; ++k) fin &= isfinite(Qo[k]) != 0;
        for (int k = 0; k < 3; ++k) fin &= isfinite(To[k]) != 0;
        if (!fin) status = VIO_ERR_NOT_FINITE;
    }
    if (lane == 0) {
        const bool ok = status == VIO_OK;
        o[0] = status; o[1] = it; o[2] = n; o[3] = ok ? cost : NAN;
        for (int k = 0; k < 4; ++k) o[4 + k] = ok ? Qo[k] : NAN;
        for (int k = 0; k < 3; ++k) o[8 + k] = ok ? To[k] : NAN;
    }
}
