// Body of k_cov_landmarks<D> and k_cov_landmarks_batch<D> (vio_covariance.hip), included inside both kernels.  In scope: D, a
// (the window's CovLmArgs), blk (the workgroup's index within the window).  A fragment for the reason vio_cov_pose_body.inc gives.
    constexpr int NT = LmNT<D>::v;
    __shared__ double sc[CD * CD];
    __shared__ double wl[CD * D * NT];          // the lane's coupling column, variable-major: [(72 * d + var) * NT + lane]
    __shared__ double sR[(NF + 1) * 9];         // rotations of the 11 poses and (slot 11) of the extrinsic
    const int tid = threadIdx.x;
    for (int q = tid; q < CD * CD; q += NT) sc[q] = a.cc[q];
    for (int f = tid; f <= NF; f += NT) d_quat_to_R(f < NF ? a.poses + 7 * f + 3 : a.ext + 3, sR + 9 * f);
    for (int q = 0; q < CD * D; ++q) wl[q * NT + tid] = 0.0;
    __syncthreads();
    const int l = blk * NT + tid;
    if (l >= a.n) return;

    const double *ric = sR + 9 * NF, *tic = a.ext;
    double ricT[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) ricT[3 * r + c] = ric[3 * c + r];
    const double s = a.sqrt_info;
    double h[D * D];
#pragma unroll
    for (int q = 0; q < D * D; ++q) h[q] = 0.0;
    unsigned mask = 0;                          // camera blocks the landmark couples to: bit 0 ext, bit 1 + f pose f
    double *w = wl + tid;

    for (int e = a.off[l]; e < a.off[l + 1]; ++e) {
        const int fj = a.ofr[e];
        const double *Rj = sR + 9 * fj, *Pj = a.poses + 7 * fj;
        double r[2], W[4];
        if (D == 1) {
            // EdgeReprojection (edge_reprojection.cc:18-109)
            const int fi = a.ohost[l];
            const double *Ri = sR + 9 * fi, *Pi = a.poses + 7 * fi;
            const double lam = a.val[l];
            const double pts_i[3] = {a.pts_i[2 * l], a.pts_i[2 * l + 1], 1.0};
            const double pc_i[3] = {pts_i[0] / lam, pts_i[1] / lam, pts_i[2] / lam};
            double pb_i[3], pw[3], dd[3], pb_j[3], ee[3], pc_j[3];
            d_m3_vec(ric, pc_i, pb_i);
            for (int k = 0; k < 3; ++k) pb_i[k] += tic[k];
            d_m3_vec(Ri, pb_i, pw);
            for (int k = 0; k < 3; ++k) dd[k] = pw[k] + Pi[k] - Pj[k];
            d_m3_tvec(Rj, dd, pb_j);
            for (int k = 0; k < 3; ++k) ee[k] = pb_j[k] - tic[k];
            d_m3_tvec(ric, ee, pc_j);
            const double dep = pc_j[2];
            r[0] = pc_j[0] / dep - a.pts_j[2 * e];
            r[1] = pc_j[1] / dep - a.pts_j[2 * e + 1];
            d_robust_info2(a.loss_type, a.loss_delta, s, r, W);
            const double red[6] = {1. / dep, 0, -pc_j[0] / (dep * dep), 0, 1. / dep, -pc_j[1] / (dep * dep)};
            double A[9], ARi[9], T[9], M[9], Ji[12], Jj[12], Je[12];
            double RjT[9];
#pragma unroll
            for (int r2 = 0; r2 < 3; ++r2)
#pragma unroll
                for (int c = 0; c < 3; ++c) RjT[3 * r2 + c] = Rj[3 * c + r2];
            d_m3_mul(ricT, RjT, A);                                  // ric^T Rj^T
            d_m3_mul(A, Ri, ARi);                                    // ric^T Rj^T Ri
            d_m3_mul(ARi, ric, T);                                   // ric^T Rj^T Ri ric
            double v[3];
            d_m3_vec(T, pts_i, v);
            double Jl[2];
            for (int r2 = 0; r2 < 2; ++r2)
                Jl[r2] = (red[3 * r2] * v[0] + red[3 * r2 + 1] * v[1] + red[3 * r2 + 2] * v[2]) * -1.0 / (lam * lam);
            // J_pose_i = reduce [ric^T Rj^T | -ric^T Rj^T Ri hat(pb_i)]
            d_reduce_mul<6>(red, A, Ji, 0);
            d_skew(pb_i, M);
            double Mm[9];
            d_m3_mul(ARi, M, Mm);
            for (int k = 0; k < 9; ++k) Mm[k] = -Mm[k];
            d_reduce_mul<6>(red, Mm, Ji, 3);
            // J_pose_j = reduce [-ric^T Rj^T | ric^T hat(pb_j)]
            for (int k = 0; k < 9; ++k) M[k] = -A[k];
            d_reduce_mul<6>(red, M, Jj, 0);
            d_skew(pb_j, M);
            d_m3_mul(ricT, M, Mm);
            d_reduce_mul<6>(red, Mm, Jj, 3);
            // J_ext = reduce [ric^T (Rj^T Ri - I) | -T hat(pc_i) + hat(T pc_i) + hat(ric^T (Rj^T (Ri tic + Pi - Pj) - tic))]
            if (a.ext_free) {
                d_m3_mul(RjT, Ri, M);
                M[0] -= 1; M[4] -= 1; M[8] -= 1;
                d_m3_mul(ricT, M, Mm);
                d_reduce_mul<6>(red, Mm, Je, 0);
                double S1[9], t1[9], v2[3], S2[9], u[3], ww[3], x[3], S3[9];
                d_skew(pc_i, S1);
                d_m3_mul(T, S1, t1);
                d_m3_vec(T, pc_i, v2);
                d_skew(v2, S2);
                d_m3_vec(Ri, tic, u);
                for (int k = 0; k < 3; ++k) u[k] = u[k] + Pi[k] - Pj[k];
                d_m3_tvec(Rj, u, ww);
                for (int k = 0; k < 3; ++k) ww[k] -= tic[k];
                d_m3_tvec(ric, ww, x);
                d_skew(x, S3);
                for (int k = 0; k < 9; ++k) M[k] = -t1[k] + S2[k] + S3[k];
                d_reduce_mul<6>(red, M, Je, 3);
            }
            // h_l += J_l^T W J_l;  w_l += (J_l^T W) [J_i | J_j | J_ext] on the host / target / extrinsic blocks
            const double t0 = Jl[0] * W[0] + Jl[1] * W[2], t1 = Jl[0] * W[1] + Jl[1] * W[3];
            h[0] += t0 * Jl[0] + t1 * Jl[1];
            const int ii = 6 + 6 * fi, jj = 6 + 6 * fj;
            for (int k = 0; k < 6; ++k) {
                w[(ii + k) * NT] += t0 * Ji[k] + t1 * Ji[6 + k];
                w[(jj + k) * NT] += t0 * Jj[k] + t1 * Jj[6 + k];
                if (a.ext_free) w[k * NT] += t0 * Je[k] + t1 * Je[6 + k];
            }
            mask |= (2u << fi) | (2u << fj) | (a.ext_free ? 1u : 0u);
        } else {
            // EdgeReprojectionXYZ (edge_reprojection.cc:130-180)
            const double *pw = a.val + 3 * l;
            double dd[3], pim[3], ee[3], pc[3];
            for (int k = 0; k < 3; ++k) dd[k] = pw[k] - Pj[k];
            d_m3_tvec(Rj, dd, pim);                                  // Rj^T (pw - Pj): pts_imu in the observing frame
            for (int k = 0; k < 3; ++k) ee[k] = pim[k] - tic[k];
            d_m3_tvec(ric, ee, pc);
            const double dep = pc[2];
            r[0] = pc[0] / dep - a.pts_j[2 * e];
            r[1] = pc[1] / dep - a.pts_j[2 * e + 1];
            d_robust_info2(a.loss_type, a.loss_delta, s, r, W);
            const double red[6] = {1. / dep, 0, -pc[0] / (dep * dep), 0, 1. / dep, -pc[1] / (dep * dep)};
            double RT[9], M[9], Mm[9], Jp[12], Jf[6];
#pragma unroll
            for (int r2 = 0; r2 < 3; ++r2)
#pragma unroll
                for (int c = 0; c < 3; ++c) RT[3 * r2 + c] = Rj[3 * c + r2];
            // J_pose = reduce [ric^T (-Ri^T) | ric^T hat(pts_imu)],  J_feature = reduce ric^T Ri^T
            d_m3_mul(ricT, RT, Mm);
            for (int k = 0; k < 9; ++k) M[k] = -Mm[k];
            d_reduce_mul<6>(red, M, Jp, 0);
            d_skew(pim, M);
            double Mh[9];
            d_m3_mul(ricT, M, Mh);
            d_reduce_mul<6>(red, Mh, Jp, 3);
            for (int r2 = 0; r2 < 2; ++r2)
                for (int c = 0; c < 3; ++c)
                    Jf[3 * r2 + c] = red[3 * r2] * Mm[c] + red[3 * r2 + 1] * Mm[3 + c] + red[3 * r2 + 2] * Mm[6 + c];
            const int ip = 6 + 6 * fj;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double t0 = Jf[d] * W[0] + Jf[3 + d] * W[2], t1 = Jf[d] * W[1] + Jf[3 + d] * W[3];     // (J_f^T W) row d
#pragma unroll
                for (int c = 0; c < 3; ++c) h[3 * d + c] += t0 * Jf[c] + t1 * Jf[3 + c];
                for (int k = 0; k < 6; ++k) w[(CD * d + ip + k) * NT] += t0 * Jp[k] + t1 * Jp[6 + k];
            }
            mask |= 2u << fj;
        }
    }

    // q = w^T Sigma_cc w over the blocks the landmark touches (D x D), block rows P, block columns Q in ascending order
    double q[D * D];
#pragma unroll
    for (int k = 0; k < D * D; ++k) q[k] = 0.0;
    for (unsigned mp = mask; mp; mp &= mp - 1) {
        const int P = __builtin_ctz(mp);
        double t[6 * D];                                               // (Sigma_cc w)_P
#pragma unroll
        for (int k = 0; k < 6 * D; ++k) t[k] = 0.0;
        for (unsigned mq = mask; mq; mq &= mq - 1) {
            const int Q = __builtin_ctz(mq);
            for (int c = 0; c < 6; ++c) {
                double wq[D];
#pragma unroll
                for (int d = 0; d < D; ++d) wq[d] = w[(CD * d + 6 * Q + c) * NT];
#pragma unroll
                for (int r2 = 0; r2 < 6; ++r2) {
                    const double sv = sc[(6 * P + r2) * CD + 6 * Q + c];
#pragma unroll
                    for (int d = 0; d < D; ++d) t[D * r2 + d] += sv * wq[d];
                }
            }
        }
#pragma unroll
        for (int r2 = 0; r2 < 6; ++r2) {
            double wp[D];
#pragma unroll
            for (int d = 0; d < D; ++d) wp[d] = w[(CD * d + 6 * P + r2) * NT];
#pragma unroll
            for (int d = 0; d < D; ++d)
#pragma unroll
                for (int d2 = 0; d2 < D; ++d2) q[D * d + d2] += wp[d] * t[D * r2 + d2];
        }
    }

    if (D == 1) {
        const double hl = h[0];
        a.info[l] = hl;
        if (!(hl > 0.0) || !isfinite(hl)) { atomicMin(a.bad, l); a.out[l] = NAN; return; }
        const double hinv = 1.0 / hl;
        a.out[l] = hinv + q[0] * hinv * hinv;
    } else {
        // H_ll^-1 by the adjugate; positive definite by Sylvester's criterion (the leading minors), else reported
        const double *H = h;
        const double m0 = H[0], m1 = H[0] * H[4] - H[1] * H[3];
        const double c00 = H[4] * H[8] - H[5] * H[7], c01 = H[2] * H[7] - H[1] * H[8], c02 = H[1] * H[5] - H[2] * H[4];
        const double c11 = H[0] * H[8] - H[2] * H[6], c12 = H[2] * H[3] - H[0] * H[5], c22 = H[0] * H[4] - H[1] * H[3];
        const double det = H[0] * c00 + H[1] * (H[5] * H[6] - H[3] * H[8]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
#pragma unroll
        for (int k = 0; k < 9; ++k) a.info[9 * l + k] = H[k];
        if (!(m0 > 0.0) || !(m1 > 0.0) || !(det > 0.0) || !isfinite(det)) {
            atomicMin(a.bad, l);
#pragma unroll
            for (int k = 0; k < 9; ++k) a.out[9 * l + k] = NAN;
            return;
        }
        const double id = 1.0 / det;
        const double Hi[9] = {c00 * id, c01 * id, c02 * id, c01 * id, c11 * id, c12 * id, c02 * id, c12 * id, c22 * id};
        double T[9], O[9];
        d_m3_mul(Hi, q, T);
        d_m3_mul(T, Hi, O);
#pragma unroll
        for (int k = 0; k < 9; ++k) a.out[9 * l + k] = Hi[k] + O[k];
    }
