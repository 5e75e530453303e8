// vio_marg.hip — libvio_marg_hip.so: Problem::Marginalize for many windows in one call (include/vio_marg.h).
//
//   k_marg_build  one workgroup per window: H_marg (171 x 171) and b_marg of the marginalisation graph (problem.cc:617-713)
//                 phase 1  thread per landmark hosted in frame 0: its edges' residuals, Jacobians and robust weights
//                          (d_robust_info2, k_cov_landmarks's), h_l, b_l and the coupling row w_l; the IMU edge 0 -> 1 in LDS
//                          (d_imu_jac_block and d_imu_residual, the solver's)
//                 phase 2  thread per entry of the lower triangle: the landmark sums in landmark order, then the IMU block and
//                          the old prior; mirrored into the upper triangle
//   k_marg_tail   one workgroup per window: the dense tail of problem.cc:717-779 — the 15 marginalised rows moved to the end,
//                 the eigen pseudo-inverse of Amm, the Schur complement, the live rows, the eigen-decomposition of the live block
//                 by a parallel cyclic Jacobi solver (packed lower triangle in LDS, eigenvectors in HBM scratch), Jt_inv, err and
//                 H = J^T J
// No atomics: every sum has a fixed order, so repeated calls are bitwise identical and a window's result does not depend on its
// batch.  The library calls no function of libvio_hip; it includes its device code (vio_device_math.h: rotations, 3 x 3 products,
// loss and robust weight; vio_imu_math.h: the IMU edge) and compiles host_dense.cpp's inverse15 a second time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vio_marg.h"
#include "host_dense.h"
#include "vio_companion.h"
#include "vio_device_math.h"
#include "vio_types.h"

namespace {

constexpr int PD = VIO_POSE_DIM;         // 171
constexpr int PRD = VIO_PRIOR_DIM;       // 156
constexpr int NF = VIO_NUM_FRAMES;       // 11
constexpr int M2 = 15;                   // marginalised variables: pose (6) + speed-bias (9) of one frame
constexpr int BUILD_NT = 256;
constexpr int TAIL_NT = 512;
constexpr int EREC = 90;                 // per edge: J (2 x 18), W J (2 x 18), -drho J^T Info r (18); columns ext | pose 0 | target
constexpr int LREC = 75;                 // per landmark: w (72), 1 / h, b_l, h
constexpr size_t OUT_STRIDE = (size_t)2 * PRD * PRD + 2 * PRD + 2;      // H, jt_inv, b, err, status, live rows
constexpr int TRI_MAX = PRD * (PRD + 1) / 2;

// One window of the batch as the kernels see it: offsets (in doubles / ints) into the uploaded arrays and the scratch.
struct MargWin {
    int32_t kind, has_imu, has_prior, nl, ne, frame;
    int64_t o_state;         // ext (7) | poses (77) | speed-bias (99)
    int64_t o_pre;           // PRE_STRIDE: the packed pre-integration of interval 0, information included
    int64_t o_hp, o_bp;      // 156 x 156, 156
    int64_t o_invd, o_ptsi;  // nl, nl x 2: the graph's landmarks in ascending order
    int64_t o_ptsj;          // ne x 2
    int64_t i_eoff, i_tgt;   // nl + 1 edge offsets, ne targets (ints)
    int64_t s_edge, s_lm, s_H, s_hpc, s_vt;     // scratch
};
constexpr int STATE_D = 7 + 77 + 99;
constexpr int CD_W = VIO_CAM_DIM;      // 72

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------------------
#include "vio_imu_math.h"       // (here, not with the other headers: its no-contraction region ends where the code below begins)

namespace {
__device__ __forceinline__ int imu_vblock(int a) { return a < 6 ? 0 : (a < 15 ? 1 : (a < 21 ? 2 : 3)); }

// camera index (0 .. 71: ext, then 6 per pose) of a pose-ordering index, or -1 for a speed-bias variable
__device__ __forceinline__ int mg_cam(int i) {
    if (i < 6) return i;
    const int f = (i - 6) / 15, o = (i - 6) - 15 * f;
    return o < 6 ? 6 + 6 * f + o : -1;
}
// column of camera variable ci in an edge record (ext 0..5, host = pose 0 6..11, target pose 12..17), or -1 when the edge has none
__device__ __forceinline__ int mg_col(int ci, int tgt) {
    if (ci < 12) return ci;
    const int f = (ci - 6) / 6;
    return f == tgt ? 12 + (ci - 6 - 6 * f) : -1;
}

struct MargCfg {
    int32_t loss_type;
    double loss_delta, sqrt_info;
    double gravity[3];
};

// ---------------------------------------------------------------------------------------------------------
// k_marg_build
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BUILD_NT) k_marg_build(const MargWin *__restrict__ wins, const int32_t *__restrict__ ints,
                                                         const double *__restrict__ dbl, double *__restrict__ scr, MargCfg cfg) {
    const MargWin W = wins[blockIdx.x];
    const int tid = threadIdx.x;
    double *Hm = scr + W.s_H, *bm = Hm + (size_t)PD * PD;
    const bool old = W.kind == VIO_MARG_OLD;
    const double *hp = W.has_prior ? dbl + W.o_hp : nullptr, *bp = W.has_prior ? dbl + W.o_bp : nullptr;
    __shared__ double sR[(NF + 1) * 9];
    __shared__ double sJ[450], sI[225], sJtI[450], sr[16], sIr[16], sT[900], sG[30];
    const double *st = dbl + W.o_state;
    const double *ext = st, *poses = st + 7, *sb = st + 7 + 77;
    const bool imu = old && W.has_imu;

    if (old) {
        for (int f = tid; f <= NF; f += BUILD_NT) d_quat_to_R(f < NF ? poses + 7 * f + 3 : ext + 3, sR + 9 * f);
        if (imu) {
            const double *pre = dbl + W.o_pre;
            for (int e = tid; e < 450; e += BUILD_NT) sJ[e] = 0.0;
            for (int e = tid; e < 225; e += BUILD_NT) sI[e] = pre[PRE_INFO + e];
        }
        __syncthreads();
        // IMU edge 0 -> 1: T = J^T Info J, G = J^T Info r (the d_imu_item of vio_kernels.hip)
        if (imu) {
            const double *pre = dbl + W.o_pre;
            const double *pi = poses, *pj = poses + 7, *si = sb, *sj = sb + 9;
            if (tid < 16) {
                ImuCommon c;
                double RiT[9];
                d_imu_common(pre, pi, si, pj, c);
                d_imu_rit(c, RiT);
                if (tid < 14) d_imu_jac_block(tid, pre, cfg.gravity, pi, si, pj, sj, c, RiT, sJ);
                else if (tid == 14) {
                    double r[15];
                    d_imu_residual(pre, cfg.gravity, pi, si, pj, sj, c, r);
                    for (int i = 0; i < 15; ++i) sr[i] = r[i];
                } else {
                    for (int i = 0; i < 3; ++i) {
                        sJ[30 * (O_BA + i) + 6 + 3 + i] = -1.0; sJ[30 * (O_BG + i) + 6 + 6 + i] = -1.0;
                        sJ[30 * (O_BA + i) + 21 + 3 + i] = 1.0; sJ[30 * (O_BG + i) + 21 + 6 + i] = 1.0;
                    }
                }
            }
            __syncthreads();
            for (int e = tid; e < 450; e += BUILD_NT) {
                const int a = e / 15, j = e % 15;
                double s = 0;
                for (int i = 0; i < 15; ++i) s = fma(sJ[30 * i + a], sI[15 * i + j], s);
                sJtI[e] = s;
            }
            if (tid < 15) {
                double s = 0;
                for (int j = 0; j < 15; ++j) s = fma(sI[15 * tid + j], sr[j], s);
                sIr[tid] = s;
            }
            __syncthreads();
            for (int e = tid; e < 900; e += BUILD_NT) {
                const int a = e / 30, b = e % 30;
                double s = 0;
                for (int j = 0; j < 15; ++j) s = fma(sJtI[15 * a + j], sJ[30 * j + b], s);
                sT[e] = s;
            }
            if (tid < 30) {
                double s = 0;
                for (int i = 0; i < 15; ++i) s = fma(sJ[30 * i + tid], sIr[i], s);
                sG[tid] = s;
            }
        }

        // phase 1: thread per landmark; EdgeReprojection (edge_reprojection.cc:18-109) with the host in frame 0.  The statements are
        // those of vio_cov_landmarks_body.inc, the blocks laid into one 2 x 18 record.  (Both kernels calling one inlined function
        // was tried: the compiler then contracted fewer products in this kernel, DESIGN.md section 14, so each keeps its own text.)
        const int32_t *eoff = ints + W.i_eoff, *tgt = ints + W.i_tgt;
        const double *invd = dbl + W.o_invd, *ptsi = dbl + W.o_ptsi, *ptsj = dbl + W.o_ptsj;
        const double *ric = sR + 9 * NF, *tic = ext;
        const double s = cfg.sqrt_info, info = s * s;
        for (int l = tid; l < W.nl; l += BUILD_NT) {
            double *lr = scr + W.s_lm + (size_t)l * LREC;
            for (int k = 0; k < CD_W; ++k) lr[k] = 0.0;
            double h = 0.0, bl = 0.0;
            const double lam = invd[l];
            const double pts_i[3] = {ptsi[2 * l], ptsi[2 * l + 1], 1.0};
            const double *Ri = sR, *Pi = poses;
            for (int e = eoff[l]; e < eoff[l + 1]; ++e) {
                const int fj = tgt[e];
                const double *Rj = sR + 9 * fj, *Pj = poses + 7 * fj;
                double ricT[9], RjT[9];
                for (int r2 = 0; r2 < 3; ++r2)
                    for (int c = 0; c < 3; ++c) { ricT[3 * r2 + c] = ric[3 * c + r2]; RjT[3 * r2 + c] = Rj[3 * c + r2]; }
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
                double r[2], Wm[4];
                r[0] = pc_j[0] / dep - ptsj[2 * e];
                r[1] = pc_j[1] / dep - ptsj[2 * e + 1];
                const double drho = d_robust_info2(cfg.loss_type, cfg.loss_delta, s, r, Wm);
                const double red[6] = {1. / dep, 0, -pc_j[0] / (dep * dep), 0, 1. / dep, -pc_j[1] / (dep * dep)};
                double A[9], ARi[9], T[9], M[9], Mm[9], J[36];
                d_m3_mul(ricT, RjT, A);
                d_m3_mul(A, Ri, ARi);
                d_m3_mul(ARi, ric, T);
                double v[3];
                d_m3_vec(T, pts_i, v);
                double Jl[2];
                for (int r2 = 0; r2 < 2; ++r2) Jl[r2] = (red[3 * r2] * v[0] + red[3 * r2 + 1] * v[1] + red[3 * r2 + 2] * v[2]) * -1.0 / (lam * lam);
                // host pose (columns 6..11): reduce [ric^T Rj^T | -ric^T Rj^T Ri hat(pb_i)]
                d_reduce_mul<18>(red, A, J, 6);
                d_skew(pb_i, M);
                d_m3_mul(ARi, M, Mm);
                for (int k = 0; k < 9; ++k) Mm[k] = -Mm[k];
                d_reduce_mul<18>(red, Mm, J, 9);
                // target pose (12..17): reduce [-ric^T Rj^T | ric^T hat(pb_j)]
                for (int k = 0; k < 9; ++k) M[k] = -A[k];
                d_reduce_mul<18>(red, M, J, 12);
                d_skew(pb_j, M);
                d_m3_mul(ricT, M, Mm);
                d_reduce_mul<18>(red, Mm, J, 15);
                // extrinsic (0..5), always a variable of Marginalize's graph
                d_m3_mul(RjT, Ri, M);
                M[0] -= 1; M[4] -= 1; M[8] -= 1;
                d_m3_mul(ricT, M, Mm);
                d_reduce_mul<18>(red, Mm, J, 0);
                {
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
                    d_reduce_mul<18>(red, M, J, 3);
                }
                double *er = scr + W.s_edge + (size_t)e * EREC;
                const double c0 = drho * (info * r[0]), c1 = drho * (info * r[1]);
                for (int k = 0; k < 18; ++k) {
                    const double j0 = J[k], j1 = J[18 + k];
                    er[k] = j0; er[18 + k] = j1;
                    er[36 + k] = Wm[0] * j0 + Wm[1] * j1;
                    er[54 + k] = Wm[2] * j0 + Wm[3] * j1;
                    er[72 + k] = -(j0 * c0 + j1 * c1);
                }
                // h_l += J_l^T W J_l, b_l -= drho J_l^T Info r, w_l += (J_l^T W) J_c
                const double t0 = Jl[0] * Wm[0] + Jl[1] * Wm[2], t1 = Jl[0] * Wm[1] + Jl[1] * Wm[3];
                h += t0 * Jl[0] + t1 * Jl[1];
                bl -= Jl[0] * c0 + Jl[1] * c1;
                for (int k = 0; k < 6; ++k) {
                    lr[k] += t0 * J[k] + t1 * J[18 + k];
                    lr[6 + k] += t0 * J[6 + k] + t1 * J[24 + k];
                    lr[6 + 6 * fj + k] += t0 * J[12 + k] + t1 * J[30 + k];
                }
            }
            lr[CD_W] = 1.0 / h;                 // (h = 0: inf, and the Schur term below NaN throughout, as in problem.cc:701-703)
            lr[CD_W + 1] = bl;
            lr[CD_W + 2] = h;
        }
    }
    __syncthreads();

    // phase 2: the lower triangle, thread per entry
    const int ntri = PD * (PD + 1) / 2;
    const int32_t *eoff = ints + W.i_eoff, *tgt = ints + W.i_tgt;
    for (int t = tid; t < ntri + PD; t += BUILD_NT) {
        if (t < ntri) {
            int i = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
            while (i * (i + 1) / 2 > t) --i;
            while ((i + 1) * (i + 2) / 2 <= t) ++i;
            const int j = t - i * (i + 1) / 2;
            double v = 0.0;
            const int ci = mg_cam(i), cj = mg_cam(j);
            if (old && ci >= 0 && cj >= 0) {
                for (int l = 0; l < W.nl; ++l) {
                    for (int e = eoff[l]; e < eoff[l + 1]; ++e) {
                        const int a = mg_col(ci, tgt[e]), b = mg_col(cj, tgt[e]);
                        if (a < 0 || b < 0) continue;
                        const double *er = scr + W.s_edge + (size_t)e * EREC;
                        v += er[a] * er[36 + b] + er[18 + a] * er[54 + b];
                    }
                    const double *lr = scr + W.s_lm + (size_t)l * LREC;
                    v -= lr[ci] * lr[cj] * lr[CD_W];
                }
            }
            if (imu && i >= 6 && i < 36 && j >= 6) {
                const int a = i - 6, bb = j - 6;
                v += (imu_vblock(a) <= imu_vblock(bb)) ? sT[a * 30 + bb] : sT[bb * 30 + a];      // upper vertex blocks computed, lower mirrored
            }
            if (hp && i < PRD) v += hp[(size_t)i * PRD + j];
            Hm[(size_t)i * PD + j] = v;
            Hm[(size_t)j * PD + i] = v;
        } else {
            const int i = t - ntri, ci = mg_cam(i);
            double v = 0.0;
            if (old && ci >= 0) {
                for (int l = 0; l < W.nl; ++l) {
                    for (int e = eoff[l]; e < eoff[l + 1]; ++e) {
                        const int a = mg_col(ci, tgt[e]);
                        if (a >= 0) v += scr[W.s_edge + (size_t)e * EREC + 72 + a];
                    }
                    const double *lr = scr + W.s_lm + (size_t)l * LREC;
                    v -= lr[ci] * lr[CD_W] * lr[CD_W + 1];
                }
            }
            if (imu && i >= 6 && i < 36) v -= sG[i - 6];
            if (bp && i < PRD) v += bp[i];
            bm[i] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// parallel cyclic Jacobi on a packed lower triangle (np even; the caller pads an odd size with a zero row)
//   round r pairs the np indices by the round-robin schedule (index 0 fixed, the others rotated by r); the np/2 rotations of a
//   round are independent: their angles are computed first, then every 2 x 2 block of the matrix and every pair of rows of V^T
//   is updated by one thread.  A sweep is np - 1 rounds; the solver stops after the first sweep in which no pair needed a
//   rotation (|a_pq| <= eps sqrt|a_pp a_qq|), or after JAC_MAX_SWEEPS.  Schedule and test depend on nothing but the values.
// ---------------------------------------------------------------------------------------------------------
constexpr int JAC_MAX_SWEEPS = 40;
__device__ __forceinline__ int tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }
__device__ __forceinline__ int rr_player(int pos, int r, int np) { return pos == 0 ? 0 : 1 + (pos - 1 + r) % (np - 1); }

__device__ void jacobi(double *A, double *Vt, int np, double *sc, double *ss, int *sp, int *sq, int *flag) {
    const int tid = threadIdx.x, nt = blockDim.x, npairs = np / 2;
    for (int t = tid; t < np * np; t += nt) Vt[t] = (t / np == t % np) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < JAC_MAX_SWEEPS; ++sweep) {
        if (tid == 0) *flag = 0;
        __syncthreads();
        for (int r = 0; r < np - 1; ++r) {
            for (int k = tid; k < npairs; k += nt) {
                int p = rr_player(k, r, np), q = rr_player(np - 1 - k, r, np);
                if (p > q) { const int x = p; p = q; q = x; }
                const double app = A[tri(p, p)], aqq = A[tri(q, q)], apq = A[tri(q, p)];
                double c = 1.0, s = 0.0;
                if (apq != 0.0 && !(fabs(apq) <= 2.220446049250313e-16 * sqrt(fabs(app) * fabs(aqq)))) {
                    const double th = (aqq - app) / (2.0 * apq);
                    const double t = fabs(th) > 1e150 ? 0.5 / th : (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                    *flag = 1;
                }
                sc[k] = c; ss[k] = s; sp[k] = p; sq[k] = q;
            }
            __syncthreads();
            // A <- J^T A J, one 2 x 2 block (pair k1 rows, pair k2 columns, k1 >= k2) per task
            const int nblk = npairs * (npairs + 1) / 2;
            for (int t = tid; t < nblk; t += nt) {
                int k1 = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
                while (k1 * (k1 + 1) / 2 > t) --k1;
                while ((k1 + 1) * (k1 + 2) / 2 <= t) ++k1;
                const int k2 = t - k1 * (k1 + 1) / 2;
                const double c1 = sc[k1], s1 = ss[k1], c2 = sc[k2], s2 = ss[k2];
                const int p1 = sp[k1], q1 = sq[k1], p2 = sp[k2], q2 = sq[k2];
                if (k1 == k2) {
                    if (s1 == 0.0) continue;
                    const double app = A[tri(p1, p1)], aqq = A[tri(q1, q1)], apq = A[tri(q1, p1)];
                    const double tt = s1 / c1;
                    A[tri(p1, p1)] = app - tt * apq;
                    A[tri(q1, q1)] = aqq + tt * apq;
                    A[tri(q1, p1)] = 0.0;
                } else {
                    if (s1 == 0.0 && s2 == 0.0) continue;
                    const int ipp = tri(p1, p2), ipq = tri(p1, q2), iqp = tri(q1, p2), iqq = tri(q1, q2);
                    const double bpp = A[ipp], bpq = A[ipq], bqp = A[iqp], bqq = A[iqq];
                    // columns: (B R2)[:, p] = c2 B[:, p] - s2 B[:, q], (B R2)[:, q] = s2 B[:, p] + c2 B[:, q]
                    const double xpp = c2 * bpp - s2 * bpq, xpq = s2 * bpp + c2 * bpq;
                    const double xqp = c2 * bqp - s2 * bqq, xqq = s2 * bqp + c2 * bqq;
                    // rows: R1^T X
                    A[ipp] = c1 * xpp - s1 * xqp;
                    A[ipq] = c1 * xpq - s1 * xqq;
                    A[iqp] = s1 * xpp + c1 * xqp;
                    A[iqq] = s1 * xpq + c1 * xqq;
                }
            }
            // V <- V J: rows p, q of V^T
            for (int t = tid; t < npairs * np; t += nt) {
                const int k = t / np, i = t - k * np;
                const double s = ss[k];
                if (s == 0.0) continue;
                const double c = sc[k];
                double *vp = Vt + (size_t)sp[k] * np + i, *vq = Vt + (size_t)sq[k] * np + i;
                const double a = *vp, b = *vq;
                *vp = c * a - s * b;
                *vq = s * a + c * b;
            }
            __syncthreads();
        }
        const int any = *flag;
        __syncthreads();
        if (!any) break;
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_marg_tail: problem.cc:717-779, one workgroup per window
// ---------------------------------------------------------------------------------------------------------
struct TailLds {
    double tri[TRI_MAX];            // the live block, packed lower triangle (np <= 156)
    double tempB[PRD * M2];         // Arm Amm^+ over the rows of rowlive
    double bp[PRD];                 // brr - Arm Amm^+ bmm
    double ev[PRD], sinv[PRD];
    double amm[16 * 17 / 2], vt16[16 * 16], ainv[M2 * M2];
    double sc[PRD / 2], ss[PRD / 2];
    int sp[PRD / 2], sq[PRD / 2];
    int order[PD];
    int flagrow[PRD], rowlive[PRD], live[PRD], lpos[PRD], rank[PRD], rowof[PRD], colof[PRD], kept[PRD];
    int nr, nl, nk, flag;
};
constexpr size_t TAIL_LDS = sizeof(TailLds);
static_assert(TAIL_LDS <= 160 * 1024, "k_marg_tail's LDS");

__global__ void __launch_bounds__(TAIL_NT) k_marg_tail(const MargWin *__restrict__ wins, double *__restrict__ scr, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double dyn_lds[];
    TailLds &L = *reinterpret_cast<TailLds *>(dyn_lds);
    const MargWin W = wins[blockIdx.x];
    const int tid = threadIdx.x;
    const double *Hin = scr + W.s_H, *bin = Hin + (size_t)PD * PD;
    double *o = out + (size_t)blockIdx.x * OUT_STRIDE;
    double *oH = o, *oJ = o + (size_t)PRD * PRD, *ob = oJ + (size_t)PRD * PRD, *oe = ob + PRD;
    constexpr int n2 = PRD;
    constexpr double eps = 1e-8;

    // a landmark block without an inverse: H_prior 0, the rest NaN (vio_marginalize's outcome for that case)
    int bad = 0;
    for (int t = tid; t < PD * PD + PD; t += TAIL_NT) bad |= !isfinite(Hin[t]);
    if (__syncthreads_or(bad)) {
        for (int t = tid; t < PRD * PRD; t += TAIL_NT) { oH[t] = 0.0; oJ[t] = NAN; }
        for (int t = tid; t < PRD; t += TAIL_NT) { ob[t] = NAN; oe[t] = NAN; }
        if (tid == 0) { oe[PRD] = (double)VIO_ERR_NOT_FINITE; oe[PRD + 1] = 0.0; }
        return;
    }
    // the two moves of problem.cc:721-745 (speed-bias of the frame to the bottom, then its pose) as one index map
    if (tid == 0) {
        int o1[PD], o2[PD];
        auto move = [](int idx, int dim, int *ob_) {
            int q = 0;
            for (int i = 0; i < PD; ++i) if (i < idx || i >= idx + dim) ob_[q++] = i;
            for (int i = idx; i < idx + dim; ++i) ob_[q++] = i;
        };
        move(12 + 15 * W.frame, 9, o1);
        move(6 + 15 * W.frame, 6, o2);
        for (int i = 0; i < PD; ++i) L.order[i] = o1[o2[i]];
    }
    __syncthreads();
    auto Hp = [&](int i, int j) -> double { return Hin[(size_t)L.order[i] * PD + L.order[j]]; };

    // Amm = (A + A^T) / 2 and its pseudo-inverse through its eigen-decomposition (problem.cc:750-756), padded to 16
    for (int t = tid; t < 136; t += TAIL_NT) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= t) ++i;
        const int j = t - i * (i + 1) / 2;
        L.amm[t] = (i < M2 && j < M2) ? 0.5 * (Hp(n2 + i, n2 + j) + Hp(n2 + j, n2 + i)) : 0.0;
    }
    // the rows of the kept block that are not exactly zero all the way (marginalize_tail's rowlive)
    for (int i = tid; i < n2; i += TAIL_NT) {
        const double *hr = Hin + (size_t)L.order[i] * PD;
        int any = 0;
        for (int j = 0; j < PD; ++j) any |= (hr[j] != 0.0);
        for (int j = n2; j < PD; ++j) any |= (Hp(j, i) != 0.0);
        L.flagrow[i] = any;
    }
    __syncthreads();
    jacobi(L.amm, L.vt16, 16, L.sc, L.ss, L.sp, L.sq, &L.flag);
    if (tid == 0) {
        int nr = 0;
        for (int i = 0; i < n2; ++i) if (L.flagrow[i]) L.rowlive[nr++] = i;
        L.nr = nr;
    }
    __syncthreads();
    for (int t = tid; t < M2 * M2; t += TAIL_NT) {
        const int i = t / M2, j = t % M2;
        double s = 0;
        for (int k = 0; k < 16; ++k) {
            const double e = L.amm[tri(k, k)];
            if (e > eps) s += L.vt16[k * 16 + i] * (1.0 / e) * L.vt16[k * 16 + j];
        }
        L.ainv[t] = s;
    }
    __syncthreads();
    const int nr = L.nr;
    // tempB = Arm Amm^+ (rows of rowlive), bp = brr - tempB bmm (problem.cc:758-762)
    for (int t = tid; t < nr * M2; t += TAIL_NT) {
        const int a = t / M2, j = t % M2, i = L.rowlive[a];
        double s = 0;
        for (int k = 0; k < M2; ++k) s += Hp(i, n2 + k) * L.ainv[k * M2 + j];
        L.tempB[t] = s;
    }
    for (int i = tid; i < n2; i += TAIL_NT) L.bp[i] = bin[L.order[i]];
    __syncthreads();
    for (int a = tid; a < nr; a += TAIL_NT) {
        const int i = L.rowlive[a];
        double s = 0;
        for (int k = 0; k < M2; ++k) s += L.tempB[a * M2 + k] * bin[L.order[n2 + k]];
        L.bp[i] = bin[L.order[i]] - s;
    }
    double *Hpc = scr + W.s_hpc;         // nr x nr, row stride 156
    for (int t = tid; t < nr * nr; t += TAIL_NT) {
        const int a = t / nr, c = t - a * nr, i = L.rowlive[a], j = L.rowlive[c];
        double s = 0;
        for (int k = 0; k < M2; ++k) s += L.tempB[a * M2 + k] * Hp(n2 + k, j);
        Hpc[(size_t)a * PRD + c] = Hp(i, j) - s;
    }
    __syncthreads();
    // the live rows: those of the reduced system that are not exactly zero (marginalize_tail's live)
    for (int a = tid; a < nr; a += TAIL_NT) {
        int any = 0;
        for (int c = 0; c < nr; ++c) any |= (Hpc[(size_t)a * PRD + c] != 0.0) | (Hpc[(size_t)c * PRD + a] != 0.0);
        L.flagrow[a] = any;
    }
    __syncthreads();
    if (tid == 0) {
        int nl = 0;
        for (int a = 0; a < nr; ++a) if (L.flagrow[a]) { L.live[nl] = L.rowlive[a]; L.lpos[nl] = a; ++nl; }
        L.nl = nl;
    }
    __syncthreads();
    const int nl = L.nl, np = nl + (nl & 1);
    for (int t = tid; t < np * (np + 1) / 2; t += TAIL_NT) {
        int a = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while (a * (a + 1) / 2 > t) --a;
        while ((a + 1) * (a + 2) / 2 <= t) ++a;
        const int c = t - a * (a + 1) / 2;
        L.tri[t] = (a < nl && c < nl) ? Hpc[(size_t)L.lpos[a] * PRD + L.lpos[c]] : 0.0;      // the lower triangle, as Eigen reads it
    }
    __syncthreads();
    double *Vt = scr + W.s_vt;           // np x np
    if (np > 0) jacobi(L.tri, Vt, np, L.sc, L.ss, L.sp, L.sq, &L.flag);
    // eigenvalues ascending (SelfAdjointEigenSolver's order); the nz dead indices are eigenvalue-0 unit vectors ahead of them
    for (int a = tid; a < nl; a += TAIL_NT) L.ev[a] = L.tri[tri(a, a)];
    __syncthreads();
    for (int a = tid; a < nl; a += TAIL_NT) {
        const double e = L.ev[a];
        int r = 0;
        for (int b = 0; b < nl; ++b) r += (L.ev[b] < e || (L.ev[b] == e && b < a)) ? 1 : 0;
        L.rank[a] = r;
        L.sinv[a] = e > eps ? sqrt(1.0 / e) : 0.0;
    }
    for (int i = tid; i < n2; i += TAIL_NT) { L.rowof[i] = -1; L.colof[i] = -1; }
    __syncthreads();
    const int nz = n2 - nl;
    for (int a = tid; a < nl; a += TAIL_NT) {
        L.colof[L.live[a]] = a;
        if (L.ev[a] > eps) L.rowof[nz + L.rank[a]] = a;
    }
    __syncthreads();
    if (tid == 0) {       // the kept eigenpairs in ascending order
        int nk = 0;
        for (int i = nz; i < n2; ++i) if (L.rowof[i] >= 0) L.kept[nk++] = L.rowof[i];
        L.nk = nk;
    }
    __syncthreads();
    const int nk = L.nk;
    // Jt_inv = S^-1/2 V^T on the kept rows (problem.cc:770-773), err = -Jt_inv b (:774)
    for (int t = tid; t < n2 * n2; t += TAIL_NT) {
        const int i = t / n2, j = t - i * n2, a = L.rowof[i], c = L.colof[j];
        oJ[t] = (a >= 0 && c >= 0) ? L.sinv[a] * Vt[(size_t)a * np + c] : 0.0;
    }
    for (int i = tid; i < n2; i += TAIL_NT) {
        const int a = L.rowof[i];
        // (compensated: the terms cancel to |err| from |Jt_inv| |b| many orders larger; TwoProduct by fma, Neumaier's TwoSum)
        double s = 0, comp = 0;
        if (a >= 0)
            for (int c = 0; c < nl; ++c) {
                const double x = -(L.sinv[a] * Vt[(size_t)a * np + c]), y = L.bp[L.live[c]];
                const double p = x * y, pe = fma(x, y, -p);
                const double t = s + p;
                comp += (fabs(s) >= fabs(p) ? (s - t) + p : (p - t) + s) + pe;
                s = t;
            }
        oe[i] = s + comp;
        ob[i] = L.bp[i];
    }
    // H_prior = J^T J = sum over the kept eigenpairs, ascending, of V_ik s_k V_jk; |H| <= 1e-9 zeroed (problem.cc:775-778)
    for (int t = tid; t < n2 * n2; t += TAIL_NT) {
        const int i = t / n2, j = t - i * n2, a = L.colof[i], c = L.colof[j];
        double v = 0.0;
        if (a >= 0 && c >= 0) {
            double s = 0;
            for (int q = 0; q < nk; ++q) {
                const int k = L.kept[q];
                s += Vt[(size_t)k * np + a] * L.ev[k] * Vt[(size_t)k * np + c];
            }
            v = fabs(s) > 1e-9 ? s : 0.0;
        }
        oH[t] = v;
    }
    if (tid == 0) { oe[PRD] = (double)VIO_OK; oe[PRD + 1] = (double)nl; }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_marg {
    vio_config cfg;
    int device = 0;
    ErrText err = {0};
    Twin<char> staging;                                   // descriptors | ints | doubles
    DevBuf<double> scr;
    Twin<double> out;
    StreamEvents<4> q;                                    // events: upload start, build, tail, end
    double timing[4] = {NAN, NAN, NAN, NAN};
    std::vector<int32_t> live;
};

namespace {

// the graph of one window: the landmarks hosted in frame 0 (MargOldFrame, estimator.cpp:762-764) with their edges in the caller's order
struct Graph {
    std::vector<int32_t> lms, eoff, edges;
};

// argument checks of one item (nothing is written); the graph of a VIO_MARG_OLD window
vio_status check_item(vio_marg *h, int i, const vio_marg_item &it, Graph &g) {
    if (it.kind != VIO_MARG_OLD && it.kind != VIO_MARG_SECOND_NEW) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: kind is neither VIO_MARG_OLD nor VIO_MARG_SECOND_NEW", i);
    if (!it.H || !it.b || !it.err || !it.jt_inv) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: an output array is NULL", i);
    if ((it.H_prior == nullptr) != (it.b_prior == nullptr)) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: H_prior and b_prior must both be given or both be NULL", i);
    if (it.kind == VIO_MARG_SECOND_NEW) return VIO_OK;
    if (!it.poses || !it.speed_bias || !it.ext) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: poses, speed_bias and ext are required", i);
    if (it.n < 0 || it.m < 0 || it.n > INT32_MAX || it.m > INT32_MAX) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: negative or too large n / m", i);
    if (it.n > 0 && !it.inv_depth) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: inv_depth is NULL", i);
    if (it.m > 0 && (!it.lm || !it.host || !it.target || !it.pts_i || !it.pts_j)) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: an observation array is NULL", i);
    std::vector<int32_t> lhost((size_t)it.n, -1), cnt((size_t)it.n + 1, 0);
    std::vector<int64_t> first((size_t)it.n, -1);
    std::vector<uint32_t> seen((size_t)it.n, 0u);
    for (int64_t e = 0; e < it.m; ++e) {
        const int32_t l = it.lm[e], ho = it.host[e], t = it.target[e];
        if (l < 0 || l >= it.n) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: observation %lld: landmark index out of range", i, (long long)e);
        if (ho < 0 || ho >= NF || t < 0 || t >= NF) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: observation %lld: frame index out of range", i, (long long)e);
        if (ho == t) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: observation %lld: host == target", i, (long long)e);
        if (first[l] < 0) { first[l] = e; lhost[l] = ho; }
        else if (lhost[l] != ho || it.pts_i[2 * e] != it.pts_i[2 * first[l]] || it.pts_i[2 * e + 1] != it.pts_i[2 * first[l] + 1])
            return fail(h->err, VIO_ERR_BAD_ARG, "window %d: landmark %d: its observations disagree on the host frame or pts_i", i, l);
        if (seen[l] & (1u << t)) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: landmark %d: two observations in one frame", i, l);
        seen[l] |= 1u << t;
        ++cnt[l + 1];
    }
    // landmarks hosted in frame 0, ascending; their edges grouped stably
    std::vector<int32_t> slot((size_t)it.n, -1);
    g.lms.clear(); g.eoff.assign(1, 0);
    for (int64_t l = 0; l < it.n; ++l)
        if (lhost[l] == 0) { slot[l] = (int32_t)g.lms.size(); g.lms.push_back((int32_t)l); g.eoff.push_back(g.eoff.back() + cnt[l + 1]); }
    g.edges.assign(g.eoff.back(), -1);
    std::vector<int32_t> fill(g.eoff.begin(), g.eoff.end() - 1);
    for (int64_t e = 0; e < it.m; ++e) {
        const int32_t s = slot[it.lm[e]];
        if (s >= 0) g.edges[fill[s]++] = (int32_t)e;
    }
    return VIO_OK;
}

}  // namespace

extern "C" {

int32_t vio_marg_version(void) { return VIO_MARG_VERSION; }

const char *vio_marg_last_error(const vio_marg *h) { return h ? h->err : "NULL handle"; }

vio_status vio_marg_set_config(vio_marg *h, const vio_config *cfg) {
    if (!h || !cfg) return VIO_ERR_BAD_ARG;
    if (cfg->device != h->cfg.device || (cfg->stream && cfg->stream != (void *)h->q.stream) || (!cfg->stream && !h->q.own_stream))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_marg_set_config: device and stream must be those of vio_marg_create");
    void *st = h->cfg.stream;
    h->cfg = *cfg;
    h->cfg.stream = st;
    return VIO_OK;
}

vio_status vio_marg_create(const vio_config *cfg, vio_marg **out) {
    if (!cfg || !out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VIO_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return VIO_ERR_BAD_ARG;
    DeviceScope dev(cfg->device);
    if (!dev.ok) return VIO_ERR_HIP;
    vio_marg *h = new (std::nothrow) vio_marg();
    if (!h) return VIO_ERR_BAD_ARG;
    h->cfg = *cfg;
    h->device = cfg->device;
    if (h->q.open_stream(cfg->stream) != hipSuccess) { delete h; return VIO_ERR_HIP; }
    h->cfg.stream = h->q.stream;
    if (h->q.create_events() != hipSuccess) { vio_marg_destroy(h); return VIO_ERR_HIP; }
    if (hipFuncSetAttribute((const void *)k_marg_tail, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TAIL_LDS) != hipSuccess) {
        vio_marg_destroy(h);
        return VIO_ERR_HIP;
    }
    *out = h;
    return VIO_OK;
}

void vio_marg_destroy(vio_marg *h) { destroy_handle(h); }

vio_status vio_marg_timing(vio_marg *h, double *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_marg_live_rows(vio_marg *h, int32_t i, int32_t *rows) {
    if (!h || !rows || i < 0 || (size_t)i >= h->live.size()) return VIO_ERR_BAD_ARG;
    *rows = h->live[(size_t)i];
    return VIO_OK;
}

vio_status vio_marg_compute(vio_marg *h, const vio_marg_item *item) {
    if (!h || !item) return VIO_ERR_BAD_ARG;
    vio_status ws = VIO_OK;
    const vio_status st = vio_marg_compute_batch(h, 1, item, &ws);
    return st;
}

vio_status vio_marg_compute_batch(vio_marg *h, int32_t count, const vio_marg_item *items, vio_status *window_status) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || (count > 0 && !items)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_marg_compute_batch: negative count or NULL items");
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Graph> graphs((size_t)count);
    for (int i = 0; i < count; ++i) {
        const vio_status st = check_item(h, i, items[i], graphs[(size_t)i]);
        if (st != VIO_OK) return st;
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    // layout of the staging buffer (descriptors | ints | doubles) and of the scratch
    std::vector<MargWin> wins((size_t)count);
    int64_t nd = 0, ni = 0, ns = 0;
    for (int i = 0; i < count; ++i) {
        const vio_marg_item &it = items[i];
        const Graph &g = graphs[(size_t)i];
        MargWin &w = wins[(size_t)i];
        std::memset(&w, 0, sizeof(w));
        const bool old = it.kind == VIO_MARG_OLD;
        w.kind = it.kind; w.frame = old ? 0 : VIO_WINDOW_SIZE - 1;
        w.has_imu = old && it.imu0 != nullptr; w.has_prior = it.H_prior != nullptr;
        w.nl = old ? (int32_t)g.lms.size() : 0; w.ne = old ? (int32_t)g.edges.size() : 0;
        w.o_state = nd; nd += STATE_D;
        w.o_pre = nd; nd += PRE_STRIDE;
        w.o_hp = nd; nd += w.has_prior ? (int64_t)PRD * PRD : 0;
        w.o_bp = nd; nd += w.has_prior ? PRD : 0;
        w.o_invd = nd; nd += w.nl;
        w.o_ptsi = nd; nd += 2 * (int64_t)w.nl;
        w.o_ptsj = nd; nd += 2 * (int64_t)w.ne;
        w.i_eoff = ni; ni += w.nl + 1;
        w.i_tgt = ni; ni += w.ne;
        w.s_edge = ns; ns += (int64_t)w.ne * EREC;
        w.s_lm = ns; ns += (int64_t)w.nl * LREC;
        w.s_H = ns; ns += (int64_t)PD * PD + PD;
        w.s_hpc = ns; ns += (int64_t)PRD * PRD;
        w.s_vt = ns; ns += (int64_t)PRD * PRD;
    }
    const size_t b_desc = align256(sizeof(MargWin) * (size_t)count);
    const size_t b_ints = align256(sizeof(int32_t) * (size_t)ni);
    const size_t stage = b_desc + b_ints + sizeof(double) * (size_t)nd;
    const size_t outb = sizeof(double) * OUT_STRIDE * (size_t)count;
    vio_status rc;
    if ((rc = h->staging.ensure(h->err, stage)) != VIO_OK || (rc = h->scr.ensure(h->err, sizeof(double) * (size_t)ns)) != VIO_OK ||
        (rc = h->out.ensure(h->err, outb)) != VIO_OK)
        return rc;
    // pack
    std::memcpy(h->staging.h, wins.data(), sizeof(MargWin) * (size_t)count);
    int32_t *hi = (int32_t *)(h->staging.h + b_desc);
    double *hd = (double *)(h->staging.h + b_desc + b_ints);
    for (int i = 0; i < count; ++i) {
        const vio_marg_item &it = items[i];
        const Graph &g = graphs[(size_t)i];
        const MargWin &w = wins[(size_t)i];
        double *st = hd + w.o_state;
        if (it.kind == VIO_MARG_OLD) {
            std::memcpy(st, it.ext, 7 * 8); std::memcpy(st + 7, it.poses, 77 * 8); std::memcpy(st + 84, it.speed_bias, 99 * 8);
        } else std::memset(st, 0, STATE_D * 8);
        double *o = hd + w.o_pre;
        std::memset(o, 0, PRE_STRIDE * 8);
        if (w.has_imu) {
            const vio_preint *pre = it.imu0;
            o[PRE_SUMDT] = pre->sum_dt;
            for (int k = 0; k < 3; ++k) { o[PRE_DP + k] = pre->delta_p[k]; o[PRE_DV + k] = pre->delta_v[k]; o[PRE_BA + k] = pre->linearized_ba[k]; o[PRE_BG + k] = pre->linearized_bg[k]; }
            for (int k = 0; k < 4; ++k) o[PRE_DQ + k] = pre->delta_q[k];
            std::memcpy(o + PRE_JAC, pre->jacobian, 225 * 8);
            vio_host::inverse15(pre->covariance, o + PRE_INFO);     // SetInformation(covariance.inverse()), edge_imu.cc:35 — libvio_hip's routine
        }
        if (w.has_prior) { std::memcpy(hd + w.o_hp, it.H_prior, (size_t)PRD * PRD * 8); std::memcpy(hd + w.o_bp, it.b_prior, PRD * 8); }
        int32_t *eoff = hi + w.i_eoff, *tgt = hi + w.i_tgt;
        eoff[0] = 0;
        for (int l = 0; l < w.nl; ++l) {
            const int32_t L = g.lms[(size_t)l];
            hd[w.o_invd + l] = it.inv_depth[L];
            const int32_t e0 = g.edges[(size_t)g.eoff[(size_t)l]];
            hd[w.o_ptsi + 2 * l] = it.pts_i[2 * e0]; hd[w.o_ptsi + 2 * l + 1] = it.pts_i[2 * e0 + 1];
            eoff[l + 1] = g.eoff[(size_t)l + 1];
        }
        for (int q = 0; q < w.ne; ++q) {
            const int32_t e = g.edges[(size_t)q];
            tgt[q] = it.target[e];
            hd[w.o_ptsj + 2 * q] = it.pts_j[2 * e]; hd[w.o_ptsj + 2 * q + 1] = it.pts_j[2 * e + 1];
        }
    }
    MargCfg mc;
    mc.loss_type = h->cfg.loss_type; mc.loss_delta = h->cfg.loss_delta; mc.sqrt_info = h->cfg.reproj_sqrt_info;
    for (int k = 0; k < 3; ++k) mc.gravity[k] = h->cfg.gravity[k];
    const MargWin *dw = (const MargWin *)h->staging.d;
    const int32_t *di = (const int32_t *)(h->staging.d + b_desc);
    const double *dd = (const double *)(h->staging.d + b_desc + b_ints);
    const auto t1 = std::chrono::steady_clock::now();
    (void)hipEventRecord(h->q.ev[0], h->q.stream);
    if (hipMemcpyAsync(h->staging.d, h->staging.h, stage, hipMemcpyHostToDevice, h->q.stream) != hipSuccess)
        return fail(h->err, VIO_ERR_HIP, "vio_marg_compute_batch: upload failed");
    (void)hipEventRecord(h->q.ev[1], h->q.stream);
    hipLaunchKernelGGL(k_marg_build, dim3(count), dim3(BUILD_NT), 0, h->q.stream, dw, di, dd, h->scr.d, mc);
    (void)hipEventRecord(h->q.ev[2], h->q.stream);
    hipLaunchKernelGGL(k_marg_tail, dim3(count), dim3(TAIL_NT), TAIL_LDS, h->q.stream, dw, h->scr.d, h->out.d);
    (void)hipEventRecord(h->q.ev[3], h->q.stream);
    if (hipGetLastError() != hipSuccess) return fail(h->err, VIO_ERR_HIP, "vio_marg_compute_batch: kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, outb, hipMemcpyDeviceToHost, h->q.stream) != hipSuccess ||
        hipStreamSynchronize(h->q.stream) != hipSuccess)
        return fail(h->err, VIO_ERR_HIP, "vio_marg_compute_batch: kernels or read-back failed");
    // hand out
    vio_status ret = VIO_OK;
    h->live.assign((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
        const vio_marg_item &it = items[i];
        const double *o = h->out.h + OUT_STRIDE * (size_t)i;
        std::memcpy(it.H, o, (size_t)PRD * PRD * 8);
        std::memcpy(it.jt_inv, o + (size_t)PRD * PRD, (size_t)PRD * PRD * 8);
        std::memcpy(it.b, o + (size_t)2 * PRD * PRD, PRD * 8);
        std::memcpy(it.err, o + (size_t)2 * PRD * PRD + PRD, PRD * 8);
        const vio_status ws = (vio_status)(int)o[(size_t)2 * PRD * PRD + 2 * PRD];
        h->live[(size_t)i] = (int32_t)o[(size_t)2 * PRD * PRD + 2 * PRD + 1];
        if (window_status) window_status[i] = ws;
        if (ws != VIO_OK) {
            ret = ws;
            if (!h->err[0])
                fail(h->err, ws, "window %d: a landmark block has no inverse; the prior is the reference's outcome for that case (H_prior 0, the rest NaN)", i);
        }
    }
    const float ms0 = elapsed_ms(h->q.ev[0], h->q.ev[1]), ms1 = elapsed_ms(h->q.ev[1], h->q.ev[2]), ms2 = elapsed_ms(h->q.ev[2], h->q.ev[3]);
    const auto t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + ms0;     // host pack, then the H2D copy on the stream
    h->timing[1] = ms1; h->timing[2] = ms2;
    h->timing[3] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return ret;
}

}  // extern "C"
