// vio_covariance.hip — marginal covariances of a solved window (include/vio_covariance.h).
//
// A companion of libvio_hip.so that uses nothing but its C ABI: the system and the states are read back through the getters, and
// the two kernels below run on the context's stream.
//   k_cov_pose          one workgroup: the reduced H_pp_schur (fixed variables removed) as a packed lower triangle in LDS, inverted
//                       in place by the symmetric sweep; Sigma written once as a full 171 x 171 and as the 72 x 72 camera block.
//   k_cov_landmarks<D>  one lane per landmark: its observations' reprojection Jacobians and robust weights recomputed, h_l and w_l
//                       accumulated in a fixed order, then the quadratic form against Sigma_cc staged in LDS.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vio_device_math.h"
#include "vio_obs_csr.h"
#include "../../include/vio_covariance.h"

#define PD VIO_POSE_DIM                    // 171
#define CD VIO_CAM_DIM                     // 72
#define NF VIO_NUM_FRAMES                  // 11
#define TRI_MAX (PD * (PD + 1) / 2)        // 14706 doubles: 117.6 KB

#define POSE_NT 1024
#define POSE_PER ((TRI_MAX + POSE_NT - 1) / POSE_NT)     // 15 packed entries per thread

// camera variable a (0..71: ext, then pose f at 6 + 6f) -> its place in the 171-ordering
__host__ __device__ inline int cam_to_full(int a) { return a < 6 ? a : 6 + 15 * ((a - 6) / 6) + (a - 6) % 6; }
__device__ inline int tri(int i, int j) { return i * (i + 1) / 2 + j; }          // i >= j

// ---------------------------------------------------------------------------------------------------------------------------------
// k_cov_pose: Sigma = S^-1 of the reduced system (n <= 171 kept variables), by the sweep operator on the packed lower triangle.
// Sweeping pivot k of a symmetric A (Goodnight 1979):
//     a_kk <- -1/a_kk,   a_ik <- a_ik / a_kk  (i != k),   a_ij <- a_ij - a_ik a_kj / a_kk  (i, j != k)
// After all n pivots A holds -S^-1.  The pivots met on the way are the D of S = L D L^T in the same order (the unswept block is
// always the Schur complement of the swept one), so "every pivot positive and finite" is exactly the LDL^T test of S being
// positive definite; the first one that fails is reported and nothing else is written.
// Every packed entry belongs to one thread for the whole sweep and is updated in the same order each time: results are bitwise
// reproducible.  (Keeping a thread's 15 entries in registers, with the pivot column double-buffered and one barrier per pivot, was
// measured slower — 504 against 437 us — and dropped: DESIGN.md section 10.)
// ratio[0]: min over the pivots of d_k / S_kk (1: diagonal; ~1/kappa: nearly singular) — VIO_OK says only that every d_k > 0.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(POSE_NT) k_cov_pose(const double *__restrict__ S, const int *__restrict__ keep, int n,
                                                       double *__restrict__ cov, double *__restrict__ cc, int *__restrict__ status,
                                                       double *__restrict__ ratio) {
    __shared__ double A[TRI_MAX];
    __shared__ double col[PD + 1];           // pivot column k
    __shared__ double dg[PD];                // diagonal of S (the pivot ratio)
    __shared__ int red[PD];                  // 171-index -> reduced index, -1: held fixed
    const int tid = threadIdx.x;
    const int ntri = n * (n + 1) / 2;

    for (int q = tid; q < PD; q += POSE_NT) red[q] = -1;
    __syncthreads();
    for (int q = tid; q < n; q += POSE_NT) { red[keep[q]] = q; dg[q] = S[(size_t)keep[q] * PD + keep[q]]; }

    // the thread's packed entries and their (row, column), found once
    int ij[POSE_PER];                        // row << 16 | column
#pragma unroll
    for (int s = 0; s < POSE_PER; ++s) {
        const int p = tid + s * POSE_NT;
        int i = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
        while ((i + 1) * (i + 2) / 2 <= p) ++i;
        while (i * (i + 1) / 2 > p) --i;
        const int j = p - i * (i + 1) / 2;
        ij[s] = (i << 16) | j;
        if (p < ntri) A[p] = S[(size_t)keep[i] * PD + keep[j]];          // lower triangle of S (keep is ascending)
    }
    __syncthreads();

    double rmin = 1.0;
    for (int k = 0; k < n; ++k) {
        if (tid < n) col[tid] = A[tid >= k ? tri(tid, k) : tri(k, tid)];
        __syncthreads();
        const double d = col[k];
        if (!(d > 0.0) || !isfinite(d)) {          // uniform: every thread read the same pivot
            if (tid == 0) status[0] = k;
            return;
        }
        rmin = fmin(rmin, d / dg[k]);
        const double dinv = 1.0 / d;
#pragma unroll
        for (int s = 0; s < POSE_PER; ++s) {
            const int p = tid + s * POSE_NT;
            if (p < ntri) {
                const int i = ij[s] >> 16, j = ij[s] & 0xffff;
                if (i == k && j == k) A[p] = -dinv;
                else if (i == k) A[p] = col[j] * dinv;
                else if (j == k) A[p] = col[i] * dinv;
                else A[p] = A[p] - (col[i] * dinv) * col[j];
            }
        }
        __syncthreads();
    }
    if (tid == 0) { status[0] = -1; ratio[0] = rmin; }

    for (int q = tid; q < PD * PD; q += POSE_NT) {
        const int r = red[q / PD], c = red[q % PD];
        cov[q] = (r >= 0 && c >= 0) ? -A[r >= c ? tri(r, c) : tri(c, r)] : 0.0;
    }
    for (int q = tid; q < CD * CD; q += POSE_NT) {
        const int r = red[cam_to_full(q / CD)], c = red[cam_to_full(q % CD)];
        cc[q] = (r >= 0 && c >= 0) ? -A[r >= c ? tri(r, c) : tri(c, r)] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k_cov_landmarks<D>: D = 1 inverse depth (EdgeReprojection), D = 3 world point (EdgeReprojectionXYZ).
// ---------------------------------------------------------------------------------------------------------------------------------
struct CovLmArgs {
    const double *cc;          // [72 x 72] Sigma_cc
    const double *poses;       // [11][7]
    const double *ext;         // [7]
    const double *val;         // [n][D] inverse depths / world points
    const double *pts_i;       // [n][2] host observation (D = 1)
    const double *pts_j;       // [m][2] in CSR order
    const int *off;            // [n + 1]
    const int *ofr;            // [m] target frame (D = 1) / observing frame (D = 3), CSR order
    const int *ohost;          // [n] host frame (D = 1)
    int n;
    int ext_free;              // D = 1: the extrinsic is a variable of the edges
    int loss_type;
    double loss_delta;
    double sqrt_info;
    double *out;               // [n] var_l  /  [n][9] Sigma_l
    double *info;              // [n] h_l    /  [n][9] H_ll
    int *bad;                  // smallest landmark whose information is not positive definite and finite (atomicMin)
};

template <int D> struct LmNT;
template <> struct LmNT<1> { static constexpr int v = 128; };     // LDS: Sigma_cc 41.5 KB + w 72 x 128 x 8 = 73.7 KB
template <> struct LmNT<3> { static constexpr int v = 64; };      // LDS: Sigma_cc 41.5 KB + W 216 x 64 x 8 = 110.6 KB

DEV void skew3(const double *v, double *S) {
    S[0] = 0;     S[1] = -v[2]; S[2] = v[1];
    S[3] = v[2];  S[4] = 0;     S[5] = -v[0];
    S[6] = -v[1]; S[7] = v[0];  S[8] = 0;
}

// Edge::RobustInfo (edge.cc:48-74) for information s^2 I2: W row-major 2x2; type 0 = no loss object.  The same expression as
// k_linearize's, so that the landmark terms carry the weights H_pp_schur was formed with.  (For Huber beyond delta the test
// rho' + 2 rho'' e2 > 0 is exactly zero in exact arithmetic and its outcome is the rounding of the residual: DESIGN.md section 10.)
DEV void robust_info2(int type, double delta, double s, const double *r, double *W) {
    const double info = s * s;
    if (type == 0) { W[0] = info; W[1] = 0; W[2] = 0; W[3] = info; return; }
    const double e2 = r[0] * (info * r[0]) + r[1] * (info * r[1]);
    double r0, r1, r2;
    d_loss(type, delta, e2, r0, r1, r2);
    const double w0 = s * r[0], w1 = s * r[1];
    double ri[4] = {r1, 0, 0, r1};
    if (r1 + 2 * r2 * e2 > 0.) {
        const double c = 2 * r2;
        ri[0] += c * w0 * w0; ri[1] += c * w0 * w1; ri[2] += c * w1 * w0; ri[3] += c * w1 * w1;
    }
    W[0] = ri[0] * info; W[1] = ri[1] * info; W[2] = ri[2] * info; W[3] = ri[3] * info;
}

// rows of reduce (2x3) times a 3x3 M: out 2x3, written into the 6 columns [c0, c0 + 3) of a 2 x 6 row-major J
DEV void reduce_mul(const double *red, const double *M, double *J, int c0) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            J[6 * r + c0 + c] = red[3 * r] * M[c] + red[3 * r + 1] * M[3 + c] + red[3 * r + 2] * M[6 + c];
}

template <int D>
__global__ void __launch_bounds__(LmNT<D>::v) k_cov_landmarks(CovLmArgs a) {
    constexpr int NT = LmNT<D>::v;
    __shared__ double sc[CD * CD];
    __shared__ double wl[CD * D * NT];          // the lane's coupling column, variable-major: [(72 * d + var) * NT + lane]
    __shared__ double sR[(NF + 1) * 9];         // rotations of the 11 poses and (slot 11) of the extrinsic
    const int tid = threadIdx.x;
    for (int q = tid; q < CD * CD; q += NT) sc[q] = a.cc[q];
    for (int f = tid; f <= NF; f += NT) d_quat_to_R(f < NF ? a.poses + 7 * f + 3 : a.ext + 3, sR + 9 * f);
    for (int q = 0; q < CD * D; ++q) wl[q * NT + tid] = 0.0;
    __syncthreads();
    const int l = blockIdx.x * NT + tid;
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
            robust_info2(a.loss_type, a.loss_delta, s, r, W);
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
            reduce_mul(red, A, Ji, 0);
            skew3(pb_i, M);
            double Mm[9];
            d_m3_mul(ARi, M, Mm);
            for (int k = 0; k < 9; ++k) Mm[k] = -Mm[k];
            reduce_mul(red, Mm, Ji, 3);
            // J_pose_j = reduce [-ric^T Rj^T | ric^T hat(pb_j)]
            for (int k = 0; k < 9; ++k) M[k] = -A[k];
            reduce_mul(red, M, Jj, 0);
            skew3(pb_j, M);
            d_m3_mul(ricT, M, Mm);
            reduce_mul(red, Mm, Jj, 3);
            // J_ext = reduce [ric^T (Rj^T Ri - I) | -T hat(pc_i) + hat(T pc_i) + hat(ric^T (Rj^T (Ri tic + Pi - Pj) - tic))]
            if (a.ext_free) {
                d_m3_mul(RjT, Ri, M);
                M[0] -= 1; M[4] -= 1; M[8] -= 1;
                d_m3_mul(ricT, M, Mm);
                reduce_mul(red, Mm, Je, 0);
                double S1[9], t1[9], v2[3], S2[9], u[3], ww[3], x[3], S3[9];
                skew3(pc_i, S1);
                d_m3_mul(T, S1, t1);
                d_m3_vec(T, pc_i, v2);
                skew3(v2, S2);
                d_m3_vec(Ri, tic, u);
                for (int k = 0; k < 3; ++k) u[k] = u[k] + Pi[k] - Pj[k];
                d_m3_tvec(Rj, u, ww);
                for (int k = 0; k < 3; ++k) ww[k] -= tic[k];
                d_m3_tvec(ric, ww, x);
                skew3(x, S3);
                for (int k = 0; k < 9; ++k) M[k] = -t1[k] + S2[k] + S3[k];
                reduce_mul(red, M, Je, 3);
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
            robust_info2(a.loss_type, a.loss_delta, s, r, W);
            const double red[6] = {1. / dep, 0, -pc[0] / (dep * dep), 0, 1. / dep, -pc[1] / (dep * dep)};
            double RT[9], M[9], Mm[9], Jp[12], Jf[6];
#pragma unroll
            for (int r2 = 0; r2 < 3; ++r2)
#pragma unroll
                for (int c = 0; c < 3; ++c) RT[3 * r2 + c] = Rj[3 * c + r2];
            // J_pose = reduce [ric^T (-Ri^T) | ric^T hat(pts_imu)],  J_feature = reduce ric^T Ri^T
            d_m3_mul(ricT, RT, Mm);
            for (int k = 0; k < 9; ++k) M[k] = -Mm[k];
            reduce_mul(red, M, Jp, 0);
            skew3(pim, M);
            double Mh[9];
            d_m3_mul(ricT, M, Mh);
            reduce_mul(red, Mh, Jp, 3);
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
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
struct vio_cov {
    vio_ctx *ctx = nullptr;
    vio_config cfg;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    char err[512] = {0};
    // device: S | poses | ext | val | pts_i | pts_j (doubles), then keep | off | ofr | ohost | status (ints): one upload
    double *d_in = nullptr;
    size_t in_cap = 0;
    double *h_in = nullptr;                 // pinned mirror of d_in
    // device: cov | cc | out | info (doubles), then status (2 ints): one read-back
    double *d_out = nullptr;
    size_t out_cap = 0;
    double *h_out = nullptr;
    int64_t last_n = -1;
    int last_dim = 0;
    std::vector<double> info;               // of the last successful compute
    double timing[4] = {0, 0, 0, 0};
    double pivot_ratio = 0.0;               // of the last successful compute
    bool relinearize = false;               // vio_cov_set_config changed what the system depends on: the context's linearisation, if it
                                            // holds one, is of the old configuration (vio_set_config keeps it), so linearise first
};

// The calling thread's current device is the caller's: switched to the context's for the library's calls, put back on the way out.
struct DeviceScope {
    int prev = -1;
    bool ok = false;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

static vio_status fail(vio_cov *cv, vio_status st, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(cv->err, sizeof(cv->err), fmt, ap);
    va_end(ap);
    return st;
}

static vio_status hip_ck(vio_cov *cv, hipError_t e, const char *what) {
    if (e == hipSuccess) return VIO_OK;
    return fail(cv, VIO_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// grow a pinned host buffer and its device twin to hold `bytes`
static vio_status ensure(vio_cov *cv, double **d, double **h, size_t *cap, size_t bytes) {
    if (bytes <= *cap) return VIO_OK;
    if (*d) hipFree(*d);
    if (*h) hipHostFree(*h);
    *d = nullptr; *h = nullptr; *cap = 0;
    size_t want = bytes + bytes / 4 + 4096;
    vio_status st = hip_ck(cv, hipMalloc((void **)d, want), "hipMalloc");
    if (st != VIO_OK) return st;
    st = hip_ck(cv, hipHostMalloc((void **)h, want, hipHostMallocDefault), "hipHostMalloc");
    if (st != VIO_OK) return st;
    *cap = want;
    return VIO_OK;
}

static const char *var_name(int full, char *buf, size_t len) {
    if (full < 6) snprintf(buf, len, "extrinsic component %d", full);
    else {
        const int f = (full - 6) / 15, o = (full - 6) % 15;
        if (o < 6) snprintf(buf, len, "pose %d component %d", f, o);
        else snprintf(buf, len, "speed-bias %d component %d", f, o - 6);
    }
    return buf;
}

#define NO_BAD_LM 0x7f7f7f7f

static size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

// D = 1: obs (host, target, pts_i, pts_j); D = 3: obs (frame, pts) in `target` / `pts_j`
static vio_status compute(vio_cov *cv, int D, int32_t gauge, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                          const double *pts_i, const double *pts_j, int64_t n, double *pose_cov, double *lm_out) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    if (gauge != VIO_COV_GAUGE_NONE && gauge != VIO_COV_GAUGE_FIX_OLDEST) return fail(cv, VIO_ERR_BAD_ARG, "unknown gauge %d", gauge);
    if (m < 0 || n < 0 || n > INT32_MAX / 9 || m > INT32_MAX) return fail(cv, VIO_ERR_BAD_ARG, "bad sizes m=%lld n=%lld", (long long)m, (long long)n);
    if (m > 0 && (!lm || !target || !pts_j || (D == 1 && (!host || !pts_i)))) return fail(cv, VIO_ERR_BAD_ARG, "observation array is NULL");
    for (int64_t e = 0; e < m; ++e) {
        if (lm[e] < 0 || lm[e] >= n || target[e] < 0 || target[e] >= NF || (D == 1 && (host[e] < 0 || host[e] >= NF)))
            return fail(cv, VIO_ERR_BAD_ARG, "observation %lld refers to landmark %d / frame out of range", (long long)e, lm[e]);
    }
    DeviceScope dev(cv->cfg.device);
    if (!dev.ok) return fail(cv, VIO_ERR_HIP, "hipSetDevice(%d)", cv->cfg.device);
    vio_status st = VIO_OK;

    // layout of the upload
    const size_t oS = 0, oP = oS + PD * PD, oE = oP + NF * 7, oV = align8(oE + 7), oPi = align8(oV + (size_t)n * D),
                 oPj = align8(oPi + (D == 1 ? 2 * (size_t)n : 0)), nd = align8(oPj + 2 * (size_t)m);
    const size_t iKeep = 0, iOff = iKeep + PD + 1, iOfr = iOff + (size_t)n + 1, iHost = iOfr + (size_t)m, ni = iHost + (size_t)n + 2;
    if ((st = ensure(cv, &cv->d_in, &cv->h_in, &cv->in_cap, nd * sizeof(double) + ni * sizeof(int))) != VIO_OK) return st;
    double *hd = cv->h_in;
    int *hi = (int *)(cv->h_in + nd);

    // H_pp_schur at the current state: linearise first when the context says it holds none, or holds one of an older configuration
    if (cv->relinearize) {
        if ((st = vio_linearize(cv->ctx)) != VIO_OK) return fail(cv, st, "vio_linearize: %s", vio_last_error(cv->ctx));
        cv->relinearize = false;
    }
    st = vio_get_schur_system(cv->ctx, hd + oS, nullptr);
    if (st == VIO_ERR_BAD_ARG) {
        if ((st = vio_linearize(cv->ctx)) != VIO_OK) return fail(cv, st, "vio_linearize: %s", vio_last_error(cv->ctx));
        st = vio_get_schur_system(cv->ctx, hd + oS, nullptr);
    }
    if (st != VIO_OK) return fail(cv, st, "vio_get_schur_system: %s", vio_last_error(cv->ctx));
    double sb[NF * 9];
    if ((st = vio_get_window(cv->ctx, hd + oP, sb, hd + oE)) != VIO_OK) return fail(cv, st, "vio_get_window: %s", vio_last_error(cv->ctx));
    st = D == 1 ? vio_get_landmarks(cv->ctx, n, hd + oV) : vio_get_landmarks_xyz(cv->ctx, n, hd + oV);
    if (st != VIO_OK) return fail(cv, st, "vio_get_landmarks%s(n=%lld): %s", D == 1 ? "" : "_xyz", (long long)n, vio_last_error(cv->ctx));

    // variables kept: everything but the extrinsic (fixed, or not a variable of XYZ edges) and frame 0's pose (gauge)
    const int ext_fixed = D == 3 || cv->cfg.ext_fixed;
    int nk = 0;
    for (int v = 0; v < PD; ++v) {
        if (v < 6 && ext_fixed) continue;
        if (gauge == VIO_COV_GAUGE_FIX_OLDEST && v >= 6 && v < 12) continue;
        hi[iKeep + nk++] = v;
    }
    // CSR over the landmarks (stable: a landmark's observations keep the caller's order)
    int *off = hi + iOff, *ofr = hi + iOfr, *oh = hi + iHost;
    for (int64_t l = 0; l < n; ++l) oh[l] = -1;
    int mixed = -1;                         // a landmark whose observations name different host frames
    const bool ok = obs_csr(m, lm, n, off, [&](int64_t e, int l, int q) {
        ofr[q] = target[e];
        hd[oPj + 2 * (size_t)q] = pts_j[2 * e];
        hd[oPj + 2 * (size_t)q + 1] = pts_j[2 * e + 1];
        if (D == 1) {
            if (oh[l] < 0) {
                oh[l] = host[e];
                hd[oPi + 2 * (size_t)l] = pts_i[2 * e];
                hd[oPi + 2 * (size_t)l + 1] = pts_i[2 * e + 1];
            } else if (oh[l] != host[e]) {
                mixed = l;
                return false;
            }
        }
        return true;
    });
    if (!ok) return fail(cv, VIO_ERR_BAD_ARG, "landmark %d has observations with different host frames", mixed);
    if (D == 1)
        for (int64_t l = 0; l < n; ++l)
            if (oh[l] < 0) { oh[l] = 0; hd[oPi + 2 * (size_t)l] = 0; hd[oPi + 2 * (size_t)l + 1] = 0; }

    void *sp = nullptr;
    if ((st = vio_get_stream(cv->ctx, &sp)) != VIO_OK) return fail(cv, st, "vio_get_stream");
    cv->stream = (hipStream_t)sp;

    const size_t o_cov = 0, o_cc = PD * PD, o_out = o_cc + CD * CD, o_info = o_out + (size_t)n * D * D, nout = align8(o_info + (size_t)n * D * D);
    if ((st = ensure(cv, &cv->d_out, &cv->h_out, &cv->out_cap, nout * sizeof(double) + 8 * sizeof(int))) != VIO_OK) return st;
    int *d_status = (int *)(cv->d_out + nout), *h_status = (int *)(cv->h_out + nout);
    int *di = (int *)(cv->d_in + nd);

    if ((st = hip_ck(cv, hipMemcpyAsync(cv->d_in, cv->h_in, nd * sizeof(double) + ni * sizeof(int), hipMemcpyHostToDevice, cv->stream), "upload")) != VIO_OK) return st;
    // status[0]: failing pivot (-1: none); status[1]: smallest landmark without a positive definite information (NO_BAD_LM: none)
    if ((st = hip_ck(cv, hipMemsetAsync(d_status, 0xff, sizeof(int), cv->stream), "hipMemsetAsync")) != VIO_OK) return st;
    if ((st = hip_ck(cv, hipMemsetAsync(d_status + 1, 0x7f, sizeof(int), cv->stream), "hipMemsetAsync")) != VIO_OK) return st;
    const double t_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();

    if ((st = hip_ck(cv, hipEventRecord(cv->ev[0], cv->stream), "hipEventRecord")) != VIO_OK) return st;
    k_cov_pose<<<1, POSE_NT, 0, cv->stream>>>(cv->d_in + oS, di + iKeep, nk, cv->d_out + o_cov, cv->d_out + o_cc, d_status,
                                              (double *)(d_status + 2));
    if ((st = hip_ck(cv, hipGetLastError(), "k_cov_pose launch")) != VIO_OK) return st;
    if ((st = hip_ck(cv, hipEventRecord(cv->ev[1], cv->stream), "hipEventRecord")) != VIO_OK) return st;
    if (n > 0) {
        CovLmArgs a;
        a.cc = cv->d_out + o_cc; a.poses = cv->d_in + oP; a.ext = cv->d_in + oE; a.val = cv->d_in + oV; a.pts_i = cv->d_in + oPi;
        a.pts_j = cv->d_in + oPj; a.off = di + iOff; a.ofr = di + iOfr; a.ohost = di + iHost; a.n = (int)n;
        a.ext_free = !ext_fixed; a.loss_type = cv->cfg.loss_type; a.loss_delta = cv->cfg.loss_delta; a.sqrt_info = cv->cfg.reproj_sqrt_info;
        a.out = cv->d_out + o_out; a.info = cv->d_out + o_info; a.bad = d_status + 1;
        if (D == 1) k_cov_landmarks<1><<<(unsigned)((n + LmNT<1>::v - 1) / LmNT<1>::v), LmNT<1>::v, 0, cv->stream>>>(a);
        else k_cov_landmarks<3><<<(unsigned)((n + LmNT<3>::v - 1) / LmNT<3>::v), LmNT<3>::v, 0, cv->stream>>>(a);
        if ((st = hip_ck(cv, hipGetLastError(), "k_cov_landmarks launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(cv, hipEventRecord(cv->ev[2], cv->stream), "hipEventRecord")) != VIO_OK) return st;
    if ((st = hip_ck(cv, hipMemcpyAsync(cv->h_out, cv->d_out, nout * sizeof(double) + 8 * sizeof(int), hipMemcpyDeviceToHost, cv->stream), "read-back")) != VIO_OK) return st;
    if ((st = hip_ck(cv, hipStreamSynchronize(cv->stream), "hipStreamSynchronize")) != VIO_OK) return st;

    char nm[64];
    if (h_status[0] >= 0)
        return fail(cv, VIO_ERR_NOT_FINITE, "pose covariance: pivot %d (%s) of the reduced H_pp_schur is not positive and finite",
                    h_status[0], var_name(hi[iKeep + h_status[0]], nm, sizeof(nm)));
    if (n > 0 && h_status[1] != NO_BAD_LM)
        return fail(cv, VIO_ERR_NOT_FINITE, "landmark %d: its information is not positive definite and finite", h_status[1]);
    if (pose_cov) memcpy(pose_cov, cv->h_out + o_cov, sizeof(double) * PD * PD);
    if (lm_out && n > 0) memcpy(lm_out, cv->h_out + o_out, sizeof(double) * (size_t)n * D * D);
    cv->info.assign(cv->h_out + o_info, cv->h_out + o_info + (size_t)n * D * D);
    cv->last_n = n;
    cv->last_dim = D;
    cv->pivot_ratio = *(const double *)(h_status + 2);
    float ms1 = 0, ms2 = 0;
    if ((st = hip_ck(cv, hipEventElapsedTime(&ms1, cv->ev[0], cv->ev[1]), "hipEventElapsedTime")) != VIO_OK ||
        (st = hip_ck(cv, hipEventElapsedTime(&ms2, cv->ev[1], cv->ev[2]), "hipEventElapsedTime")) != VIO_OK) {
        for (double &t : cv->timing) t = NAN;   // (the outputs are written: only the timings are unknown)
        return VIO_OK;
    }
    cv->timing[0] = t_host;
    cv->timing[1] = ms1;
    cv->timing[2] = ms2;
    cv->timing[3] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    return VIO_OK;
}

extern "C" {

vio_status vio_cov_create(struct vio_ctx *ctx, const vio_config *cfg, vio_cov **out) {
    if (!out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    if (!ctx || !cfg) return VIO_ERR_BAD_ARG;
    if (cfg->shard_count > 1) return VIO_ERR_UNSUPPORTED;       // a shard holds part of the landmarks: no covariance of its own
    vio_cov *cv = new (std::nothrow) vio_cov;
    if (!cv) return VIO_ERR_BAD_ARG;
    cv->ctx = ctx;
    cv->cfg = *cfg;
    DeviceScope dev(cfg->device);
    if (!dev.ok) { delete cv; return VIO_ERR_HIP; }
    for (int k = 0; k < 3; ++k)
        if (hipEventCreate(&cv->ev[k]) != hipSuccess) { vio_cov_destroy(cv); return VIO_ERR_HIP; }
    *out = cv;
    return VIO_OK;
}

void vio_cov_destroy(vio_cov *cv) {
    if (!cv) return;
    DeviceScope dev(cv->cfg.device);
    if (cv->stream) hipStreamSynchronize(cv->stream);
    for (int k = 0; k < 3; ++k) if (cv->ev[k]) hipEventDestroy(cv->ev[k]);
    if (cv->d_in) hipFree(cv->d_in);
    if (cv->d_out) hipFree(cv->d_out);
    if (cv->h_in) hipHostFree(cv->h_in);
    if (cv->h_out) hipHostFree(cv->h_out);
    delete cv;
}

vio_status vio_cov_set_config(vio_cov *cv, const vio_config *cfg) {
    if (!cv || !cfg) return VIO_ERR_BAD_ARG;
    if (cfg->device != cv->cfg.device) return fail(cv, VIO_ERR_BAD_ARG, "device %d: the handle was made for device %d", cfg->device, cv->cfg.device);
    if (cfg->shard_count > 1) return fail(cv, VIO_ERR_UNSUPPORTED, "sharded context");
    const vio_config &o = cv->cfg;
    if (cfg->ext_fixed != o.ext_fixed || cfg->loss_type != o.loss_type || cfg->loss_delta != o.loss_delta ||
        cfg->reproj_sqrt_info != o.reproj_sqrt_info || memcmp(cfg->gravity, o.gravity, sizeof(o.gravity)) != 0 || cfg->item_policy != o.item_policy)
        cv->relinearize = true;
    cv->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_cov_pivot_ratio(vio_cov *cv, double *ratio) {
    if (!cv || !ratio) return VIO_ERR_BAD_ARG;
    if (cv->last_n < 0) return fail(cv, VIO_ERR_BAD_ARG, "no successful compute yet");
    *ratio = cv->pivot_ratio;
    return VIO_OK;
}

const char *vio_cov_last_error(const vio_cov *cv) { return cv ? cv->err : "null handle"; }

int32_t vio_cov_version(void) { return VIO_COV_VERSION; }

vio_status vio_cov_compute(vio_cov *cv, int32_t gauge, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                           const double *pts_i, const double *pts_j, int64_t n, double *pose_cov, double *lm_var) {
    if (!cv) return VIO_ERR_BAD_ARG;
    cv->err[0] = 0;
    return compute(cv, 1, gauge, m, lm, host, target, pts_i, pts_j, n, pose_cov, lm_var);
}

vio_status vio_cov_compute_xyz(vio_cov *cv, int32_t gauge, int64_t m, const int32_t *lm, const int32_t *frame, const double *pts,
                               int64_t n, double *pose_cov, double *lm_cov) {
    if (!cv) return VIO_ERR_BAD_ARG;
    cv->err[0] = 0;
    return compute(cv, 3, gauge, m, lm, nullptr, frame, nullptr, pts, n, pose_cov, lm_cov);
}

vio_status vio_cov_landmark_information(vio_cov *cv, int64_t n, double *info) {
    if (!cv) return VIO_ERR_BAD_ARG;
    if (cv->last_n < 0 || n != cv->last_n) return fail(cv, VIO_ERR_BAD_ARG, "no compute with n=%lld to read back", (long long)n);
    if (info && n > 0) memcpy(info, cv->info.data(), sizeof(double) * cv->info.size());
    return VIO_OK;
}

vio_status vio_cov_timing(vio_cov *cv, double *out4) {
    if (!cv || !out4) return VIO_ERR_BAD_ARG;
    memcpy(out4, cv->timing, sizeof(cv->timing));
    return VIO_OK;
}

}   // extern "C"
