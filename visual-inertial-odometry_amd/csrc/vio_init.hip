// vio_init.hip — libvio_init_hip.so: visual-inertial alignment of many windows in one call (include/vio_init.h).
//
//   k_init_gyro   one thread per window: solveGyroscopeBias (initial_aligment.cpp:3-37) — the F-1 terms J_bg^T J_bg and
//                 J_bg^T 2 (delta_q^-1 q_ij).vec() summed in interval order, then one 3 x 3 LDLT
//   k_init_align  one wavefront (one 64-thread workgroup) per window: LinearAlignment (:141-200), the four iterations of
//                 RefineGravity (:55-139), visualInitialAlign's state change (estimator.cpp:397-458).  Per solve:
//                   phase 1  lane i < F-1 builds interval i's tmp_A / tmp_b and writes the lower triangle of r_A = tmp_A^T tmp_A and
//                            r_b = tmp_A^T tmp_b into LDS
//                   phase 2  lane-strided over the packed lower triangle of A (and over b): each entry sums its intervals' terms in
//                            interval order, then A *= 1000 (RefineGravity: onto its previous, scaled value, kept in HBM scratch)
//                   phase 3  Eigen's LDLT in place in LDS (Cholesky/LDLT.h:291-400): the pivot by a wave argmax, the swaps and the
//                            column update lane-parallel, every dot in ascending order as vioo_ldlt_solve (oracle/vio_oracle.c) has it
//                   phase 4  the solve (:558-600): forward substitution column by column with x in registers (the order per row is
//                            the routine's), the back substitution row by row on every lane
// The dense systems are at most 3F + 4 = 100 wide; their packed lower triangle is 40.4 KB at F = 32 and 5.6 KB at F = 11.
// Contraction is off: products and sums round as the host restatement's (tests/init_reference.py) do.  No atomics; every sum has a
// fixed order, so repeated calls are bitwise identical and a window's result does not depend on its batch.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_init.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

constexpr int FREC = 13;        // per frame: R (9, row-major), T (3), is_key (1.0 / 0.0)
constexpr int IREC = 20;        // per interval: sum_dt, delta_p (3), delta_v (3), delta_q (4, xyzw), J(O_R, O_BG) (9, row-major)
constexpr int RAB = 65;         // per interval in LDS: lower triangle of r_A (at most 10 x 10: 55) and r_b (at most 10)
constexpr int ALIGN_NT = 64;    // one wavefront per window
constexpr int GYRO_NT = 64;     // windows per workgroup of k_init_gyro
constexpr int OREC = 22;        // per window: status, n_key, s, g (3), g_world (3), s_linear, g_linear (3), rot (9) at 0, 1, 2, 3, 6, 9, 10, 13
constexpr int OUT_STRIDE = OREC + VIO_INIT_X_STRIDE + VIO_INIT_POSE_STRIDE + VIO_INIT_SB_STRIDE;

struct InitWin {
    int32_t F, K;
    int64_t o_frame, o_pre;     // into the staged doubles
    int64_t o_scr;              // into the scratch: RefineGravity's A (packed lower, tri(3F+3)) and b (3F+3)
    double bg[3];
};

__host__ __device__ constexpr int tri(int n) { return n * (n + 1) / 2; }
__device__ __forceinline__ int pidx(int i, int j) { return i * (i + 1) / 2 + j; }       // packed lower, j <= i

// ---------------------------------------------------------------------------------------------------------
// small dense helpers, in Eigen's evaluation order (3-term sums left to right)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mTm(const double *A, const double *B, double *C) {      // C = A^T B, all 3 x 3 row-major
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[3 * a + b] = A[a] * B[b] + A[3 + a] * B[3 + b] + A[6 + a] * B[6 + b];
}
__device__ __forceinline__ void mm(const double *A, const double *B, double *C) {       // C = A B
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[3 * a + b] = A[3 * a] * B[b] + A[3 * a + 1] * B[3 + b] + A[3 * a + 2] * B[6 + b];
}
__device__ __forceinline__ void mv(const double *A, const double *v, double *o) {       // o = A v
    for (int a = 0; a < 3; ++a) o[a] = A[3 * a] * v[0] + A[3 * a + 1] * v[1] + A[3 * a + 2] * v[2];
}
__device__ __forceinline__ void mTv(const double *A, const double *v, double *o) {      // o = A^T v
    for (int a = 0; a < 3; ++a) o[a] = A[a] * v[0] + A[3 + a] * v[1] + A[6 + a] * v[2];
}
__device__ __forceinline__ double sqn3(const double *v) { return v[0] * v[0] + v[1] * v[1] + v[2] * v[2]; }
__device__ __forceinline__ void normalized3(const double *v, double *o) {               // MatrixBase::normalized (Dot.h:121-131)
    const double z = sqn3(v);
    if (z > 0) { const double r = sqrt(z); o[0] = v[0] / r; o[1] = v[1] / r; o[2] = v[2] / r; }
    else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
}
// Quaterniond(Matrix3d) (Quaternion.h:747-784), out xyzw
__device__ void quat_from_mat(const double *m, double *q) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        double v[3];
        v[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        v[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        v[k] = (m[3 * k + i] + m[3 * i + k]) * t;
        q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
    }
}
// QuaternionBase::toRotationMatrix (Quaternion.h:530-562), q xyzw
__device__ void quat_to_mat(const double *q, double *R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// Eigen::Matrix<double,3,2> column-pivoting Householder QR's Q, column 2 (ColPivHouseholderQR.h:480-575, Householder.h:43-155,
// HouseholderSequence.h evalTo): the null vector JacobiSVD<Matrix<double,2,3>>(m, ComputeFullV).matrixV().col(2) returns for
// m = [v0^T; v1^T] (its 2 x 2 Jacobi sweeps and the sort touch columns 0 and 1 only)
__device__ void householder(double c0, const double *tail, int nt, double &tau, double &beta, double *ess) {
    double tsq = 0;
    for (int k = 0; k < nt; ++k) tsq = (k == 0) ? tail[0] * tail[0] : tsq + tail[k] * tail[k];
    if (tsq <= DBL_MIN) { tau = 0; beta = c0; for (int k = 0; k < nt; ++k) ess[k] = 0; return; }
    beta = sqrt(c0 * c0 + tsq);
    if (c0 >= 0) beta = -beta;
    for (int k = 0; k < nt; ++k) ess[k] = tail[k] / (c0 - beta);
    tau = (beta - c0) / beta;
}
__device__ void null_axis(const double *v0, const double *v1, double *axis) {
    double scale = 0;
    for (int k = 0; k < 3; ++k) { scale = fmax(scale, fabs(v0[k])); scale = fmax(scale, fabs(v1[k])); }      // cwiseAbs().maxCoeff()
    if (scale == 0) scale = 1;
    double c0[3], c1[3];                               // columns of (m / scale)^T
    for (int k = 0; k < 3; ++k) { c0[k] = v0[k] / scale; c1[k] = v1[k] / scale; }
    const double n0 = sqrt(sqn3(c0)), n1 = sqrt(sqn3(c1));
    if (n1 > n0) for (int k = 0; k < 3; ++k) { const double t = c0[k]; c0[k] = c1[k]; c1[k] = t; }       // maxCoeff: the first maximum
    double tau0, beta0, e0[2];
    householder(c0[0], c0 + 1, 2, tau0, beta0, e0);
    if (tau0 != 0) {                                   // applyHouseholderOnTheLeft on column 1
        const double t = e0[0] * c1[1] + e0[1] * c1[2] + c1[0];
        c1[0] -= tau0 * t; c1[1] -= (tau0 * e0[0]) * t; c1[2] -= (tau0 * e0[1]) * t;
    }
    double tau1, beta1, e1[1];
    householder(c1[1], c1 + 2, 1, tau1, beta1, e1);
    double d[3] = {0, 0, 1};                           // Q e2 = H0 (H1 e2)
    if (tau1 != 0) {
        const double t = e1[0] * d[2] + d[1];
        d[1] -= tau1 * t; d[2] -= (tau1 * e1[0]) * t;
    }
    if (tau0 != 0) {
        const double t = e0[0] * d[1] + e0[1] * d[2] + d[0];
        d[0] -= tau0 * t; d[1] -= (tau0 * e0[0]) * t; d[2] -= (tau0 * e0[1]) * t;
    }
    axis[0] = d[0]; axis[1] = d[1]; axis[2] = d[2];
}
// Quaterniond::FromTwoVectors(a, (0,0,1)).toRotationMatrix() (Quaternion.h:577-612)
__device__ void from_two_vectors_z(const double *a, double *R) {
    double v0[3];
    normalized3(a, v0);
    const double v1[3] = {0, 0, 1};
    double c = v1[0] * v0[0] + v1[1] * v0[1] + v1[2] * v0[2];
    double q[4];
    if (c < -1.0 + 1e-12) {                            // NumTraits<double>::dummy_precision(): nearly opposite
        c = fmax(c, -1.0);
        double axis[3];
        null_axis(v0, v1, axis);
        const double w2 = (1.0 + c) * 0.5;
        const double sv = sqrt(1.0 - w2);
        q[3] = sqrt(w2); q[0] = axis[0] * sv; q[1] = axis[1] * sv; q[2] = axis[2] * sv;
    } else {
        const double axis[3] = {v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]};
        const double s = sqrt((1.0 + c) * 2.0);
        const double invs = 1.0 / s;
        q[0] = axis[0] * invs; q[1] = axis[1] * invs; q[2] = axis[2] * invs; q[3] = s * 0.5;
    }
    quat_to_mat(q, R);
}
// R <- ypr2R(-R2ypr(M).x(), 0, 0) * R (utility.h:68-110): Ry and Rx are the identity, so ypr2R is Rz exactly
__device__ void yaw_zero(const double *M, double *R) {
    const double yaw = atan2(M[3], M[0]) / M_PI * 180.0;
    const double y = -yaw / 180.0 * M_PI;
    const double cy = cos(y), sy = sin(y);
    const double Rz[9] = {cy, -sy, 0, sy, cy, 0, 0, 0, 1};
    double o[9];
    mm(Rz, R, o);
    for (int k = 0; k < 9; ++k) R[k] = o[k];
}
__device__ __forceinline__ bool fin(double v) { return isfinite(v); }

// Eigen::LDLT<MatrixXd>(A).solve(b) on one thread, n <= 3 (the gyro system): vioo_ldlt_solve's operations, full row-major A
__device__ void ldlt_solve3(double *M, const double *b, double *x) {
    const int n = 3;
    int tr[3];
    double temp[3];
    bool zero_all = false;
    for (int k = 0; k < n && !zero_all; ++k) {
        int big = k; double bv = fabs(M[4 * k]);
        for (int i = k + 1; i < n; ++i) if (fabs(M[4 * i]) > bv) { bv = fabs(M[4 * i]); big = i; }
        tr[k] = big;
        if (k != big) {
            const int s = n - big - 1;
            for (int j = 0; j < k; ++j) { const double t = M[3 * k + j]; M[3 * k + j] = M[3 * big + j]; M[3 * big + j] = t; }
            for (int i = 0; i < s; ++i) { const int r = n - s + i; const double t = M[3 * r + k]; M[3 * r + k] = M[3 * r + big]; M[3 * r + big] = t; }
            { const double t = M[4 * k]; M[4 * k] = M[4 * big]; M[4 * big] = t; }
            for (int i = k + 1; i < big; ++i) { const double t = M[3 * i + k]; M[3 * i + k] = M[3 * big + i]; M[3 * big + i] = t; }
        }
        const int rs = n - k - 1;
        if (k > 0) {
            for (int j = 0; j < k; ++j) temp[j] = M[4 * j] * M[3 * k + j];
            double s = 0;
            for (int j = 0; j < k; ++j) s += M[3 * k + j] * temp[j];
            M[4 * k] -= s;
            for (int i = 0; i < rs; ++i) {
                double t = 0;
                for (int j = 0; j < k; ++j) t += M[3 * (k + 1 + i) + j] * temp[j];
                M[3 * (k + 1 + i) + k] -= t;
            }
        }
        const double akk = M[4 * k];
        const bool valid = fabs(akk) > 0;
        if (k == 0 && !valid) { for (int j = 0; j < n; ++j) tr[j] = j; zero_all = true; break; }
        if (rs > 0 && valid) for (int i = 0; i < rs; ++i) M[3 * (k + 1 + i) + k] /= akk;
    }
    for (int i = 0; i < n; ++i) x[i] = b[i];
    for (int k = 0; k < n; ++k) if (tr[k] != k) { const double t = x[k]; x[k] = x[tr[k]]; x[tr[k]] = t; }
    for (int i = 0; i < n; ++i) { double s = x[i]; for (int j = 0; j < i; ++j) s -= M[3 * i + j] * x[j]; x[i] = s; }
    const double tol = 1.0 / DBL_MAX;
    for (int i = 0; i < n; ++i) { if (fabs(M[4 * i]) > tol) x[i] /= M[4 * i]; else x[i] = 0; }
    for (int i = n - 1; i >= 0; --i) { double s = x[i]; for (int j = i + 1; j < n; ++j) s -= M[3 * j + i] * x[j]; x[i] = s; }
    for (int k = n - 1; k >= 0; --k) if (tr[k] != k) { const double t = x[k]; x[k] = x[tr[k]]; x[tr[k]] = t; }
}

// ---------------------------------------------------------------------------------------------------------
// k_init_gyro: solveGyroscopeBias, one thread per window
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GYRO_NT) void k_init_gyro(int count, const InitWin *__restrict__ wins, const double *__restrict__ dd,
                                                       double *__restrict__ out /*[count][4]: bg_out, status*/) {
    const int w = blockIdx.x * GYRO_NT + threadIdx.x;
    if (w >= count) return;
    const InitWin W = wins[w];
    const double *fr = dd + W.o_frame, *pr = dd + W.o_pre;
    double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    bool ok = fin(W.bg[0]) && fin(W.bg[1]) && fin(W.bg[2]);
    for (int i = 0; i + 1 < W.F; ++i) {
        const double *Ri = fr + FREC * i, *Rj = fr + FREC * (i + 1), *p = pr + IREC * i;
        for (int k = 0; k < 9; ++k) ok = ok && fin(Ri[k]) && fin(Rj[k]) && fin(p[11 + k]);
        for (int k = 0; k < 4; ++k) ok = ok && fin(p[7 + k]);
        double M[9], qij[4];
        mTm(Ri, Rj, M);                                            // frame_i.R^T frame_j.R
        quat_from_mat(M, qij);
        const double *dq = p + 7, *tA = p + 11;                    // jacobian.block<3,3>(O_R, O_BG)
        const double n2 = (dq[0] * dq[0] + dq[2] * dq[2]) + (dq[1] * dq[1] + dq[3] * dq[3]);   // squaredNorm, two lanes of packets
        double iq[4];
        if (n2 > 0) { iq[0] = -dq[0] / n2; iq[1] = -dq[1] / n2; iq[2] = -dq[2] / n2; iq[3] = dq[3] / n2; }
        else { iq[0] = iq[1] = iq[2] = iq[3] = 0; }
        // (delta_q.inverse() * q_ij).vec(), times 2
        const double tb[3] = {
            2 * (iq[3] * qij[0] + iq[0] * qij[3] + iq[1] * qij[2] - iq[2] * qij[1]),
            2 * (iq[3] * qij[1] + iq[1] * qij[3] + iq[2] * qij[0] - iq[0] * qij[2]),
            2 * (iq[3] * qij[2] + iq[2] * qij[3] + iq[0] * qij[1] - iq[1] * qij[0])};
        double AtA[9], Atb[3];
        mTm(tA, tA, AtA);
        mTv(tA, tb, Atb);
        for (int k = 0; k < 9; ++k) A[k] += AtA[k];
        for (int k = 0; k < 3; ++k) b[k] += Atb[k];
    }
    double d[3];
    ldlt_solve3(A, b, d);
    double o[3];
    for (int k = 0; k < 3; ++k) o[k] = W.bg[k] + d[k];
    ok = ok && fin(o[0]) && fin(o[1]) && fin(o[2]);
    for (int k = 0; k < 3; ++k) out[4 * w + k] = ok ? o[k] : NAN;
    out[4 * w + 3] = ok ? (double)VIO_OK : (double)VIO_ERR_NOT_FINITE;
}

// ---------------------------------------------------------------------------------------------------------
// k_init_align: one wavefront per window
// ---------------------------------------------------------------------------------------------------------
struct AlignArgs {
    const InitWin *wins;
    const double *dd;
    double *scr;
    double *out;
    double tic[3];
    double G;
    int nmax, fmax;
};

// (value, row) argmax over the lanes: the largest value, the lowest row among equals — the first maximum of a sequential scan
__device__ __forceinline__ void wave_argmax(double &v, int &i) {
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// Eigen's LDLT of the packed lower triangle L (n x n) in place, then x = A^-1 b; on entry x holds b.  All 64 lanes.
__device__ void ldlt_wave(int n, double *L, int *tr, double *temp, double *x, int lane) {
    bool zero_all = false;
    if (n <= 1) {
        if (lane == 0) tr[0] = 0;
    } else {
        for (int k = 0; k < n; ++k) {
            // pivot: the largest |diagonal| among rows k.. (not yet updated: LDLT.h:317-320), the first of equals
            double bv = -1.0;
            int bi = n;
            for (int i = k + lane; i < n; i += ALIGN_NT) {
                double v = fabs(L[pidx(i, i)]);
                if (!(v == v)) v = -1.0;
                if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
            }
            wave_argmax(bv, bi);
            const int big = (bi < n) ? bi : k;
            if (lane == 0) tr[k] = big;
            if (big != k) {                                // the four swaps touch disjoint entries: one lane-parallel pass
                for (int j = lane; j < k; j += ALIGN_NT) {
                    const double t = L[pidx(k, j)]; L[pidx(k, j)] = L[pidx(big, j)]; L[pidx(big, j)] = t;
                }
                for (int i = big + 1 + lane; i < n; i += ALIGN_NT) {
                    const double t = L[pidx(i, k)]; L[pidx(i, k)] = L[pidx(i, big)]; L[pidx(i, big)] = t;
                }
                if (lane == 0) { const double t = L[pidx(k, k)]; L[pidx(k, k)] = L[pidx(big, big)]; L[pidx(big, big)] = t; }
                for (int i = k + 1 + lane; i < big; i += ALIGN_NT) {
                    const double t = L[pidx(i, k)]; L[pidx(i, k)] = L[pidx(big, i)]; L[pidx(big, i)] = t;
                }
            }
            __syncthreads();
            const int rk = pidx(k, 0);
            double akk = L[rk + k];
            if (k > 0) {
                for (int j = lane; j < k; j += ALIGN_NT) temp[j] = L[pidx(j, j)] * L[rk + j];
                __syncthreads();
                double s = 0;
#pragma unroll 8
                for (int j = 0; j < k; ++j) s += L[rk + j] * temp[j];
                akk -= s;
            }
            const bool valid = fabs(akk) > 0;
            if (k == 0 && !valid) { zero_all = true; break; }
            for (int i = k + 1 + lane; i < n; i += ALIGN_NT) {
                const int ri = pidx(i, 0);
                double v = L[ri + k];
                if (k > 0) {
                    double t = 0;
#pragma unroll 8
                    for (int j = 0; j < k; ++j) t += L[ri + j] * temp[j];
                    v -= t;
                }
                if (valid) v /= akk;
                L[ri + k] = v;
            }
            if (lane == 0) L[rk + k] = akk;
            __syncthreads();
        }
    }
    if (zero_all) {
        for (int j = lane; j < n; j += ALIGN_NT) tr[j] = j;
        __syncthreads();
    }
    // dst = P b
    if (lane == 0)
        for (int k = 0; k < n; ++k) if (tr[k] != k) { const double t = x[k]; x[k] = x[tr[k]]; x[tr[k]] = t; }
    __syncthreads();
    // L^-1: row i takes x[i] -= L(i,j) x[j] for j = 0, 1, .. in turn: the routine's order; x in registers (rows lane, lane + 64)
    const int r0 = lane, r1 = lane + ALIGN_NT;
    double x0 = (r0 < n) ? x[r0] : 0.0, x1 = (r1 < n) ? x[r1] : 0.0;
    for (int j = 0; j + 1 < n; ++j) {
        const double xj = __shfl(j < ALIGN_NT ? x0 : x1, j & (ALIGN_NT - 1));
        if (r0 > j && r0 < n) x0 -= L[pidx(r0, j)] * xj;
        if (r1 > j && r1 < n) x1 -= L[pidx(r1, j)] * xj;
    }
    // D^+ (LDLT.h:575-586: 1 / highest() as the tolerance)
    const double tol = 1.0 / DBL_MAX;
    if (r0 < n) { const double d = L[pidx(r0, r0)]; x0 = (fabs(d) > tol) ? x0 / d : 0.0; }
    if (r1 < n) { const double d = L[pidx(r1, r1)]; x1 = (fabs(d) > tol) ? x1 / d : 0.0; }
    __syncthreads();
    if (r0 < n) x[r0] = x0;
    if (r1 < n) x[r1] = x1;
    __syncthreads();
    // L^-T, row by row from the bottom, each dot in ascending order: every lane the same values
    for (int i = n - 1; i >= 0; --i) {
        double s = x[i];
#pragma unroll 8
        for (int j = i + 1; j < n; ++j) s -= L[pidx(j, i)] * x[j];
        if (lane == 0) x[i] = s;
        __syncthreads();
    }
    // P^-1
    if (lane == 0)
        for (int k = n - 1; k >= 0; --k) if (tr[k] != k) { const double t = x[k]; x[k] = x[tr[k]]; x[tr[k]] = t; }
    __syncthreads();
}

// interval i's tmp_A (6 x nv, row-major) and tmp_b (6): LinearAlignment (:151-168) with lxly == nullptr, RefineGravity (:84-97) else
__device__ void interval_rows(const double *fi, const double *fj, const double *p, const double *tic, const double *lxly,
                              const double *g0, double *tA, double *tb) {
    const int nv = lxly ? 9 : 10;
    for (int k = 0; k < 6 * nv; ++k) tA[k] = 0;
    const double dt = p[0];
    const double *Ri = fi, *Rj = fj;
    double Rt2[9], Rt1[9], RiRj[9];                    // R_i^T dt dt / 2, R_i^T dt, R_i^T R_j
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) { Rt2[3 * a + b] = Ri[3 * b + a] * dt * dt / 2; Rt1[3 * a + b] = Ri[3 * b + a] * dt; }
    mTm(Ri, Rj, RiRj);
    double dT[3], RdT[3];
    for (int k = 0; k < 3; ++k) dT[k] = fj[9 + k] - fi[9 + k];
    mTv(Ri, dT, RdT);
    double RRt[3];
    mv(RiRj, tic, RRt);
    for (int a = 0; a < 3; ++a) {
        tA[nv * a + a] = -dt;                                        // -dt I
        tA[nv * (3 + a) + a] = -1.0;                                 // -I
        for (int b = 0; b < 3; ++b) tA[nv * (3 + a) + 3 + b] = RiRj[3 * a + b];
        if (!lxly) {
            for (int b = 0; b < 3; ++b) { tA[nv * a + 6 + b] = Rt2[3 * a + b]; tA[nv * (3 + a) + 6 + b] = Rt1[3 * a + b]; }
        } else {
            for (int b = 0; b < 2; ++b) {                            // (R^T dt dt / 2) lxly, (R^T dt) lxly
                tA[nv * a + 6 + b] = Rt2[3 * a] * lxly[b] + Rt2[3 * a + 1] * lxly[2 + b] + Rt2[3 * a + 2] * lxly[4 + b];
                tA[nv * (3 + a) + 6 + b] = Rt1[3 * a] * lxly[b] + Rt1[3 * a + 1] * lxly[2 + b] + Rt1[3 * a + 2] * lxly[4 + b];
            }
        }
        tA[nv * a + nv - 1] = RdT[a] / 100.0;
        tb[a] = p[1 + a] + RRt[a] - tic[a];                          // delta_p + R_i^T R_j TIC - TIC
        tb[3 + a] = p[4 + a];                                        // delta_v
    }
    if (lxly) {
        double u[3], v[3];
        mv(Rt2, g0, u);
        mv(Rt1, g0, v);
        for (int a = 0; a < 3; ++a) { tb[a] = tb[a] - u[a]; tb[3 + a] = tb[3 + a] - v[a]; }
    }
}

// TangentBasis (initial_aligment.cpp:40-54): lxly 3 x 2 row-major
__device__ void tangent_basis(const double *g0, double *lxly) {
    double a[3];
    normalized3(g0, a);
    double tmp[3] = {0, 0, 1};
    if (a[0] == tmp[0] && a[1] == tmp[1] && a[2] == tmp[2]) { tmp[0] = 1; tmp[2] = 0; }      // the reference's exact comparison
    const double at = a[0] * tmp[0] + a[1] * tmp[1] + a[2] * tmp[2];
    double bb[3], b[3];
    for (int k = 0; k < 3; ++k) bb[k] = tmp[k] - a[k] * at;
    normalized3(bb, b);
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    for (int k = 0; k < 3; ++k) { lxly[2 * k] = b[k]; lxly[2 * k + 1] = c[k]; }
}

// One solve of the alignment: m = 4 (LinearAlignment) or 3 (RefineGravity iteration `it`); x (n) ends in sx.
__device__ void align_solve(const AlignArgs &a, const InitWin &W, int m, int it, const double *lxly, const double *g0,
                            double *sL, double *sx, double *sT, double *sR, int *sTr, int lane) {
    const int F = W.F, nv = 6 + m, n = 3 * F + m, nt = tri(n), base = 3 * F;
    const double *fr = a.dd + W.o_frame, *pr = a.dd + W.o_pre;
    // phase 1: interval i -> lane i
    if (lane + 1 < F) {
        double tA[60], tb[6];
        interval_rows(fr + FREC * lane, fr + FREC * (lane + 1), pr + IREC * lane, a.tic, m == 3 ? lxly : nullptr, g0, tA, tb);
        double *o = sR + RAB * lane;
        int e = 0;
        for (int r = 0; r < nv; ++r)
            for (int c = 0; c <= r; ++c) {                            // r_A = tmp_A^T (cov_inv = I) tmp_A
                double s = tA[r] * tA[c];
                for (int q = 1; q < 6; ++q) s += tA[nv * q + r] * tA[nv * q + c];
                o[e++] = s;
            }
        for (int r = 0; r < nv; ++r) {
            double s = tA[r] * tb[0];
            for (int q = 1; q < 6; ++q) s += tA[nv * q + r] * tb[q];
            o[55 + r] = s;
        }
    }
    __syncthreads();
    // phase 2: A += (the blocks of every interval, in interval order); A *= 1000 (:125-127, :171-173)
    double *pA = a.scr + W.o_scr, *pb = pA + tri(3 * F + 3);
    int r = 0, c = lane;
    while (c > r) { c -= r + 1; ++r; }
    for (int e = lane; e < nt; e += ALIGN_NT) {
        double s = (m == 3 && it > 0) ? pA[e] : 0.0;
        if (r < base) {                                               // A.block<6,6>(3i, 3i) += r_A.topLeftCorner<6,6>()
            const int ilo = (r >= 5) ? (r - 5 + 2) / 3 : 0, ihi = c / 3;
            for (int i = ilo; i <= ihi && i < F - 1; ++i) {
                const int rr = r - 3 * i, cc = c - 3 * i;
                if (rr < 6 && cc >= 0) s += sR[RAB * i + tri(rr) + cc];
            }
        } else if (c < base) {                                        // A.block<m,6>(n-m, 3i) += r_A.bottomLeftCorner<m,6>()
            const int ilo = (c >= 5) ? (c - 5 + 2) / 3 : 0, ihi = c / 3;
            for (int i = ilo; i <= ihi && i < F - 1; ++i) s += sR[RAB * i + tri(6 + r - base) + c - 3 * i];
        } else {                                                      // A.bottomRightCorner<m,m>() += r_A.bottomRightCorner<m,m>()
            for (int i = 0; i < F - 1; ++i) s += sR[RAB * i + tri(6 + r - base) + 6 + c - base];
        }
        s = s * 1000.0;
        if (m == 3) pA[e] = s;
        sL[e] = s;
        c += ALIGN_NT;
        while (c > r) { c -= r + 1; ++r; }
    }
    for (int q = lane; q < n; q += ALIGN_NT) {
        double s = (m == 3 && it > 0) ? pb[q] : 0.0;
        if (q < base) {                                               // b.segment<6>(3i) += r_b.head<6>()
            const int ilo = (q >= 5) ? (q - 5 + 2) / 3 : 0, ihi = q / 3;
            for (int i = ilo; i <= ihi && i < F - 1; ++i) s += sR[RAB * i + 55 + q - 3 * i];
        } else {
            for (int i = 0; i < F - 1; ++i) s += sR[RAB * i + 55 + 6 + q - base];
        }
        s = s * 1000.0;
        if (m == 3) pb[q] = s;
        sx[q] = s;
    }
    __syncthreads();
    ldlt_wave(n, sL, sTr, sT, sx, lane);
}

__global__ __launch_bounds__(ALIGN_NT) void k_init_align(AlignArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int w = blockIdx.x;
    const InitWin W = a.wins[w];
    const int F = W.F, K = W.K;
    double *sL = lds, *sx = sL + tri(a.nmax), *sT = sx + a.nmax, *sR = sT + a.nmax;
    int *sTr = (int *)(sR + RAB * (a.fmax - 1));
    double *o = a.out + (size_t)OUT_STRIDE * w;
    double *ox = o + OREC, *op = ox + VIO_INIT_X_STRIDE, *osb = op + VIO_INIT_POSE_STRIDE;
    const double *fr = a.dd + W.o_frame, *pr = a.dd + W.o_pre;
    const double G = a.G;

    // every output NaN to begin with (a window that does not succeed keeps them)
    for (int k = lane; k < OUT_STRIDE; k += ALIGN_NT) o[k] = NAN;
    __syncthreads();                                                  // (ordered before the stores below)
    // inputs finite?
    int bad = 0;
    for (int k = lane; k < FREC * F; k += ALIGN_NT) bad |= !fin(fr[k]);
    for (int k = lane; k < IREC * (F - 1); k += ALIGN_NT) bad |= !fin(pr[k]);
    if (lane < 3) bad |= !fin(a.tic[lane]) || !fin(W.bg[lane]);
    bad |= !fin(G);
    bad = __syncthreads_or(bad);
    int status = VIO_OK;
    if (bad) status = VIO_ERR_NOT_FINITE;

    // ---- LinearAlignment (:141-200)
    double s_lin = NAN, g[3] = {NAN, NAN, NAN};
    if (status == VIO_OK) {
        align_solve(a, W, 4, 0, nullptr, nullptr, sL, sx, sT, sR, sTr, lane);
        const int n = 3 * F + 4;
        int nf = 0;
        for (int k = lane; k < n; k += ALIGN_NT) nf |= !fin(sx[k]);
        nf = __syncthreads_or(nf);
        s_lin = sx[n - 1] / 100.0;
        for (int k = 0; k < 3; ++k) g[k] = sx[n - 4 + k];
        if (nf) status = VIO_ERR_NOT_FINITE;
        else if (fabs(sqrt(sqn3(g)) - G) > 1.0) status = VIO_INIT_FAIL_GRAVITY;
        else if (s_lin < 0) status = VIO_INIT_FAIL_SCALE;
    }
    if (lane == 0 && status != VIO_ERR_NOT_FINITE) { o[9] = s_lin; o[10] = g[0]; o[11] = g[1]; o[12] = g[2]; }

    // ---- RefineGravity (:55-139).  Its A and b are zeroed once, before the loop: each iteration adds to the scaled previous one.
    double s = NAN;
    if (status == VIO_OK) {
        const int n = 3 * F + 3;
        double g0[3], gn[3];
        normalized3(g, gn);
        for (int k = 0; k < 3; ++k) g0[k] = gn[k] * G;
        int nf = 0;
        for (int it = 0; it < 4; ++it) {
            double lxly[6];
            tangent_basis(g0, lxly);
            align_solve(a, W, 3, it, lxly, g0, sL, sx, sT, sR, sTr, lane);
            for (int k = lane; k < n; k += ALIGN_NT) nf |= !fin(sx[k]);
            const double dg0 = sx[n - 3], dg1 = sx[n - 2];
            double t[3];
            for (int k = 0; k < 3; ++k) t[k] = g0[k] + (lxly[2 * k] * dg0 + lxly[2 * k + 1] * dg1);
            normalized3(t, gn);
            for (int k = 0; k < 3; ++k) g0[k] = gn[k] * G;
        }
        nf = __syncthreads_or(nf);
        for (int k = 0; k < 3; ++k) g[k] = g0[k];
        s = sx[n - 1] / 100.0;
        __syncthreads();
        if (lane == 0) sx[n - 1] = s;                                // (x.tail<1>())(0) = s
        __syncthreads();
        if (nf || !fin(s) || !fin(g[0]) || !fin(g[1]) || !fin(g[2])) status = VIO_ERR_NOT_FINITE;
        else {
            if (lane == 0) { o[2] = s; o[3] = g[0]; o[4] = g[1]; o[5] = g[2]; }
            for (int k = lane; k < n; k += ALIGN_NT) ox[k] = sx[k];
            if (s < 0) status = VIO_INIT_FAIL_REFINED_SCALE;
        }
    }

    // ---- visualInitialAlign's state change (estimator.cpp:397-458)
    if (status == VIO_OK) {
        // R0 = g2R(g) (utility.cpp:3-13), then the yaw of R0 Rs[0] removed
        double R0[9];
        double ng1[3];
        normalized3(g, ng1);                                          // g.normalized(), normalised again by FromTwoVectors
        from_two_vectors_z(ng1, R0);
        yaw_zero(R0, R0);
        int f0 = 0;
        while (fr[FREC * f0 + 12] == 0.0) ++f0;                      // Headers[0]
        double M[9];
        mm(R0, fr + FREC * f0, M);
        yaw_zero(M, R0);
        double gw[3];
        mv(R0, g, gw);
        // keyframe kv (lane kv): the kv-th frame with is_key set
        if (lane < K) {
            int f = -1, seen = -1;
            while (seen < lane) { ++f; if (fr[FREC * f + 12] != 0.0) ++seen; }
            const double *Rf = fr + FREC * f, *R00 = fr + FREC * f0;
            double Rt[3], R0t[3], P[3], V[3];
            mv(Rf, a.tic, Rt);
            mv(R00, a.tic, R0t);
            for (int k = 0; k < 3; ++k) P[k] = (s * Rf[9 + k] - Rt[k]) - (s * R00[9 + k] - R0t[k]);
            mv(Rf, sx + 3 * lane, V);                                 // x.segment<3>(kv * 3): an all-frame index (the reference's)
            double Pw[3], Vw[3], Rw[9], q[4];
            mv(R0, P, Pw);
            mv(R0, V, Vw);
            mm(R0, Rf, Rw);
            quat_from_mat(Rw, q);
            for (int k = 0; k < 3; ++k) { op[7 * lane + k] = Pw[k]; osb[9 * lane + k] = Vw[k]; osb[9 * lane + 3 + k] = 0.0; osb[9 * lane + 6 + k] = W.bg[k]; }
            for (int k = 0; k < 4; ++k) op[7 * lane + 3 + k] = q[k];
        }
        if (lane == 0) {
            for (int k = 0; k < 3; ++k) o[6 + k] = gw[k];
            for (int k = 0; k < 9; ++k) o[13 + k] = R0[k];
        }
    }
    if (lane == 0) { o[0] = (double)status; o[1] = (double)K; }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_init {
    int device = 0;
    ErrText err = {0};
    Twin<char> staging;                                  // descriptors | doubles
    DevBuf<double> scr;
    Twin<double> out;
    StreamEvents<3> q;                                   // events: upload start, kernel start, kernel end
    double timing[3] = {NAN, NAN, NAN};
};

namespace {

// a failure after work was enqueued: wait for the stream first, so that no copy still reads the pinned staging buffer the next call fills
vio_status check_item(vio_init *h, int i, const vio_init_item &it, int &K) {
    if (it.n_frames < 2 || it.n_frames > VIO_INIT_MAX_FRAMES)
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: n_frames must be in [2, %d]", i, VIO_INIT_MAX_FRAMES);
    if (!it.R || !it.T || !it.pre) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: R, T and pre are required", i);
    K = 0;
    for (int f = 0; f < it.n_frames; ++f) K += it.is_key ? (it.is_key[f] != 0) : 1;
    if (K < 2) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: fewer than two keyframes", i);
    return VIO_OK;
}

// stage the windows: descriptors, then per window F frame records and F-1 interval records.  Returns the bytes staged.
vio_status stage(vio_init *h, int count, const vio_init_item *items, const double *bg, size_t &b_desc, size_t &bytes, int &fmax,
                 int64_t &scr) {
    std::vector<int> Ks((size_t)count);
    for (int i = 0; i < count; ++i) {
        const vio_status st = check_item(h, i, items[i], Ks[(size_t)i]);
        if (st != VIO_OK) return st;
    }
    b_desc = align256(sizeof(InitWin) * (size_t)count);
    int64_t nd = 0;
    scr = 0;
    fmax = 2;
    std::vector<InitWin> wins((size_t)count);
    for (int i = 0; i < count; ++i) {
        InitWin &w = wins[(size_t)i];
        std::memset(&w, 0, sizeof(w));
        w.F = items[i].n_frames; w.K = Ks[(size_t)i];
        w.o_frame = nd; nd += (int64_t)FREC * w.F;
        w.o_pre = nd; nd += (int64_t)IREC * (w.F - 1);
        w.o_scr = scr; scr += tri(3 * w.F + 3) + 3 * w.F + 3;
        for (int k = 0; k < 3; ++k) w.bg[k] = bg ? bg[3 * i + k] : 0.0;
        if (w.F > fmax) fmax = w.F;
    }
    bytes = b_desc + sizeof(double) * (size_t)nd;
    const vio_status st = h->staging.ensure(h->err, bytes);
    if (st != VIO_OK) return st;
    std::memcpy(h->staging.h, wins.data(), sizeof(InitWin) * (size_t)count);
    double *hd = (double *)(h->staging.h + b_desc);
    for (int i = 0; i < count; ++i) {
        const vio_init_item &it = items[i];
        const InitWin &w = wins[(size_t)i];
        for (int f = 0; f < w.F; ++f) {
            double *o = hd + w.o_frame + (int64_t)FREC * f;
            std::memcpy(o, it.R + 9 * f, 9 * 8);
            std::memcpy(o + 9, it.T + 3 * f, 3 * 8);
            o[12] = (it.is_key ? it.is_key[f] != 0 : true) ? 1.0 : 0.0;
        }
        for (int k = 0; k + 1 < w.F; ++k) {
            const vio_preint &p = it.pre[k];
            double *o = hd + w.o_pre + (int64_t)IREC * k;
            o[0] = p.sum_dt;
            for (int c = 0; c < 3; ++c) { o[1 + c] = p.delta_p[c]; o[4 + c] = p.delta_v[c]; }
            for (int c = 0; c < 4; ++c) o[7 + c] = p.delta_q[c];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) o[11 + 3 * r + c] = p.jacobian[15 * (3 + r) + 12 + c];      // block<3,3>(O_R, O_BG)
        }
    }
    return VIO_OK;
}

void finish_timing(vio_init *h, std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1) {
    const float ms0 = elapsed_ms(h->q.ev[0], h->q.ev[1]), ms1 = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    const auto t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + ms0;
    h->timing[1] = ms1;
    h->timing[2] = std::chrono::duration<double, std::milli>(t2 - t0).count();
}

}  // namespace

extern "C" {

int32_t vio_init_version(void) { return VIO_INIT_VERSION; }

const char *vio_init_last_error(const vio_init *h) { return h ? h->err : "NULL handle"; }

vio_status vio_init_create(int32_t device, void *stream, vio_init **out) {
    return create_handle(device, stream, out, vio_init_destroy, [](vio_init *) {
        return hipFuncSetAttribute((const void *)k_init_align, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    });
}

void vio_init_destroy(vio_init *h) { destroy_handle(h); }

vio_status vio_init_timing(const vio_init *h, double *out3) {
    if (!h || !out3) return VIO_ERR_BAD_ARG;
    std::memcpy(out3, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_init_gyro_bias_batch(vio_init *h, int32_t count, const vio_init_item *items, const double *bg_in, double *bg_out,
                                    int32_t *status) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || (count > 0 && (!items || !bg_in || !bg_out)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_init_gyro_bias_batch: negative count or a NULL array");
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    size_t b_desc = 0, bytes = 0;
    int fmax = 0;
    int64_t scr = 0;
    DeviceScope dev(h->device);                     // before stage(): its buffers belong on the handle's device
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st = stage(h, count, items, bg_in, b_desc, bytes, fmax, scr);
    if (st != VIO_OK) return st;
    const size_t outb = sizeof(double) * 4 * (size_t)count;
    if ((st = h->out.ensure(h->err, outb)) != VIO_OK) return st;
    const auto t1 = std::chrono::steady_clock::now();
    (void)hipEventRecord(h->q.ev[0], h->q.stream);
    if (hipMemcpyAsync(h->staging.d, h->staging.h, bytes, hipMemcpyHostToDevice, h->q.stream) != hipSuccess)
        return fail_synced(h, "vio_init_gyro_bias_batch: upload failed");
    (void)hipEventRecord(h->q.ev[1], h->q.stream);
    hipLaunchKernelGGL(k_init_gyro, dim3((count + GYRO_NT - 1) / GYRO_NT), dim3(GYRO_NT), 0, h->q.stream, count,
                       (const InitWin *)h->staging.d, (const double *)(h->staging.d + b_desc), h->out.d);
    (void)hipEventRecord(h->q.ev[2], h->q.stream);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "vio_init_gyro_bias_batch: kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, outb, hipMemcpyDeviceToHost, h->q.stream) != hipSuccess ||
        hipStreamSynchronize(h->q.stream) != hipSuccess)
        return fail_synced(h, "vio_init_gyro_bias_batch: kernel or read-back failed");
    vio_status ret = VIO_OK;
    for (int i = 0; i < count; ++i) {
        const double *o = h->out.h + 4 * (size_t)i;
        for (int k = 0; k < 3; ++k) bg_out[3 * i + k] = o[k];
        const int32_t ws = (int32_t)o[3];
        if (status) status[i] = ws;
        if (ws != VIO_OK) {
            ret = VIO_ERR_NOT_FINITE;
            if (!h->err[0]) fail(h->err, ret, "window %d: non-finite input or result", i);
        }
    }
    finish_timing(h, t0, t1);
    return ret;
}

vio_status vio_init_align_batch(vio_init *h, int32_t count, const vio_init_item *items, const double *tic, double g_norm,
                                const double *bg, vio_init_result *res, double *x, double *poses, double *speed_bias) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || (count > 0 && (!items || !tic || !bg || !res)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_init_align_batch: negative count or a NULL array");
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    size_t b_desc = 0, bytes = 0;
    int fmax = 0;
    int64_t scr = 0;
    DeviceScope dev(h->device);                     // before stage(): its buffers belong on the handle's device
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st = stage(h, count, items, bg, b_desc, bytes, fmax, scr);
    if (st != VIO_OK) return st;
    const size_t outb = sizeof(double) * OUT_STRIDE * (size_t)count;
    if ((st = h->out.ensure(h->err, outb)) != VIO_OK || (st = h->scr.ensure(h->err, sizeof(double) * (size_t)scr)) != VIO_OK) return st;
    AlignArgs a;
    a.wins = (const InitWin *)h->staging.d;
    a.dd = (const double *)(h->staging.d + b_desc);
    a.scr = h->scr.d;
    a.out = h->out.d;
    for (int k = 0; k < 3; ++k) a.tic[k] = tic[k];
    a.G = g_norm;
    a.nmax = 3 * fmax + 4;
    a.fmax = fmax;
    const size_t lds = sizeof(double) * ((size_t)tri(a.nmax) + 2 * (size_t)a.nmax + (size_t)RAB * (fmax - 1)) + sizeof(int) * (size_t)a.nmax;
    const auto t1 = std::chrono::steady_clock::now();
    (void)hipEventRecord(h->q.ev[0], h->q.stream);
    if (hipMemcpyAsync(h->staging.d, h->staging.h, bytes, hipMemcpyHostToDevice, h->q.stream) != hipSuccess)
        return fail_synced(h, "vio_init_align_batch: upload failed");
    (void)hipEventRecord(h->q.ev[1], h->q.stream);
    hipLaunchKernelGGL(k_init_align, dim3(count), dim3(ALIGN_NT), lds, h->q.stream, a);
    (void)hipEventRecord(h->q.ev[2], h->q.stream);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "vio_init_align_batch: kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, outb, hipMemcpyDeviceToHost, h->q.stream) != hipSuccess ||
        hipStreamSynchronize(h->q.stream) != hipSuccess)
        return fail_synced(h, "vio_init_align_batch: kernel or read-back failed");
    vio_status ret = VIO_OK;
    for (int i = 0; i < count; ++i) {
        const double *o = h->out.h + (size_t)OUT_STRIDE * i;
        vio_init_result &r = res[i];
        r.status = (int32_t)o[0];
        r.n_key = (int32_t)o[1];
        r.s = o[2];
        for (int k = 0; k < 3; ++k) { r.g[k] = o[3 + k]; r.g_world[k] = o[6 + k]; r.g_linear[k] = o[10 + k]; }
        r.s_linear = o[9];
        for (int k = 0; k < 9; ++k) r.rot[k] = o[13 + k];
        const int F = items[i].n_frames, K = r.n_key;
        if (x) std::memcpy(x + (size_t)VIO_INIT_X_STRIDE * i, o + OREC, sizeof(double) * (3 * F + 3));
        if (poses) std::memcpy(poses + (size_t)VIO_INIT_POSE_STRIDE * i, o + OREC + VIO_INIT_X_STRIDE, sizeof(double) * 7 * K);
        if (speed_bias)
            std::memcpy(speed_bias + (size_t)VIO_INIT_SB_STRIDE * i, o + OREC + VIO_INIT_X_STRIDE + VIO_INIT_POSE_STRIDE, sizeof(double) * 9 * K);
        if (r.status == VIO_ERR_NOT_FINITE) {
            ret = VIO_ERR_NOT_FINITE;
            if (!h->err[0]) fail(h->err, ret, "window %d: non-finite input or result", i);
        }
    }
    finish_timing(h, t0, t1);
    return ret;
}

}  // extern "C"
