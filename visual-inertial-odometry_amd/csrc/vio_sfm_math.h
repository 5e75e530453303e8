// vio_sfm_math.h — the small dense device math libvio_sfm_hip (vio_sfm.hip), libvio_exrot_hip (vio_exrot.hip) and libvio_pnp_hip
// (vio_pnp.hip) share: one copy of the hash mixer, the fixed-sweep cyclic Jacobi, the SO(3) / quaternion helpers, the two-view
// triangulation, the normalised 8-point model, and the reprojection residual, its camera Jacobian, the 6 x 6 Cholesky solve and the
// trust-region radius rule of the PnP solves.  Device code only, one thread per call.  The including source sets `#pragma clang fp contract(off)` first: products
// and sums round as the host restatement's (tests/sfm_reference.py) do.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/vio_sfm.h"

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// cyclic Jacobi on the symmetric n x n matrix A (row-major, destroyed: its diagonal becomes the eigenvalues); V: the eigenvectors
// in columns
__device__ void jacobi(int n, double *A, double *V) {
    for (int i = 0; i < n * n; ++i) V[i] = 0.0;
    for (int i = 0; i < n; ++i) V[i * n + i] = 1.0;
    for (int sw = 0; sw < VIO_SFM_JACOBI_SWEEPS; ++sw)
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (apq == 0.0) t = 0.0;
                if (!isfinite(t)) t = 0.0;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double rp = A[p * n + k], rq = A[q * n + k];
                    A[p * n + k] = c * rp - s * rq;
                    A[q * n + k] = s * rp + c * rq;
                }
                for (int k = 0; k < n; ++k) {
                    const double cp = A[k * n + p], cq = A[k * n + q];
                    A[k * n + p] = c * cp - s * cq;
                    A[k * n + q] = s * cp + c * cq;
                    const double vp = V[k * n + p], vq = V[k * n + q];
                    V[k * n + p] = c * vp - s * vq;
                    V[k * n + q] = s * vp + c * vq;
                }
            }
}
__device__ int argmin_diag(int n, const double *A) {
    int k = 0;
    for (int i = 1; i < n; ++i)
        if (A[i * n + i] < A[k * n + k]) k = i;
    return k;
}

__device__ void exp_so3(const double *w, double *R) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(th2);
    double a, b;
    if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double kk = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
            R[3 * r + c] = ((r == c ? 1.0 : 0.0) + a * K[3 * r + c]) + b * kk;
        }
}
__device__ void rot_to_quat(const double *R, double *q) {     // (w, x, y, z): Eigen's Quaternion(Matrix3d)
    double t = R[0] + R[4] + R[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (R[7] - R[5]) * t; q[2] = (R[2] - R[6]) * t; q[3] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[3 * k + j] - R[3 * j + k]) * t;
        q[1 + j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[1 + k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
}
__device__ void quat_to_rot(const double *q, double *R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}
__device__ void mm3(const double *A, const double *B, double *C) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// GlobalSFM::triangulatePoint: cameras (R0, t0), (R1, t1) (rows of Pose = (R row, t)), points p0, p1
__device__ void triangulate(const double *R0, const double *t0, const double *R1, const double *t1, const double *p0, const double *p1,
                            double *X) {
    double D[16], N[16], V[16];
    for (int c = 0; c < 4; ++c) {
        const double a2 = c < 3 ? R0[6 + c] : t0[2], a0 = c < 3 ? R0[c] : t0[0], a1 = c < 3 ? R0[3 + c] : t0[1];
        const double b2 = c < 3 ? R1[6 + c] : t1[2], b0 = c < 3 ? R1[c] : t1[0], b1 = c < 3 ? R1[3 + c] : t1[1];
        D[c] = p0[0] * a2 - a0;
        D[4 + c] = p0[1] * a2 - a1;
        D[8 + c] = p1[0] * b2 - b0;
        D[12 + c] = p1[1] * b2 - b1;
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) N[4 * r + c] = ((D[r] * D[c] + D[4 + r] * D[4 + c]) + D[8 + r] * D[8 + c]) + D[12 + r] * D[12 + c];
    jacobi(4, N, V);
    const int k = argmin_diag(4, N);
    const double w = V[12 + k];
    X[0] = V[k] / w; X[1] = V[4 + k] / w; X[2] = V[8 + k] / w;
}

// the normalised 8-point model over the correspondences corr[idx[0 .. n-1]] (x_a, y_a, x_b, y_b): x_b^T F x_a = 0
__device__ void eight_point(const double *corr, const int *idx, int n, double *Fm) {
    double ca[2] = {0, 0}, cb[2] = {0, 0};
    for (int k = 0; k < n; ++k) {
        const double *p = corr + 4 * idx[k];
        ca[0] += p[0]; ca[1] += p[1]; cb[0] += p[2]; cb[1] += p[3];
    }
    for (int k = 0; k < 2; ++k) { ca[k] /= n; cb[k] /= n; }
    double ma = 0, mb = 0;
    for (int k = 0; k < n; ++k) {
        const double *p = corr + 4 * idx[k];
        const double ax = p[0] - ca[0], ay = p[1] - ca[1], bx = p[2] - cb[0], by = p[3] - cb[1];
        ma += sqrt(ax * ax + ay * ay);
        mb += sqrt(bx * bx + by * by);
    }
    const double sa = sqrt(2.0) / (ma / n), sb = sqrt(2.0) / (mb / n);
    double N[81], V[81];
    for (int i = 0; i < 81; ++i) N[i] = 0.0;
    for (int k = 0; k < n; ++k) {
        const double *p = corr + 4 * idx[k];
        const double x1 = (p[0] - ca[0]) * sa, y1 = (p[1] - ca[1]) * sa, x2 = (p[2] - cb[0]) * sb, y2 = (p[3] - cb[1]) * sb;
        const double r[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
        for (int i = 0; i < 9; ++i)
            for (int j = 0; j < 9; ++j) N[9 * i + j] += r[i] * r[j];
    }
    jacobi(9, N, V);
    int m = argmin_diag(9, N);
    double Fh[9];
    for (int i = 0; i < 9; ++i) Fh[i] = V[9 * i + m];
    double G[9], W[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) G[3 * r + c] = Fh[r] * Fh[c] + Fh[3 + r] * Fh[3 + c] + Fh[6 + r] * Fh[6 + c];
    jacobi(3, G, W);
    m = argmin_diag(3, G);
    const double v[3] = {W[m], W[3 + m], W[6 + m]};
    for (int r = 0; r < 3; ++r) {
        const double fv = Fh[3 * r] * v[0] + Fh[3 * r + 1] * v[1] + Fh[3 * r + 2] * v[2];
        for (int c = 0; c < 3; ++c) Fh[3 * r + c] = Fh[3 * r + c] - fv * v[c];
    }
    const double T1[9] = {sa, 0, -sa * ca[0], 0, sa, -sa * ca[1], 0, 0, 1.0};
    const double T2t[9] = {sb, 0, 0, 0, sb, 0, -sb * cb[0], -sb * cb[1], 1.0};
    double tmp[9];
    mm3(T2t, Fh, tmp);
    mm3(tmp, T1, Fm);
}

// ---- the same fit with the 9 x 9 matrices addressed through a stride (libvio_reject_hip: entry e of a lane's N and V at [e * S] of
// its LDS column, include/vio_reject.h) and the 3 x 3 work unrolled into registers.  The operations and their order are jacobi's and
// eight_point's above, so the bits are theirs.
template <int S> __device__ __forceinline__ void jacobi9_strided(double *A, double *V) {
    constexpr int n = 9;
    for (int i = 0; i < n * n; ++i) V[i * S] = 0.0;
    for (int i = 0; i < n; ++i) V[(i * n + i) * S] = 1.0;
    for (int sw = 0; sw < VIO_SFM_JACOBI_SWEEPS; ++sw)
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[(p * n + q) * S];
                const double theta = (A[(q * n + q) * S] - A[(p * n + p) * S]) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (apq == 0.0) t = 0.0;
                if (!isfinite(t)) t = 0.0;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < n; ++k) {
                    const double rp = A[(p * n + k) * S], rq = A[(q * n + k) * S];
                    A[(p * n + k) * S] = c * rp - s * rq;
                    A[(q * n + k) * S] = s * rp + c * rq;
                }
#pragma unroll
                for (int k = 0; k < n; ++k) {
                    const double cp = A[(k * n + p) * S], cq = A[(k * n + q) * S];
                    A[(k * n + p) * S] = c * cp - s * cq;
                    A[(k * n + q) * S] = s * cp + c * cq;
                    const double vp = V[(k * n + p) * S], vq = V[(k * n + q) * S];
                    V[(k * n + p) * S] = c * vp - s * vq;
                    V[(k * n + q) * S] = s * vp + c * vq;
                }
            }
}

// jacobi(3, A, V) with every index a constant: A and V stay in registers
__device__ __forceinline__ void jacobi3_unrolled(double *A, double *V) {
    constexpr int n = 3;
#pragma unroll
    for (int i = 0; i < n * n; ++i) V[i] = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) V[i * n + i] = 1.0;
    for (int sw = 0; sw < VIO_SFM_JACOBI_SWEEPS; ++sw) {
#pragma unroll
        for (int p = 0; p < n - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (apq == 0.0) t = 0.0;
                if (!isfinite(t)) t = 0.0;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < n; ++k) {
                    const double rp = A[p * n + k], rq = A[q * n + k];
                    A[p * n + k] = c * rp - s * rq;
                    A[q * n + k] = s * rp + c * rq;
                }
#pragma unroll
                for (int k = 0; k < n; ++k) {
                    const double cp = A[k * n + p], cq = A[k * n + q];
                    A[k * n + p] = c * cp - s * cq;
                    A[k * n + q] = s * cp + c * cq;
                    const double vp = V[k * n + p], vq = V[k * n + q];
                    V[k * n + p] = c * vp - s * vq;
                    V[k * n + q] = s * vp + c * vq;
                }
            }
    }
}

// Hartley's statistics of eight_point: the centroids and the scales of the correspondences corr[idx[0 .. n-1]]
struct HartleyScale {
    double ca[2], cb[2], sa, sb;
};

// row k of the 8-point design matrix of a correspondence p under the scaling
__device__ __forceinline__ void eight_point_row(const double *p, const HartleyScale &h, double *r) {
    const double x1 = (p[0] - h.ca[0]) * h.sa, y1 = (p[1] - h.ca[1]) * h.sa, x2 = (p[2] - h.cb[0]) * h.sb, y2 = (p[3] - h.cb[1]) * h.sb;
    r[0] = x2 * x1; r[1] = x2 * y1; r[2] = x2; r[3] = y2 * x1; r[4] = y2 * y1; r[5] = y2; r[6] = x1; r[7] = y1; r[8] = 1.0;
}

// eight_point from the summed normal matrix on: N (destroyed) and V at stride S, the model to Fm
template <int S> __device__ __forceinline__ void eight_point_finish_strided(double *N, double *V, const HartleyScale &h, double *Fm) {
    jacobi9_strided<S>(N, V);
    int m = 0;
    for (int i = 1; i < 9; ++i)
        if (N[(i * 9 + i) * S] < N[(m * 9 + m) * S]) m = i;
    double Fh[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Fh[i] = V[(9 * i + m) * S];
    double G[9], W[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[3 * r + c] = Fh[r] * Fh[c] + Fh[3 + r] * Fh[3 + c] + Fh[6 + r] * Fh[6 + c];
    jacobi3_unrolled(G, W);
    int m3 = 0;                                             // argmin_diag(3, G)
    if (G[4] < G[0]) m3 = 1;
    if (G[8] < (m3 == 1 ? G[4] : G[0])) m3 = 2;
    double v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = m3 == 0 ? W[3 * c] : (m3 == 1 ? W[3 * c + 1] : W[3 * c + 2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double fv = Fh[3 * r] * v[0] + Fh[3 * r + 1] * v[1] + Fh[3 * r + 2] * v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) Fh[3 * r + c] = Fh[3 * r + c] - fv * v[c];
    }
    const double T1[9] = {h.sa, 0, -h.sa * h.ca[0], 0, h.sa, -h.sa * h.ca[1], 0, 0, 1.0};
    const double T2t[9] = {h.sb, 0, 0, 0, h.sb, 0, -h.sb * h.cb[0], -h.sb * h.cb[1], 1.0};
    double tmp[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) tmp[3 * r + c] = T2t[3 * r] * Fh[c] + T2t[3 * r + 1] * Fh[3 + c] + T2t[3 * r + 2] * Fh[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Fm[3 * r + c] = tmp[3 * r] * T1[c] + tmp[3 * r + 1] * T1[3 + c] + tmp[3 * r + 2] * T1[6 + c];
}

// eight_point(corr, idx, 8, Fm) of one thread with N and V at stride S
template <int S> __device__ __forceinline__ void eight_point8_strided(const double *corr, const int *idx, double *N, double *V, double *Fm) {
    constexpr int n = 8;
    HartleyScale h;
    h.ca[0] = 0; h.ca[1] = 0; h.cb[0] = 0; h.cb[1] = 0;
#pragma unroll
    for (int k = 0; k < n; ++k) {
        const double *p = corr + 4 * idx[k];
        h.ca[0] += p[0]; h.ca[1] += p[1]; h.cb[0] += p[2]; h.cb[1] += p[3];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) { h.ca[k] /= n; h.cb[k] /= n; }
    double ma = 0, mb = 0;
#pragma unroll
    for (int k = 0; k < n; ++k) {
        const double *p = corr + 4 * idx[k];
        const double ax = p[0] - h.ca[0], ay = p[1] - h.ca[1], bx = p[2] - h.cb[0], by = p[3] - h.cb[1];
        ma += sqrt(ax * ax + ay * ay);
        mb += sqrt(bx * bx + by * by);
    }
    h.sa = sqrt(2.0) / (ma / n); h.sb = sqrt(2.0) / (mb / n);
    for (int i = 0; i < 81; ++i) N[i * S] = 0.0;
#pragma unroll
    for (int k = 0; k < n; ++k) {
        double r[9];
        eight_point_row(corr + 4 * idx[k], h, r);
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j) N[(9 * i + j) * S] += r[i] * r[j];
    }
    eight_point_finish_strided<S>(N, V, h, Fm);
}

__device__ __forceinline__ double epipolar_error(const double *F, const double *p) {
    const double ax = p[0], ay = p[1], bx = p[2], by = p[3];
    const double A = F[0] * ax + F[1] * ay + F[2], B = F[3] * ax + F[4] * ay + F[5], C = F[6] * ax + F[7] * ay + F[8];
    const double d2 = bx * A + by * B + C, s2 = 1.0 / (A * A + B * B);
    const double A1 = F[0] * bx + F[3] * by + F[6], B1 = F[1] * bx + F[4] * by + F[7], C1 = F[2] * bx + F[5] * by + F[8];
    const double d1 = ax * A1 + ay * B1 + C1, s1 = 1.0 / (A1 * A1 + B1 * B1);
    return fmax(d1 * d1 * s1, d2 * d2 * s2);
}

// Ceres' trust-region rule of both Levenberg-Marquardt solves (include/vio_sfm.h) and of libvio_pnp_hip's (include/vio_pnp.h)
constexpr double LM_RADIUS_MAX = 1e16, LM_RADIUS_MIN = 1e-32, LM_MIN_RHO = 1e-3, LM_DIAG_MIN = 1e-6, LM_DIAG_MAX = 1e32;

// normalised reprojection residual of point X in camera (R, t), the camera point and R X
__device__ __forceinline__ void residual(const double *R, const double *t, const double *X, const double *p, double *r, double *Xc,
                                         double *RX) {
    for (int k = 0; k < 3; ++k) {
        RX[k] = (R[3 * k] * X[0] + R[3 * k + 1] * X[1]) + R[3 * k + 2] * X[2];
        Xc[k] = RX[k] + t[k];
    }
    r[0] = Xc[0] / Xc[2] - p[0];
    r[1] = Xc[1] / Xc[2] - p[1];
}
// Jc (2 x 6, row-major) over (left rotation increment, translation)
__device__ __forceinline__ void jac_cam(const double *Xc, const double *RX, double *Jc, double *Jpr) {
    const double iz = 1.0 / Xc[2];
    Jpr[0] = iz; Jpr[1] = 0.0; Jpr[2] = -Xc[0] * iz * iz;
    Jpr[3] = 0.0; Jpr[4] = iz; Jpr[5] = -Xc[1] * iz * iz;
    const double S[9] = {0.0, RX[2], -RX[1], -RX[2], 0.0, RX[0], RX[1], -RX[0], 0.0};
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 3; ++c) {
            Jc[6 * r + c] = (Jpr[3 * r] * S[c] + Jpr[3 * r + 1] * S[3 + c]) + Jpr[3 * r + 2] * S[6 + c];
            Jc[6 * r + 3 + c] = Jpr[3 * r + c];
        }
}

__device__ bool cholesky_solve6(double *A, const double *b, double *x) {     // lower Cholesky in place, one thread
    for (int j = 0; j < 6; ++j) {
        double d = 0.0;
        for (int k = 0; k < j; ++k) d += A[6 * j + k] * A[6 * j + k];
        d = A[6 * j + j] - d;
        if (!(d > 0.0)) return false;
        A[6 * j + j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double s = 0.0;
            for (int k = 0; k < j; ++k) s += A[6 * i + k] * A[6 * j + k];
            A[6 * i + j] = (A[6 * i + j] - s) / A[6 * j + j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double s = 0.0;
        for (int k = 0; k < i; ++k) s += A[6 * i + k] * y[k];
        y[i] = (b[i] - s) / A[6 * i + i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = 0.0;
        for (int k = i + 1; k < 6; ++k) s += A[6 * k + i] * x[k];
        x[i] = (y[i] - s) / A[6 * i + i];
    }
    return true;
}

__device__ __forceinline__ double lm_radius(double radius, double rho) {
    const double x = 2.0 * rho - 1.0;
    return fmin(radius / fmax(1.0 / 3.0, 1.0 - x * x * x), LM_RADIUS_MAX);
}
