// vio_flow_math.h — the per-sample arithmetic of the Lucas-Kanade tracker (include/vio_flow.h): BORDER_REFLECT_101, IsValidPatch, the
// bilinear value and Scharr gradient at a sample, and the 2 x 2 fullPivHouseholderQr solve.  Device code of csrc/vio_flow.hip; plain
// C++ otherwise, so that tests/test_flow_host_mirror.py can compile it for the host (with __device__ and __forceinline__ defined away)
// and hold it to tests/flow_reference.py bit for bit.  Include it with contraction off.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/vio_flow.h"

__device__ __forceinline__ int flow_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int flow_max(int a, int b) { return a > b ? a : b; }

// BORDER_REFLECT_101 for an index at most one image away, kept inside [0, n) whatever comes
__device__ __forceinline__ int refl(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return flow_min(flow_max(i, 0), n - 1);
}

__device__ __forceinline__ bool valid_patch(double x, double y, int w, int h, int hp) {
    return (double)hp <= x && x < (double)(w - hp) && (double)hp <= y && y < (double)(h - hp);
}

// The bilinear value at (x, y) of the level p (w x h), and with GRAD its Scharr gradient over VIO_FLOW_GRADIENT_DIVISOR.  (x, y) is
// inside a valid patch, so int(x), int(y) are pixels of the image; the clamps keep every load inside it whatever comes.
// pitch: the bytes between the level's rows (>= w).
template <bool GRAD> __device__ __forceinline__ void sample_pitched(const uint8_t *p, int pitch, int w, int h, double x, double y, double &val,
                                                                    double &jx, double &jy) {
    const int c0 = flow_min(flow_max((int)x, 0), w - 1), r0 = flow_min(flow_max((int)y, 0), h - 1);
    const int c1 = flow_min(c0 + 1, w - 1), r1 = flow_min(r0 + 1, h - 1);
    const double xx = x - (double)c0, yy = y - (double)r0;
    const double w00 = (1.0 - xx) * (1.0 - yy), w01 = xx * (1.0 - yy), w10 = (1.0 - xx) * yy, w11 = xx * yy;
    if (!GRAD) {
        const uint8_t *ra = p + (int64_t)r0 * pitch, *rb = p + (int64_t)r1 * pitch;
        val = ((w00 * (double)ra[c0] + w01 * (double)ra[c1]) + w10 * (double)rb[c0]) + w11 * (double)rb[c1];
        return;
    }
    // the 4 x 4 pixels around the sample; where x1 (y1) was clamped, the neighbours of both corners are the reflected column (row)
    const bool cx = c1 == c0, cy = r1 == r0;
    const int C[4] = {refl(c0 - 1, w), c0, c1, refl(c1 + 1, w)}, R[4] = {refl(r0 - 1, h), r0, r1, refl(r1 + 1, h)};
    int dxr[4][2], smr[4][2], v12[2][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint8_t *row = p + (int64_t)R[i] * pitch;
        const int v0 = row[C[0]], v1 = row[C[1]], v2 = row[C[2]], v3 = row[C[3]];
        const int L0 = v0, C0 = v1, R0 = cx ? v0 : v2, L1 = cx ? v0 : v1, C1 = v2, R1 = v3;
        dxr[i][0] = R0 - L0; dxr[i][1] = R1 - L1;
        smr[i][0] = 3 * L0 + 10 * C0 + 3 * R0; smr[i][1] = 3 * L1 + 10 * C1 + 3 * R1;
        if (i == 1) { v12[0][0] = v1; v12[0][1] = v2; }
        if (i == 2) { v12[1][0] = v1; v12[1][1] = v2; }
    }
    val = ((w00 * (double)v12[0][0] + w01 * (double)v12[0][1]) + w10 * (double)v12[1][0]) + w11 * (double)v12[1][1];
    int gx[2][2], gy[2][2];             // [corner row][corner column]
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        gx[0][b] = 3 * dxr[0][b] + 10 * dxr[1][b] + 3 * (cy ? dxr[0][b] : dxr[2][b]);
        gy[0][b] = (cy ? smr[0][b] : smr[2][b]) - smr[0][b];
        gx[1][b] = 3 * (cy ? dxr[0][b] : dxr[1][b]) + 10 * dxr[2][b] + 3 * dxr[3][b];
        gy[1][b] = smr[3][b] - (cy ? smr[0][b] : smr[1][b]);
    }
    jx = (((w00 * (double)gx[0][0] + w01 * (double)gx[0][1]) + w10 * (double)gx[1][0]) + w11 * (double)gx[1][1]) / VIO_FLOW_GRADIENT_DIVISOR;
    jy = (((w00 * (double)gy[0][0] + w01 * (double)gy[0][1]) + w10 * (double)gy[1][0]) + w11 * (double)gy[1][1]) / VIO_FLOW_GRADIENT_DIVISOR;
}

// the same for a level whose rows are tightly packed
template <bool GRAD> __device__ __forceinline__ void sample(const uint8_t *p, int w, int h, double x, double y, double &val, double &jx,
                                                            double &jy) {
    sample_pitched<GRAD>(p, w, w, h, x, y, val, jx, jy);
}

// H.fullPivHouseholderQr().solve(b) of Eigen 3.3 for the symmetric 2 x 2 H = [h00 h01; h01 h11] (include/vio_flow.h)
__device__ __forceinline__ void solve2(double h00, double h01, double h11, double b0, double b1, double &d0, double &d1) {
    const double prec = 2.0 * DBL_EPSILON;
    double m00 = h00, m01 = h01, m10 = h01, m11 = h11;
    int r = 0, c = 0;
    double best = fabs(m00);
    if (fabs(m10) > best) { r = 1; c = 0; best = fabs(m10); }
    if (fabs(m01) > best) { r = 0; c = 1; best = fabs(m01); }
    if (fabs(m11) > best) { r = 1; c = 1; best = fabs(m11); }
    const double biggest = best;
    d0 = 0.0; d1 = 0.0;
    if (best <= biggest * prec) return;
    if (r) { double t = m00; m00 = m10; m10 = t; t = m01; m01 = m11; m11 = t; }
    if (c) { double t = m00; m00 = m01; m01 = t; t = m10; m10 = m11; m11 = t; }
    const double tail2 = m10 * m10, c0 = m00;
    double tau = 0.0, beta = c0, ess = 0.0;
    if (!(tail2 <= DBL_MIN)) {
        beta = sqrt(c0 * c0 + tail2);
        if (c0 >= 0.0) beta = -beta;
        ess = m10 / (c0 - beta);
        tau = (beta - c0) / beta;
    }
    m00 = beta;
    double maxpivot = fabs(beta);
    if (tau != 0.0) {
        double tmp = ess * m11;
        tmp = tmp + m01;
        m01 = m01 - tau * tmp;
        m11 = m11 - (tau * ess) * tmp;
    }
    int nonzero = 2;
    if (fabs(m11) <= biggest * prec) nonzero = 1;
    else if (fabs(m11) > maxpivot) maxpivot = fabs(m11);
    const double thr = maxpivot * prec;
    int rank = 0;
    if (fabs(m00) > thr) rank += 1;
    if (nonzero == 2 && fabs(m11) > thr) rank += 1;
    if (rank == 0) return;
    double v0 = r ? b1 : b0, v1 = r ? b0 : b1;
    if (tau != 0.0) {
        double tmp = ess * v1;
        tmp = tmp + v0;
        v0 = v0 - tau * tmp;
        v1 = v1 - (tau * ess) * tmp;
    }
    if (rank == 2) {
        v1 = v1 / m11;
        v0 = v0 - v1 * m01;
        v0 = v0 / m00;
    } else {
        v0 = v0 / m00;
        v1 = 0.0;
    }
    d0 = c ? v1 : v0;
    d1 = c ? v0 : v1;
}

// The verdict of the forward-backward check (include/vio_flow_back.h) for a keypoint at (px, py) whose backward pass ended at
// (bx, by): d2 is formed whenever the pass ran; a lost pass is VIO_FLOW_FAIL_BACK_LOST, a comparison that is false (NaN included)
// VIO_FLOW_FAIL_BACK_FAR.  max_d2: the host's max_dist * max_dist.
__device__ __forceinline__ int flow_back_verdict(bool back_ok, float px, float py, float bx, float by, double max_d2, double &d2) {
    const double dx = (double)bx - (double)px, dy = (double)by - (double)py;
    d2 = dx * dx + dy * dy;
    if (!back_ok) return VIO_FLOW_FAIL_BACK_LOST;
    return d2 <= max_d2 ? VIO_OK : VIO_FLOW_FAIL_BACK_FAR;
}
