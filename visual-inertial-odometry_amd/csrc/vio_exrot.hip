// vio_exrot.hip — libvio_exrot_hip.so: camera-IMU extrinsic rotation calibration of many windows in one call (include/vio_exrot.h,
// DESIGN.md section 17).
//
//   k_exrot_pairs   one 256-thread workgroup per (window, consecutive frame pair): solveRelativeR.  The threads list the pair's
//                   correspondences in track order (thread t takes the t-th run of consecutive tracks, an integer prefix sum places
//                   the runs), form each point's scaled row of the 8-point design matrix, and 45 threads sum the upper triangle of the
//                   9 x 9 normal matrix, each entry over the correspondences in track order.  One lane runs the Jacobi on the matrix
//                   in LDS, the rank-2 step and decomposeE; the four triangulation tests run thread per (candidate, correspondence)
//                   into integer LDS counters.
//   k_exrot_solve   one wavefront per window: lane k prepares pair k (the quaternions, D = L(q_c) - R(q_imu), D^T D) into LDS, then
//                   lane 0 runs the recursion over the pairs: Rc_g from the ric of the step before, the Huber weight, the 4 x 4 normal
//                   matrix, its Jacobi, the new ric, the gate.
// Summation orders (none depends on the workgroup's size): the centroid, mean-distance and normal-matrix sums each have one
// accumulator that takes the correspondences in track order; the 4 x 4 normal matrix is N_k = N_(k-1) + h_k^2 D_k^T D_k, which is
// the sum over the pairs in pair order restarted at every step, bit for bit (an old pair's weight never changes).
// Contraction is off: products and sums round as the host restatement's (tests/exrot_reference.py) do.  No floating-point atomics, so
// repeated calls are bitwise identical and a window's result does not depend on its batch.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_exrot.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_sfm_math.h"

constexpr int NT = 256;                 // k_exrot_pairs
constexpr int NW = 64;                  // k_exrot_solve: one wavefront
constexpr int MAXP = VIO_EXROT_MAX_FRAMES - 1;
constexpr int PO = 8;                   // per pair: status, n_corres, front (4), choice, det_flip
constexpr int SO = 17;                  // per step: q (4), R (9), sigma (3), huber
constexpr int WO = 15;                  // per window: status, step, q (4), R (9)
constexpr int PAIR_LDS = 23;            // per pair in k_exrot_solve: q_c (4), upper D^T D (10), Rimu (9)
static_assert(MAXP <= NW - 1, "k_exrot_solve prepares one pair per lane");

struct ExWin {
    int32_t F, nt, nobs, pad;
    int64_t o_int;      // staged int32: start_frame [nt], obs_offset [nt + 1]
    int64_t o_pts;      // staged doubles: pts [nobs][2]
    int64_t o_dq;       // staged doubles: delta_q [F - 1][4]
    int64_t o_pair;     // the window's first row in the per-pair and per-step arrays
};

struct ExPair {
    int32_t win, k;     // frames (k, k + 1) of window win
    int32_t cap, pad;   // the pair's correspondences, counted on the host: the size of its scratch
    int64_t o_scr;      // double scratch: corr 4 cap | rows 9 cap
};

struct ExArgs {
    const ExWin *wins;
    const ExPair *pairs;
    const int32_t *ints;
    const double *dd;
    double *scr;
    double *pout;       // [pairs][PO]
    double *rc;         // [pairs][9]
    double *sout;       // [pairs][SO]
    double *wout;       // [count][WO]
    int32_t min_frames;
    double min_sigma, huber_deg;
};

// ---------------------------------------------------------------------------------------------------------
// k_exrot_pairs
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_exrot_pairs(ExArgs a) {
    const ExPair P = a.pairs[blockIdx.x];
    const ExWin W = a.wins[P.win];
    const int tid = threadIdx.x, nt = W.nt, f0 = P.k;
    const int32_t *sf = a.ints + W.o_int, *off = sf + nt;
    const double *pts = a.dd + W.o_pts;
    double *corr = a.scr + P.o_scr, *rows = corr + 4 * (int64_t)P.cap;
    double *o = a.pout + (int64_t)PO * blockIdx.x, *orc = a.rc + 9 * (int64_t)blockIdx.x;

    __shared__ int s_cnt[NT];
    __shared__ double s_N[81], s_V[81];
    __shared__ double s_h[6];           // centroids of a and b, scales of a and b
    __shared__ double s_R[2][9], s_t[3];
    __shared__ int s_i[6];              // front (4), det_flip, finite

    int bad = 0;
    for (int k = tid; k < 2 * W.nobs; k += NT) bad |= !isfinite(pts[k]);
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid < 9) orc[tid] = NAN;
        if (tid < PO) o[tid] = tid == 0 ? (double)VIO_ERR_NOT_FINITE : 0.0;
        return;
    }
    // the correspondences in track order: thread t takes tracks [t C, (t + 1) C)
    const int C = (nt + NT - 1) / NT, j0 = tid * C, j1 = min(nt, j0 + C);
    int mine = 0;
    for (int j = j0; j < j1; ++j) mine += sf[j] <= f0 && sf[j] + (off[j + 1] - off[j]) - 1 >= f0 + 1;
    s_cnt[tid] = mine;
    if (tid < 6) s_i[tid] = 0;
    __syncthreads();
    int m = 0, n = 0;
    for (int t = 0; t < NT; ++t) {
        if (t == tid) m = n;
        n += s_cnt[t];
    }
    for (int j = j0; j < j1; ++j)
        if (sf[j] <= f0 && sf[j] + (off[j + 1] - off[j]) - 1 >= f0 + 1) {
            const double *p0 = pts + 2 * (int64_t)(off[j] + f0 - sf[j]);
            if (m < P.cap) { corr[4 * m] = p0[0]; corr[4 * m + 1] = p0[1]; corr[4 * m + 2] = p0[2]; corr[4 * m + 3] = p0[3]; }
            ++m;
        }
    if (n < VIO_EXROT_MIN_CORRES || n > P.cap) {        // (n > cap cannot happen: the host counts with the same test)
        if (tid < 9) orc[tid] = tid % 4 == 0 ? 1.0 : 0.0;
        if (tid < PO) o[tid] = tid == 1 ? (double)n : 0.0;
        return;
    }
    __syncthreads();
    // Hartley scaling: the sums of eight_point, each in track order
    if (tid < 4) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += corr[4 * k + tid];
        s_h[tid] = s / n;
    }
    __syncthreads();
    if (tid < 2) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) {
            const double dx = corr[4 * k + 2 * tid] - s_h[2 * tid], dy = corr[4 * k + 2 * tid + 1] - s_h[2 * tid + 1];
            s += sqrt(dx * dx + dy * dy);
        }
        s_h[4 + tid] = sqrt(2.0) / (s / n);
    }
    __syncthreads();
    for (int k = tid; k < n; k += NT) {
        const double *p = corr + 4 * k;
        const double x1 = (p[0] - s_h[0]) * s_h[4], y1 = (p[1] - s_h[1]) * s_h[4], x2 = (p[2] - s_h[2]) * s_h[5], y2 = (p[3] - s_h[3]) * s_h[5];
        double *r = rows + 9 * (int64_t)k;
        r[0] = x2 * x1; r[1] = x2 * y1; r[2] = x2; r[3] = y2 * x1; r[4] = y2 * y1; r[5] = y2; r[6] = x1; r[7] = y1; r[8] = 1.0;
    }
    __syncthreads();
    if (tid < 45) {                     // entry (i, j), i <= j, of the normal matrix
        int i = 0, e = tid;
        while (e >= 9 - i) { e -= 9 - i; ++i; }
        const int j = i + e;
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += rows[9 * (int64_t)k + i] * rows[9 * (int64_t)k + j];
        s_N[9 * i + j] = s;
        s_N[9 * j + i] = s;
    }
    __syncthreads();
    if (tid == 0) {
        jacobi(9, s_N, s_V);            // (in LDS: no per-lane copy of the two 9 x 9 matrices)
        int mi = argmin_diag(9, s_N);
        double Fh[9];
        for (int i = 0; i < 9; ++i) Fh[i] = s_V[9 * i + mi];
        double G[9], Wv[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) G[3 * r + c] = Fh[r] * Fh[c] + Fh[3 + r] * Fh[3 + c] + Fh[6 + r] * Fh[6 + c];
        jacobi(3, G, Wv);
        mi = argmin_diag(3, G);
        const double v[3] = {Wv[mi], Wv[3 + mi], Wv[6 + mi]};
        for (int r = 0; r < 3; ++r) {
            const double fv = Fh[3 * r] * v[0] + Fh[3 * r + 1] * v[1] + Fh[3 * r + 2] * v[2];
            for (int c = 0; c < 3; ++c) Fh[3 * r + c] = Fh[3 * r + c] - fv * v[c];
        }
        const double sa = s_h[4], sb = s_h[5];
        const double T1[9] = {sa, 0, -sa * s_h[0], 0, sa, -sa * s_h[1], 0, 0, 1.0};
        const double T2t[9] = {sb, 0, 0, 0, sb, 0, -sb * s_h[2], -sb * s_h[3], 1.0};
        double tmp[9], E[9];
        mm3(T2t, Fh, tmp);
        mm3(tmp, T1, E);
        // decomposeE: E = U diag V^T from the eigenvectors of E^T E (no sign fix of V), R1 = U W V^T, R2 = U W^T V^T, t = +-u2
        double V[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) G[3 * r + c] = E[r] * E[c] + E[3 + r] * E[3 + c] + E[6 + r] * E[6 + c];
        jacobi(3, G, V);
        int ord[3] = {0, 1, 2};
        for (int x = 1; x < 3; ++x)                     // stable, descending
            for (int y = x; y > 0 && G[4 * ord[y]] > G[4 * ord[y - 1]]; --y) { const int t = ord[y]; ord[y] = ord[y - 1]; ord[y - 1] = t; }
        double Vs[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Vs[3 * r + c] = V[3 * r + ord[c]];
        double u0[3], u1[3], u2[3];
        const double s0 = sqrt(G[4 * ord[0]]), s1 = sqrt(G[4 * ord[1]]);
        for (int r = 0; r < 3; ++r) {
            u0[r] = (E[3 * r] * Vs[0] + E[3 * r + 1] * Vs[3] + E[3 * r + 2] * Vs[6]) / s0;
            u1[r] = (E[3 * r] * Vs[1] + E[3 * r + 1] * Vs[4] + E[3 * r + 2] * Vs[7]) / s1;
        }
        const double d01 = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
        for (int r = 0; r < 3; ++r) u1[r] = u1[r] - d01 * u0[r];
        const double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
        for (int r = 0; r < 3; ++r) u1[r] = u1[r] / n1;
        u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
        double R1[9], R2[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                // U W = (u1, -u0, u2), U W^T = (-u1, u0, u2), times V^T
                R1[3 * r + c] = (u1[r] * Vs[3 * c] + (-u0[r]) * Vs[3 * c + 1]) + u2[r] * Vs[3 * c + 2];
                R2[3 * r + c] = ((-u1[r]) * Vs[3 * c] + u0[r] * Vs[3 * c + 1]) + u2[r] * Vs[3 * c + 2];
            }
        const double det = R1[0] * (R1[4] * R1[8] - R1[5] * R1[7]) - R1[1] * (R1[3] * R1[8] - R1[5] * R1[6]) +
                           R1[2] * (R1[3] * R1[7] - R1[4] * R1[6]);
        const bool flip = det + 1.0 < 1e-9;             // E = -E: its SVD is (-U, S, V)
        int fin = 1;
        for (int k = 0; k < 9; ++k) {
            s_R[0][k] = flip ? -R1[k] : R1[k];
            s_R[1][k] = flip ? -R2[k] : R2[k];
            fin &= isfinite(R1[k]) != 0 && isfinite(R2[k]) != 0;
        }
        for (int k = 0; k < 3; ++k) { s_t[k] = flip ? -u2[k] : u2[k]; fin &= isfinite(u2[k]) != 0; }
        s_i[4] = flip;
        s_i[5] = fin;
    }
    __syncthreads();
    if (!s_i[5]) {
        if (tid < 9) orc[tid] = NAN;
        if (tid < PO) o[tid] = tid == 0 ? (double)VIO_ERR_NOT_FINITE : (tid == 1 ? (double)n : 0.0);
        return;
    }
    {
        const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z3[3] = {0, 0, 0};
        for (int e = tid; e < 4 * n; e += NT) {
            const int c = e / n, k = e % n;
            const double *R = s_R[c >> 1];
            const double sg = (c & 1) ? -1.0 : 1.0;
            const double t[3] = {sg * s_t[0], sg * s_t[1], sg * s_t[2]};
            double X[3];
            triangulate(I3, z3, R, t, corr + 4 * k, corr + 4 * k + 2, X);
            const double z1 = X[2], z2 = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2]) + t[2];
            if (z1 > 0 && z2 > 0) atomicAdd(&s_i[c], 1);
        }
    }
    __syncthreads();
    const int r1 = max(s_i[0], s_i[1]), r2 = max(s_i[2], s_i[3]);
    const int choice = r1 > r2 ? 1 : 2;
    if (tid < 9) orc[tid] = s_R[choice - 1][3 * (tid % 3) + tid / 3];       // transposed
    if (tid == 0) {
        o[0] = VIO_OK; o[1] = n;
        for (int c = 0; c < 4; ++c) o[2 + c] = s_i[c];
        o[6] = choice; o[7] = s_i[4];
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_exrot_solve
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NW) void k_exrot_solve(ExArgs a) {
    const ExWin W = a.wins[blockIdx.x];
    const int lane = threadIdx.x, np = W.F - 1;
    const double *rc = a.rc + 9 * W.o_pair, *dq = a.dd + W.o_dq;
    double *so = a.sout + (int64_t)SO * W.o_pair, *wo = a.wout + (int64_t)WO * blockIdx.x;
    __shared__ double s_p[MAXP][PAIR_LDS];

    int bad = 0;
    if (lane < np) {
        for (int k = 0; k < 9; ++k) bad |= !isfinite(rc[9 * lane + k]);
        for (int k = 0; k < 4; ++k) bad |= !isfinite(dq[4 * lane + k]);
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int e = lane; e < SO * np; e += NW) so[e] = NAN;
        if (lane < WO) wo[lane] = lane == 0 ? (double)VIO_ERR_NOT_FINITE : (lane == 1 ? -1.0 : NAN);
        return;
    }
    if (lane < np) {
        // Quaternion(Rc[k]), Quaternion(Rimu[k]) with Rimu = delta_q.toRotationMatrix(); D = L(q_c) - R(q_imu) over (x, y, z, w)
        double *p = s_p[lane];
        double qc[4], qi[4], Rimu[9];
        rot_to_quat(rc + 9 * lane, qc);
        quat_to_rot(dq + 4 * lane, Rimu);
        rot_to_quat(Rimu, qi);
        const double cw = qc[0], cx = qc[1], cy = qc[2], cz = qc[3], iw = qi[0], ix = qi[1], iy = qi[2], iz = qi[3];
        const double L[16] = {cw, -cz, cy, cx, cz, cw, -cx, cy, -cy, cx, cw, cz, -cx, -cy, -cz, cw};
        const double R[16] = {iw, iz, -iy, ix, -iz, iw, ix, iy, iy, -ix, iw, iz, -ix, -iy, -iz, iw};
        double D[16];
        for (int k = 0; k < 16; ++k) D[k] = L[k] - R[k];
        for (int k = 0; k < 4; ++k) p[k] = qc[k];
        int e = 4;
        for (int r = 0; r < 4; ++r)
            for (int c = r; c < 4; ++c) p[e++] = ((D[r] * D[c] + D[4 + r] * D[4 + c]) + D[8 + r] * D[8 + c]) + D[12 + r] * D[12 + c];
        for (int k = 0; k < 9; ++k) p[14 + k] = Rimu[k];
    }
    __syncthreads();
    if (lane != 0) return;
    double ric[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, N[16];
    for (int k = 0; k < 16; ++k) N[k] = 0.0;
    int first = -1, fin = 1;
    for (int k = 0; k < np; ++k) {
        const double *p = s_p[k];
        double ricT[9], tmp[9], Rg[9], qg[4];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) ricT[3 * r + c] = ric[3 * c + r];
        mm3(ricT, p + 14, tmp);
        mm3(tmp, ric, Rg);
        rot_to_quat(Rg, qg);
        // angularDistance: d = q_c * conj(q_g), 2 atan2(|vec d|, |d.w|)
        const double aw = p[0], ax = p[1], ay = p[2], az = p[3], bw = qg[0], bx = -qg[1], by = -qg[2], bz = -qg[3];
        const double dw = ((aw * bw - ax * bx) - ay * by) - az * bz;
        const double dx = ((aw * bx + ax * bw) + ay * bz) - az * by;
        const double dy = ((aw * by + ay * bw) + az * bx) - ax * bz;
        const double dz = ((aw * bz + az * bw) + ax * by) - ay * bx;
        const double deg = 180.0 / M_PI * (2.0 * atan2(sqrt((dx * dx + dy * dy) + dz * dz), fabs(dw)));
        const double huber = deg > a.huber_deg ? a.huber_deg / deg : 1.0;
        const double h2 = huber * huber;
        int e = 4;
        for (int r = 0; r < 4; ++r)
            for (int c = r; c < 4; ++c) {
                N[4 * r + c] = N[4 * r + c] + h2 * p[e++];
                N[4 * c + r] = N[4 * r + c];
            }
        double A[16], V[16];
        for (int i = 0; i < 16; ++i) A[i] = N[i];
        jacobi(4, A, V);
        const int mi = argmin_diag(4, A);
        int ord[4] = {0, 1, 2, 3};
        for (int x = 1; x < 4; ++x)                     // stable, descending
            for (int y = x; y > 0 && A[5 * ord[y]] > A[5 * ord[y - 1]]; --y) { const int t = ord[y]; ord[y] = ord[y - 1]; ord[y - 1] = t; }
        double sig[3];
        for (int i = 0; i < 3; ++i) sig[i] = sqrt(fmax(A[5 * ord[1 + i]], 0.0));
        const double x[4] = {V[12 + mi], V[mi], V[4 + mi], V[8 + mi]};         // (w, x, y, z) of Quaterniond(x): x holds (x, y, z, w)
        double Rx[9], q[4];
        quat_to_rot(x, Rx);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) ric[3 * r + c] = Rx[3 * c + r];
        rot_to_quat(ric, q);
        double *s = so + (int64_t)SO * k;
        for (int i = 0; i < 4; ++i) { s[i] = q[i]; fin &= isfinite(q[i]) != 0; }
        for (int i = 0; i < 9; ++i) { s[4 + i] = ric[i]; fin &= isfinite(ric[i]) != 0; }
        for (int i = 0; i < 3; ++i) { s[13 + i] = sig[i]; fin &= isfinite(sig[i]) != 0; }
        s[16] = huber;
        if (first < 0 && k + 1 >= a.min_frames && sig[1] > a.min_sigma) {
            first = k;
            for (int i = 0; i < 13; ++i) wo[2 + i] = s[i];
        }
    }
    if (!fin) {
        for (int e = 0; e < SO * np; ++e) so[e] = NAN;
        wo[0] = VIO_ERR_NOT_FINITE; wo[1] = -1;
        for (int i = 0; i < 13; ++i) wo[2 + i] = NAN;
        return;
    }
    wo[0] = first >= 0 ? VIO_OK : VIO_EXROT_FAIL_NOT_OBSERVABLE;
    wo[1] = first >= 0 ? first + 1 : -1;
    if (first < 0)
        for (int i = 0; i < 13; ++i) wo[2 + i] = NAN;
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_exrot {
    int device = 0;
    ErrText err = {0};
    vio_exrot_config cfg = {VIO_EXROT_DEFAULT_MIN_FRAMES, 0, VIO_EXROT_DEFAULT_MIN_SIGMA, VIO_EXROT_DEFAULT_HUBER_DEG};
    Twin<char> staging;                                  // window descriptors | pair descriptors | int32 | doubles
    DevBuf<double> scr;
    Twin<double> pout, rc, sout, wout;
    StreamEvents<4> q;                                   // events: upload start, stage 1 start, stage 2 start, end
    double timing[4] = {NAN, NAN, NAN, NAN};
};

namespace {

vio_status check_item(vio_exrot *h, int i, const vio_exrot_item &it, bool tracks, bool imu) {
    if (it.n_frames < 2 || it.n_frames > VIO_EXROT_MAX_FRAMES)
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: n_frames must be in [2, %d]", i, VIO_EXROT_MAX_FRAMES);
    if (imu && !it.delta_q) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: delta_q is required", i);
    if (!tracks) return VIO_OK;
    if (it.n_tracks < 0 || it.n_tracks > VIO_EXROT_MAX_TRACKS)
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: n_tracks must be in [0, %d]", i, VIO_EXROT_MAX_TRACKS);
    if (!it.obs_offset || (it.n_tracks > 0 && (!it.start_frame || !it.pts)))
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: start_frame, obs_offset and pts are required", i);
    if (it.obs_offset[0] != 0) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: obs_offset[0] must be 0", i);
    for (int j = 0; j < it.n_tracks; ++j) {
        const int64_t len = it.obs_offset[j + 1] - it.obs_offset[j];
        if (len < 1 || it.start_frame[j] < 0 || it.start_frame[j] + len > it.n_frames)
            return fail(h->err, VIO_ERR_BAD_ARG, "window %d: track %d is empty or leaves the window", i, j);
    }
    return VIO_OK;
}

struct Staged {
    size_t b_win = 0, b_pair = 0, b_int = 0, bytes = 0;
    int64_t scr = 0, npairs = 0;
};

vio_status stage(vio_exrot *h, int count, const vio_exrot_item *items, bool tracks, bool imu, Staged &s) {
    for (int i = 0; i < count; ++i) {
        const vio_status st = check_item(h, i, items[i], tracks, imu);
        if (st != VIO_OK) return st;
    }
    int64_t ni = 0, nd = 0;
    std::vector<ExWin> wins((size_t)count);
    std::vector<ExPair> pairs;
    for (int i = 0; i < count; ++i) {
        const vio_exrot_item &it = items[i];
        ExWin &w = wins[(size_t)i];
        std::memset(&w, 0, sizeof(w));
        w.F = it.n_frames;
        w.nt = tracks ? it.n_tracks : 0;
        w.nobs = tracks ? (int32_t)it.obs_offset[w.nt] : 0;
        w.o_int = ni; ni += 2 * (int64_t)w.nt + 1;
        w.o_pts = nd; nd += 2 * (int64_t)w.nobs;
        w.o_dq = nd; nd += imu ? 4 * (int64_t)(w.F - 1) : 0;
        w.o_pair = s.npairs;
        // getCorresponding(k, k + 1): track j is in pairs start_frame[j] .. start_frame[j] + len - 2
        std::vector<int32_t> cap((size_t)(w.F - 1), 0);
        for (int j = 0; j < w.nt; ++j) {
            const int len = (int)(it.obs_offset[j + 1] - it.obs_offset[j]);
            for (int k = it.start_frame[j]; k < it.start_frame[j] + len - 1; ++k) ++cap[(size_t)k];
        }
        for (int k = 0; k < w.F - 1; ++k) {
            ExPair p;
            std::memset(&p, 0, sizeof(p));
            p.win = i; p.k = k; p.cap = cap[(size_t)k]; p.o_scr = s.scr;
            s.scr += 13 * (int64_t)p.cap;
            pairs.push_back(p);
        }
        s.npairs += w.F - 1;
    }
    s.b_win = align256(sizeof(ExWin) * (size_t)count);
    s.b_pair = align256(sizeof(ExPair) * pairs.size());
    s.b_int = align256(sizeof(int32_t) * (size_t)ni);
    s.bytes = s.b_win + s.b_pair + s.b_int + sizeof(double) * (size_t)nd;
    const vio_status st = h->staging.ensure(h->err, s.bytes);
    if (st != VIO_OK) return st;
    std::memcpy(h->staging.h, wins.data(), sizeof(ExWin) * (size_t)count);
    std::memcpy(h->staging.h + s.b_win, pairs.data(), sizeof(ExPair) * pairs.size());
    int32_t *hi = (int32_t *)(h->staging.h + s.b_win + s.b_pair);
    double *hd = (double *)(h->staging.h + s.b_win + s.b_pair + s.b_int);
    for (int i = 0; i < count; ++i) {
        const vio_exrot_item &it = items[i];
        const ExWin &w = wins[(size_t)i];
        for (int j = 0; j < w.nt; ++j) hi[w.o_int + j] = it.start_frame[j];
        for (int j = 0; j <= w.nt; ++j) hi[w.o_int + w.nt + j] = tracks ? (int32_t)it.obs_offset[j] : 0;
        if (w.nobs) std::memcpy(hd + w.o_pts, it.pts, sizeof(double) * 2 * (size_t)w.nobs);
        if (imu) std::memcpy(hd + w.o_dq, it.delta_q, sizeof(double) * 4 * (size_t)(w.F - 1));
    }
    return VIO_OK;
}

// the three entry points: stage 1 (do1), stage 2 (do2) or both
vio_status run(vio_exrot *h, const char *name, int32_t count, const vio_exrot_item *items, bool do1, bool do2, const double *rc_in,
               vio_exrot_pair *pairs, vio_exrot_result *res, vio_exrot_step *steps) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || (count > 0 && (!items || (do1 && !do2 && !pairs) || (do2 && !do1 && !rc_in) || (do2 && !res))))
        return fail(h->err, VIO_ERR_BAD_ARG, "%s: negative count or a NULL array", name);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    DeviceScope dev(h->device);                     // before stage(): its buffers belong on the handle's device
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    Staged s;
    vio_status st = stage(h, count, items, do1, do2, s);
    if (st != VIO_OK) return st;
    const size_t np = (size_t)s.npairs;
    const size_t poutb = sizeof(double) * PO * np, rcb = sizeof(double) * 9 * np, soutb = sizeof(double) * SO * np;
    const size_t woutb = sizeof(double) * WO * (size_t)count;
    if ((st = h->pout.ensure(h->err, poutb)) != VIO_OK || (st = h->rc.ensure(h->err, rcb)) != VIO_OK ||
        (st = h->sout.ensure(h->err, soutb)) != VIO_OK || (st = h->wout.ensure(h->err, woutb)) != VIO_OK ||
        (st = h->scr.ensure(h->err, sizeof(double) * (size_t)(s.scr + 1))) != VIO_OK)
        return st;
    if (rc_in) std::memcpy(h->rc.h, rc_in, rcb);
    ExArgs a;
    a.wins = (const ExWin *)h->staging.d;
    a.pairs = (const ExPair *)(h->staging.d + s.b_win);
    a.ints = (const int32_t *)(h->staging.d + s.b_win + s.b_pair);
    a.dd = (const double *)(h->staging.d + s.b_win + s.b_pair + s.b_int);
    a.scr = h->scr.d; a.pout = h->pout.d; a.rc = h->rc.d; a.sout = h->sout.d; a.wout = h->wout.d;
    a.min_frames = h->cfg.min_frames; a.min_sigma = h->cfg.min_sigma; a.huber_deg = h->cfg.huber_deg;
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->staging.d, h->staging.h, s.bytes, hipMemcpyHostToDevice, q) != hipSuccess ||
        (rc_in && hipMemcpyAsync(h->rc.d, h->rc.h, rcb, hipMemcpyHostToDevice, q) != hipSuccess))
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    if (do1) hipLaunchKernelGGL(k_exrot_pairs, dim3((unsigned)np), dim3(NT), 0, q, a);
    (void)hipEventRecord(h->q.ev[2], q);
    if (do2) hipLaunchKernelGGL(k_exrot_solve, dim3(count), dim3(NW), 0, q, a);
    (void)hipEventRecord(h->q.ev[3], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    bool okc = true;
    if (do1) {
        okc = okc && hipMemcpyAsync(h->pout.h, h->pout.d, poutb, hipMemcpyDeviceToHost, q) == hipSuccess;
        okc = okc && hipMemcpyAsync(h->rc.h, h->rc.d, rcb, hipMemcpyDeviceToHost, q) == hipSuccess;
    }
    if (do2) {
        okc = okc && hipMemcpyAsync(h->sout.h, h->sout.d, soutb, hipMemcpyDeviceToHost, q) == hipSuccess;
        okc = okc && hipMemcpyAsync(h->wout.h, h->wout.d, woutb, hipMemcpyDeviceToHost, q) == hipSuccess;
    }
    if (!okc || hipStreamSynchronize(q) != hipSuccess) return fail_synced(h, "kernel or read-back failed");
    vio_status ret = VIO_OK;
    size_t row = 0;
    for (int i = 0; i < count; ++i) {
        const int wp = items[i].n_frames - 1;
        bool bad = false;
        if (do1)
            for (int k = 0; k < wp; ++k) {
                const double *o = h->pout.h + (size_t)PO * (row + k);
                bad = bad || (int32_t)o[0] == VIO_ERR_NOT_FINITE;
                if (!pairs) continue;
                vio_exrot_pair &p = pairs[row + k];
                p.status = (int32_t)o[0]; p.n_corres = (int32_t)o[1];
                for (int c = 0; c < 4; ++c) p.front[c] = (int32_t)o[2 + c];
                p.choice = (int32_t)o[6]; p.det_flip = (int32_t)o[7];
                std::memcpy(p.Rc, h->rc.h + 9 * (row + k), sizeof(double) * 9);
            }
        if (do2) {
            const double *o = h->wout.h + (size_t)WO * i;
            vio_exrot_result &r = res[i];
            r.status = (int32_t)o[0]; r.step = (int32_t)o[1];
            std::memcpy(r.q, o + 2, sizeof(double) * 4);
            std::memcpy(r.R, o + 6, sizeof(double) * 9);
            bad = bad || r.status == VIO_ERR_NOT_FINITE;
            if (steps)
                for (int k = 0; k < wp; ++k) {
                    const double *so = h->sout.h + (size_t)SO * (row + k);
                    vio_exrot_step &t = steps[row + k];
                    std::memcpy(t.q, so, sizeof(double) * 4);
                    std::memcpy(t.R, so + 4, sizeof(double) * 9);
                    std::memcpy(t.sigma, so + 13, sizeof(double) * 3);
                    t.huber = so[16];
                }
        }
        if (bad) {
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "window %d: non-finite input or result", i);
            ret = VIO_ERR_NOT_FINITE;
        }
        row += (size_t)wp;
    }
    const auto t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[1] = do1 ? elapsed_ms(h->q.ev[1], h->q.ev[2]) : NAN;
    h->timing[2] = do2 ? elapsed_ms(h->q.ev[2], h->q.ev[3]) : NAN;
    h->timing[3] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return ret;
}

}  // namespace

extern "C" {

int32_t vio_exrot_version(void) { return VIO_EXROT_VERSION; }

const char *vio_exrot_last_error(const vio_exrot *h) { return h ? h->err : "NULL handle"; }

vio_status vio_exrot_create(int32_t device, void *stream, vio_exrot **out) { return create_handle(device, stream, out, vio_exrot_destroy); }

void vio_exrot_destroy(vio_exrot *h) { destroy_handle(h); }

vio_status vio_exrot_set_config(vio_exrot *h, const vio_exrot_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg || cfg->min_frames < 1 || !(cfg->min_sigma >= 0.0) || !std::isfinite(cfg->min_sigma) || !(cfg->huber_deg > 0.0) ||
        !std::isfinite(cfg->huber_deg))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_exrot_set_config: min_frames >= 1, min_sigma >= 0 and huber_deg > 0 (finite) are required");
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_exrot_timing(const vio_exrot *h, double *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_exrot_relative_rotations_batch(vio_exrot *h, int32_t count, const vio_exrot_item *items, vio_exrot_pair *pairs) {
    return run(h, "vio_exrot_relative_rotations_batch", count, items, true, false, nullptr, pairs, nullptr, nullptr);
}

vio_status vio_exrot_calibrate_batch(vio_exrot *h, int32_t count, const vio_exrot_item *items, const double *Rc, vio_exrot_result *res,
                                     vio_exrot_step *steps) {
    return run(h, "vio_exrot_calibrate_batch", count, items, false, true, Rc, nullptr, res, steps);
}

vio_status vio_exrot_batch(vio_exrot *h, int32_t count, const vio_exrot_item *items, vio_exrot_pair *pairs, vio_exrot_result *res,
                           vio_exrot_step *steps) {
    return run(h, "vio_exrot_batch", count, items, true, true, nullptr, pairs, res, steps);
}

}  // extern "C"
