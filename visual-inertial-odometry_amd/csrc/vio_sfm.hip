// vio_sfm.hip — libvio_sfm_hip.so: structure-from-motion of many windows in one call (include/vio_sfm.h).
//
//   k_sfm_relpose    one 256-thread workgroup per window: relativePose + solveRelativeRT.  Thread c < F-1 counts candidate c's
//                    correspondences and sums their parallax in track order; then the candidates in ascending order, the first one
//                    that passes wins: one thread lists the correspondences, thread h fits hypothesis h (sample, Hartley scaling,
//                    9 x 9 normal matrix, Jacobi, rank 2) and scores it over all correspondences, the winner (most inliers, lowest
//                    h) is refitted on its inliers by one thread, the final mask and recoverPose's four cheirality counts are taken
//                    thread per correspondence (integer LDS counters)
//   k_sfm_construct  one 256-thread workgroup per window: GlobalSFM::construct.  Triangulation thread per track; PnP with the
//                    6 x 6 normal equations summed entry per thread over the per-point terms in point order; the bundle adjustment
//                    thread per track for the linearisation, the point blocks and the back substitution, entry per thread for the
//                    Schur complement (each entry sums its tracks' terms in track order), Cholesky column by column in LDS
// The per-window arrays (correspondences, points, per-track and per-observation blocks) live in HBM scratch; LDS holds the camera
// states, the reduced system (the packed lower triangle of 6F x 6F doubles) and the small vectors: 18 F^2 + 87 F doubles.  Contraction is off: products and sums round as the host
// restatement's (tests/sfm_reference.py) do.  No floating-point atomics; every sum has a fixed order, so repeated calls are bitwise
// identical and a window's result does not depend on its batch.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_sfm.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_sfm_math.h"

constexpr int NT = 256;
constexpr int MAXF = VIO_SFM_MAX_FRAMES;
constexpr int REL = 18 + 2 * MAXF;      // status, l, hyp, n_corres, n_inliers, n_front, R (9), T (3), corres (MAXF), parallax (MAXF)
constexpr int OUTC = 7 + 8 * MAXF;      // status, fail_frame, ba_it, converged, n_tri, c0, c1, Q (4 MAXF), T (3 MAXF), pnp_it (MAXF)
constexpr int TR = 33;                  // per track: Hpp 9, Hinv 9, gp 3, Dp 3, dp 3, cost, gmax, d2, x2, gdot, ddd
constexpr int OB = 56;                  // per observation: Jc 12, Jp 6, r 2, W 18, Y 18
constexpr int PC = 28;                  // per PnP point: upper triangle of Jc^T Jc (21), Jc^T r (6), r^2

constexpr double FOCAL = 460.0;
constexpr double RANSAC_THR = 0.3 / 460.0;
constexpr double MAX_DEPTH = 50.0;
constexpr double BA_COST_OK = 5e-3;

struct SfmWin {
    int32_t F, nt, nobs, pad;
    int64_t o_int;      // staged int32: start_frame [nt], obs_offset [nt + 1]
    int64_t o_pts;      // staged doubles: pts [nobs][2]
    int64_t o_scr;      // double scratch: corr 4 nt | X 3 nt | X2 3 nt | TR nt | OB nobs | PC nt
    int64_t o_iscr;     // int scratch: state nt | list nt | mask nt
    int64_t o_trk;      // the window's first row in the flat per-track outputs
};

struct SfmArgs {
    const SfmWin *wins;
    const int32_t *ints;
    const double *dd;
    double *scr;
    int32_t *iscr;
    double *rel;        // [count][REL]
    double *out;        // [count][OUTC]
    double *pts_out;    // [tracks][4]: point, state
    uint32_t seed;
    int32_t hyps;
};

// ---------------------------------------------------------------------------------------------------------
// small dense kernels (one thread)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hash4(uint32_t seed, uint32_t i, uint32_t h, uint32_t k) {
    return mix32(mix32(mix32(mix32(seed + 0x9e3779b9u) + i) + h) + k);
}
__device__ void sample8(uint32_t seed, int i, int h, int n, int *out) {
    int taken[8];
    for (int k = 0; k < 8; ++k) {
        int idx = (int)(hash4(seed, (uint32_t)i, (uint32_t)h, (uint32_t)k) % (uint32_t)(n - k));
        int pos = 0;
        while (pos < k && idx >= taken[pos]) { ++idx; ++pos; }
        for (int m = k; m > pos; --m) taken[m] = taken[m - 1];
        taken[pos] = idx;
        out[k] = idx;
    }
}


__host__ __device__ constexpr int tri(int i) { return i * (i + 1) / 2; }      // packed lower triangle: row i starts here
__device__ __forceinline__ bool has_frame(int sf, int n, int f) { return sf <= f && sf + n - 1 >= f; }

// ---------------------------------------------------------------------------------------------------------
// k_sfm_relpose
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_sfm_relpose(SfmArgs a) {
    const SfmWin W = a.wins[blockIdx.x];
    const int tid = threadIdx.x, F = W.F, nt = W.nt;
    const int32_t *sf = a.ints + W.o_int, *off = sf + nt;
    const double *pts = a.dd + W.o_pts;
    double *corr = a.scr + W.o_scr;
    int32_t *list = a.iscr + W.o_iscr + nt, *mask = a.iscr + W.o_iscr + 2 * (int64_t)nt;
    double *o = a.rel + (int64_t)REL * blockIdx.x;

    __shared__ int s_cnt[MAXF];
    __shared__ double s_par[MAXF];
    __shared__ int s_bc[NT], s_bh[NT];
    __shared__ double s_F[NT][9];
    __shared__ double s_E[9], s_R[4][9], s_t[4][3];
    __shared__ int s_i[8];              // n, winner thread, ok, n_inliers, front[4]

    int bad = 0;
    for (int k = tid; k < 2 * W.nobs; k += NT) bad |= !isfinite(pts[k]);
    for (int k = tid; k < nt; k += NT) mask[k] = 0;
    if (tid >= 6 && tid < REL) o[tid] = tid < 18 ? NAN : 0.0;
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) { o[0] = VIO_ERR_NOT_FINITE; o[1] = -1; o[2] = -1; o[3] = 0; o[4] = 0; o[5] = 0; }
        return;
    }
    if (tid < F - 1) {
        int n = 0;
        double s = 0.0;
        for (int j = 0; j < nt; ++j) {
            const int len = off[j + 1] - off[j];
            if (sf[j] <= tid && sf[j] + len - 1 >= F - 1) {
                const double *p0 = pts + 2 * (int64_t)(off[j] + tid - sf[j]), *p1 = pts + 2 * (int64_t)(off[j] + F - 1 - sf[j]);
                const double dx = p0[0] - p1[0], dy = p0[1] - p1[1];
                s = s + sqrt(dx * dx + dy * dy);
                ++n;
            }
        }
        s_cnt[tid] = n;
        s_par[tid] = n ? s / n * FOCAL : 0.0;
        o[18 + tid] = n;
        o[18 + MAXF + tid] = s_par[tid];
    }
    __syncthreads();
    const double thr = RANSAC_THR * RANSAC_THR;
    int status = VIO_SFM_FAIL_RELATIVE_POSE, l = -1;
    for (int i = 0; i < F - 1; ++i) {
        if (!(s_cnt[i] > 20 && s_par[i] > 30.0)) continue;          // (uniform: LDS values)
        const int n = s_cnt[i];
        if (tid == 0) {
            int m = 0;
            for (int j = 0; j < nt; ++j) {
                const int len = off[j + 1] - off[j];
                if (sf[j] <= i && sf[j] + len - 1 >= F - 1) {
                    const double *p0 = pts + 2 * (int64_t)(off[j] + i - sf[j]), *p1 = pts + 2 * (int64_t)(off[j] + F - 1 - sf[j]);
                    corr[4 * m] = p0[0]; corr[4 * m + 1] = p0[1]; corr[4 * m + 2] = p1[0]; corr[4 * m + 3] = p1[1];
                    ++m;
                }
            }
            for (int k = 0; k < 8; ++k) s_i[k] = 0;
        }
        __syncthreads();
        int bc = -1, bh = 0x7fffffff;
        double bF[9];
        for (int h = tid; h < a.hyps; h += NT) {
            int idx[8];
            double Fm[9];
            sample8(a.seed, i, h, n, idx);
            eight_point(corr, idx, 8, Fm);
            int c = 0;
            for (int k = 0; k < n; ++k) c += epipolar_error(Fm, corr + 4 * k) <= thr;
            if (c > bc) {
                bc = c; bh = h;
                for (int k = 0; k < 9; ++k) bF[k] = Fm[k];
            }
        }
        s_bc[tid] = bc; s_bh[tid] = bh;
        for (int k = 0; k < 9; ++k) s_F[tid][k] = bc >= 0 ? bF[k] : 0.0;
        __syncthreads();
        if (tid == 0) {
            int w = 0;
            for (int t = 1; t < NT; ++t)
                if (s_bc[t] > s_bc[w] || (s_bc[t] == s_bc[w] && s_bh[t] < s_bh[w])) w = t;
            s_i[1] = w;
            int ok = s_bc[w] >= 8;
            if (ok) {
                int m = 0;
                for (int k = 0; k < n; ++k)
                    if (epipolar_error(s_F[w], corr + 4 * k) <= thr) list[m++] = k;
                double Fm[9];
                eight_point(corr, list, m, Fm);
                for (int k = 0; k < 9; ++k) { s_E[k] = Fm[k]; ok &= isfinite(Fm[k]) != 0; }
            }
            s_i[2] = ok;
        }
        __syncthreads();
        const int hyp = s_bh[s_i[1]];
        if (!s_i[2]) { __syncthreads(); continue; }
        for (int k = tid; k < n; k += NT) {
            const int in = epipolar_error(s_E, corr + 4 * k) <= thr;
            mask[k] = in;
            if (in) atomicAdd(&s_i[3], 1);
        }
        if (tid == 0) {
            // recoverPose: E = U diag V^T from the eigenvectors of E^T E, the four (R, t)
            double G[9], V[9], E[9];
            for (int k = 0; k < 9; ++k) E[k] = s_E[k];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) G[3 * r + c] = E[r] * E[c] + E[3 + r] * E[3 + c] + E[6 + r] * E[6 + c];
            jacobi(3, G, V);
            int ord[3] = {0, 1, 2};
            for (int x = 1; x < 3; ++x)                     // stable, descending
                for (int y = x; y > 0 && G[4 * ord[y]] > G[4 * ord[y - 1]]; --y) { const int t = ord[y]; ord[y] = ord[y - 1]; ord[y - 1] = t; }
            double Vs[9], U[9];
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
            const double det = Vs[0] * (Vs[4] * Vs[8] - Vs[5] * Vs[7]) - Vs[1] * (Vs[3] * Vs[8] - Vs[5] * Vs[6]) +
                               Vs[2] * (Vs[3] * Vs[7] - Vs[4] * Vs[6]);
            if (det < 0)
                for (int r = 0; r < 3; ++r) Vs[3 * r + 2] = -Vs[3 * r + 2];
            for (int r = 0; r < 3; ++r) { U[3 * r] = u0[r]; U[3 * r + 1] = u1[r]; U[3 * r + 2] = u2[r]; }
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    // U W = (u1, -u0, u2), U W^T = (-u1, u0, u2), times V^T
                    const double r1 = (U[3 * r + 1] * Vs[3 * c] + (-U[3 * r]) * Vs[3 * c + 1]) + U[3 * r + 2] * Vs[3 * c + 2];
                    const double r2 = ((-U[3 * r + 1]) * Vs[3 * c] + U[3 * r] * Vs[3 * c + 1]) + U[3 * r + 2] * Vs[3 * c + 2];
                    s_R[0][3 * r + c] = r1; s_R[2][3 * r + c] = r1;
                    s_R[1][3 * r + c] = r2; s_R[3][3 * r + c] = r2;
                }
            for (int r = 0; r < 3; ++r) { s_t[0][r] = u2[r]; s_t[1][r] = u2[r]; s_t[2][r] = -u2[r]; s_t[3][r] = -u2[r]; }
        }
        __syncthreads();
        {
            const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z3[3] = {0, 0, 0};
            for (int e = tid; e < 4 * n; e += NT) {
                const int c = e / n, k = e % n;
                if (!mask[k]) continue;
                double X[3];
                triangulate(I3, z3, s_R[c], s_t[c], corr + 4 * k, corr + 4 * k + 2, X);
                const double z1 = X[2], z2 = (s_R[c][6] * X[0] + s_R[c][7] * X[1] + s_R[c][8] * X[2]) + s_t[c][2];
                if (z1 > 0 && z1 < MAX_DEPTH && z2 > 0 && z2 < MAX_DEPTH) atomicAdd(&s_i[4 + c], 1);
            }
        }
        __syncthreads();
        int best = 0;
        for (int c = 1; c < 4; ++c)
            if (s_i[4 + c] > s_i[4 + best]) best = c;
        int fin = 1;
        for (int k = 0; k < 9; ++k) fin &= isfinite(s_R[best][k]) != 0;
        for (int k = 0; k < 3; ++k) fin &= isfinite(s_t[best][k]) != 0;
        const bool ok = fin && s_i[4 + best] > 12;
        if (ok) {
            if (tid == 0) {
                const double *R = s_R[best], *t = s_t[best];
                o[2] = hyp; o[3] = n; o[4] = s_i[3]; o[5] = s_i[4 + best];
                for (int r = 0; r < 3; ++r) {
                    for (int c = 0; c < 3; ++c) o[6 + 3 * r + c] = R[3 * c + r];
                    o[15 + r] = -((R[r] * t[0] + R[3 + r] * t[1]) + R[6 + r] * t[2]);
                }
            }
            status = VIO_OK;
            l = i;
            break;
        }
        __syncthreads();
        for (int k = tid; k < n; k += NT) mask[k] = 0;
        __syncthreads();
    }
    if (tid == 0) {
        o[0] = status; o[1] = l;
        if (status != VIO_OK) { o[2] = -1; o[3] = 0; o[4] = 0; o[5] = 0; }
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_sfm_construct
// ---------------------------------------------------------------------------------------------------------
struct Lm {
    double cost, cost2, prev, radius, v, rho, lam, c0;      // cost: at the state; cost2: at the trial state; prev: before the step taken
    int it, ok, stop, converged, npts;
};

struct Ctx {
    int tid, F, nt, l;
    const int32_t *sf, *off;
    const double *pts;
    double *X, *X2, *trk, *obs, *pc;
    int32_t *state, *list;
    double *camR, *camt, *camR2, *camt2;     // LDS: [F][9], [F][3]
    double *S, *rhs, *dc, *Dc, *gc, *Hcc;    // LDS: packed lower triangle of n x n, n, n, n, n, F x 36
    double *h28;                             // LDS: 28
    Lm *lm;
};

// PnP sums over the listed points: with full, the 28 entries of (upper Jc^T Jc, Jc^T r, r^2) into h28; without, r^2 alone (h28[27])
__device__ void pnp_sums(const Ctx &c, int i, const double *R, const double *t, bool full) {
    const int n = c.lm->npts;
    for (int k = c.tid; k < n; k += NT) {
        const int j = c.list[k];
        double r[2], Xc[3], RX[3];
        residual(R, t, c.X + 3 * (int64_t)j, c.pts + 2 * (int64_t)(c.off[j] + i - c.sf[j]), r, Xc, RX);
        double *o = c.pc + (int64_t)PC * k;
        o[27] = r[0] * r[0] + r[1] * r[1];
        if (full) {
            double Jc[12], Jp[6];
            jac_cam(Xc, RX, Jc, Jp);
            int e = 0;
            for (int x = 0; x < 6; ++x)
                for (int y = x; y < 6; ++y) o[e++] = Jc[x] * Jc[y] + Jc[6 + x] * Jc[6 + y];
            for (int x = 0; x < 6; ++x) o[21 + x] = Jc[x] * r[0] + Jc[6 + x] * r[1];
        }
    }
    __syncthreads();
    if (c.tid < PC && (full || c.tid == 27)) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s = s + c.pc[(int64_t)PC * k + c.tid];
        c.h28[c.tid] = s;
    }
    __syncthreads();
}

// GlobalSFM::solveFrameByPnP of frame i from frame guess's pose; false: the construct fails at frame i
__device__ bool pnp(const Ctx &c, int i, int guess, double *o_it) {
    Lm *lm = c.lm;
    const int tid = c.tid;
    if (tid == 0) {
        int n = 0;
        for (int j = 0; j < c.nt; ++j)
            if (c.state[j] && has_frame(c.sf[j], c.off[j + 1] - c.off[j], i)) c.list[n++] = j;
        lm->npts = n;
    }
    __syncthreads();
    if (lm->npts < 10) return false;
    double *R = c.camR + 9 * i, *t = c.camt + 3 * i, *R2 = c.camR2 + 9 * i, *t2 = c.camt2 + 3 * i;
    if (tid < 9) R[tid] = c.camR[9 * guess + tid];
    if (tid < 3) t[tid] = c.camt[3 * guess + tid];
    __syncthreads();
    pnp_sums(c, i, R, t, true);
    if (tid == 0) {
        lm->cost = 0.5 * c.h28[27];
        lm->radius = VIO_SFM_LM_INITIAL_RADIUS; lm->v = 2.0; lm->it = 0; lm->stop = 0;
        double gm = 0.0;
        for (int k = 0; k < 6; ++k) gm = fmax(gm, fabs(c.h28[21 + k]));
        if (!isfinite(lm->cost)) lm->stop = 2;
        else if (gm <= VIO_SFM_BA_GRADIENT_TOL) lm->stop = 1;
    }
    __syncthreads();
    for (;;) {
        const bool go = !lm->stop && lm->it < VIO_SFM_PNP_MAX_ITER;
        __syncthreads();             // (every thread has read the flags before thread 0 moves them)
        if (!go) break;
        if (tid == 0) {
            lm->it += 1;
            lm->lam = 1.0 / lm->radius;
            double A[36], g[6], D[6], d[6];
            int e = 0;
            for (int x = 0; x < 6; ++x)
                for (int y = x; y < 6; ++y) { A[6 * x + y] = c.h28[e]; A[6 * y + x] = c.h28[e]; ++e; }
            for (int k = 0; k < 6; ++k) {
                g[k] = -c.h28[21 + k];
                D[k] = fmin(fmax(A[7 * k], LM_DIAG_MIN), LM_DIAG_MAX);
                A[7 * k] = A[7 * k] + lm->lam * D[k];
            }
            lm->ok = cholesky_solve6(A, g, d);
            if (lm->ok) {
                double d2 = 0.0;
                for (int k = 0; k < 6; ++k) d2 += d[k] * d[k];
                if (sqrt(d2) <= VIO_SFM_PNP_STEP_TOL) lm->stop = 1;
                double E[9];
                exp_so3(d, E);
                mm3(E, R, R2);
                for (int k = 0; k < 3; ++k) t2[k] = t[k] + d[3 + k];
                double ddd = 0.0, gd = 0.0;
                for (int k = 0; k < 6; ++k) { ddd += (d[k] * D[k]) * d[k]; gd += d[k] * c.h28[21 + k]; }
                lm->rho = 0.5 * (lm->lam * ddd - gd);           // the model's decrease, until the trial cost is known
            }
        }
        __syncthreads();
        const int stop = lm->stop, solved = lm->ok;
        __syncthreads();
        if (stop) break;
        if (solved) pnp_sums(c, i, R2, t2, false);
        if (tid == 0) {
            bool take = false;
            if (lm->ok) {
                lm->cost2 = 0.5 * c.h28[27];
                const double model = lm->rho;
                lm->rho = (isfinite(lm->cost2) && model > 0) ? (lm->cost - lm->cost2) / model : -1.0;
                take = lm->rho > LM_MIN_RHO;
            }
            lm->ok = take;
            if (take) {
                for (int k = 0; k < 9; ++k) R[k] = R2[k];
                for (int k = 0; k < 3; ++k) t[k] = t2[k];
            } else {
                lm->radius = lm->radius / lm->v;
                lm->v = lm->v * 2.0;
                if (lm->radius < LM_RADIUS_MIN) lm->stop = 1;
            }
        }
        __syncthreads();
        if (lm->ok) {
            pnp_sums(c, i, R, t, true);
            if (tid == 0) {
                lm->cost = 0.5 * c.h28[27];
                double gm = 0.0;
                for (int k = 0; k < 6; ++k) gm = fmax(gm, fabs(c.h28[21 + k]));
                if (gm <= VIO_SFM_BA_GRADIENT_TOL) lm->stop = 1;
                else { lm->radius = lm_radius(lm->radius, lm->rho); lm->v = 2.0; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0) *o_it = lm->it;
    int fin = lm->stop != 2;
    for (int k = 0; k < 9; ++k) fin &= isfinite(R[k]) != 0;
    for (int k = 0; k < 3; ++k) fin &= isfinite(t[k]) != 0;
    __syncthreads();
    return fin;
}

// triangulateTwoFrames(f0, f1): the tracks not triangulated yet that are seen in both
__device__ void tri_two(const Ctx &c, int f0, int f1) {
    for (int j = c.tid; j < c.nt; j += NT) {
        const int len = c.off[j + 1] - c.off[j];
        if (!c.state[j] && has_frame(c.sf[j], len, f0) && has_frame(c.sf[j], len, f1)) {
            triangulate(c.camR + 9 * f0, c.camt + 3 * f0, c.camR + 9 * f1, c.camt + 3 * f1, c.pts + 2 * (int64_t)(c.off[j] + f0 - c.sf[j]),
                        c.pts + 2 * (int64_t)(c.off[j] + f1 - c.sf[j]), c.X + 3 * (int64_t)j);
            c.state[j] = 1;
        }
    }
    __syncthreads();
}

// the cost of (camR, camt, X) into lm->cost (or cost2); with full, the linearisation as well: per observation Jc, Jp, r, W; per track
// Hpp, gp; per frame Hcc, gc; returns (to thread 0, in *gmax) the gradient's largest entry
__device__ void ba_eval(const Ctx &c, const double *camR, const double *camt, const double *X, bool full, double *cost, double *gmax) {
    const int F = c.F;
    for (int j = c.tid; j < c.nt; j += NT) {
        if (!c.state[j]) continue;
        double *T = c.trk + (int64_t)TR * j;
        double Hpp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0}, cj = 0.0;
        for (int o = c.off[j]; o < c.off[j + 1]; ++o) {
            const int f = c.sf[j] + o - c.off[j];
            double r[2], Xc[3], RX[3];
            residual(camR + 9 * f, camt + 3 * f, X + 3 * (int64_t)j, c.pts + 2 * (int64_t)o, r, Xc, RX);
            cj = cj + (r[0] * r[0] + r[1] * r[1]);
            if (!full) continue;
            double *O = c.obs + (int64_t)OB * o;
            double Jc[12], Jpr[6], Jp[6];
            jac_cam(Xc, RX, Jc, Jpr);
            const double *R = camR + 9 * f;
            for (int x = 0; x < 2; ++x)
                for (int y = 0; y < 3; ++y) Jp[3 * x + y] = (Jpr[3 * x] * R[y] + Jpr[3 * x + 1] * R[3 + y]) + Jpr[3 * x + 2] * R[6 + y];
            for (int k = 0; k < 12; ++k) O[k] = Jc[k];
            for (int k = 0; k < 6; ++k) O[12 + k] = Jp[k];
            O[18] = r[0]; O[19] = r[1];
            for (int x = 0; x < 6; ++x)
                for (int y = 0; y < 3; ++y) O[20 + 3 * x + y] = Jc[x] * Jp[y] + Jc[6 + x] * Jp[3 + y];
            for (int x = 0; x < 3; ++x) {
                for (int y = 0; y < 3; ++y) Hpp[3 * x + y] += Jp[x] * Jp[y] + Jp[3 + x] * Jp[3 + y];
                gp[x] += Jp[x] * r[0] + Jp[3 + x] * r[1];
            }
        }
        T[27] = cj;
        if (full) {
            for (int k = 0; k < 9; ++k) T[k] = Hpp[k];
            for (int k = 0; k < 3; ++k) T[18 + k] = gp[k];
            T[28] = fmax(fabs(gp[0]), fmax(fabs(gp[1]), fabs(gp[2])));
        }
    }
    __syncthreads();
    if (full)
        for (int e = c.tid; e < 42 * F; e += NT) {
            const int f = e / 42, k = e % 42;
            double s = 0.0;
            for (int j = 0; j < c.nt; ++j) {
                if (!c.state[j] || !has_frame(c.sf[j], c.off[j + 1] - c.off[j], f)) continue;
                const double *O = c.obs + (int64_t)OB * (c.off[j] + f - c.sf[j]);
                if (k < 36) s += O[k / 6] * O[k % 6] + O[6 + k / 6] * O[6 + k % 6];
                else s += O[k - 36] * O[18] + O[6 + k - 36] * O[19];
            }
            if (k < 36) c.Hcc[36 * f + k] = s;
            else c.gc[6 * f + k - 36] = s;
        }
    if (c.tid == 0) {
        double s = 0.0, gm = 0.0;
        for (int j = 0; j < c.nt; ++j)
            if (c.state[j]) {
                s = s + c.trk[(int64_t)TR * j + 27];
                if (full) gm = fmax(gm, c.trk[(int64_t)TR * j + 28]);
            }
        *cost = 0.5 * s;
        *gmax = gm;
    }
    __syncthreads();
    if (full && c.tid == 0) {
        double gm = *gmax;
        for (int k = 0; k < 6 * F; ++k) {
            const int f = k / 6;
            const bool cst = f == c.l || (f == F - 1 && k % 6 >= 3);
            if (!cst) gm = fmax(gm, fabs(c.gc[k]));
        }
        *gmax = gm;
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void k_sfm_construct(SfmArgs a) {
    extern __shared__ double lds[];
    const SfmWin W = a.wins[blockIdx.x];
    const int tid = threadIdx.x, F = W.F, nt = W.nt, n = 6 * F;
    const double *rel = a.rel + (int64_t)REL * blockIdx.x;
    double *o = a.out + (int64_t)OUTC * blockIdx.x;
    double *po = a.pts_out + 4 * W.o_trk;
    __shared__ Lm lm_s;
    __shared__ double s_gmax, s_h28[PC], s_sum[6];

    Ctx c;
    c.tid = tid; c.F = F; c.nt = nt;
    c.sf = a.ints + W.o_int; c.off = c.sf + nt;
    c.pts = a.dd + W.o_pts;
    double *scr = a.scr + W.o_scr;
    c.X = scr + 4 * (int64_t)nt; c.X2 = c.X + 3 * (int64_t)nt; c.trk = c.X2 + 3 * (int64_t)nt;
    c.obs = c.trk + (int64_t)TR * nt; c.pc = c.obs + (int64_t)OB * W.nobs;
    c.state = a.iscr + W.o_iscr; c.list = c.state + nt;
    c.S = lds; c.rhs = c.S + tri(n); c.dc = c.rhs + n; c.Dc = c.dc + n; c.gc = c.Dc + n; c.Hcc = c.gc + n;
    c.camR = c.Hcc + 36 * F; c.camt = c.camR + 9 * F; c.camR2 = c.camt + 3 * F; c.camt2 = c.camR2 + 9 * F;
    c.h28 = s_h28; c.lm = &lm_s;
    Lm *lm = &lm_s;

    // outputs start as a failed window's: NaN poses and points
    for (int k = tid; k < OUTC; k += NT) o[k] = k < 7 ? 0.0 : (k < 7 + 7 * MAXF ? NAN : 0.0);
    for (int j = tid; j < nt; j += NT) { po[4 * j] = NAN; po[4 * j + 1] = NAN; po[4 * j + 2] = NAN; po[4 * j + 3] = 0.0; c.state[j] = 0; }
    int status = (int)rel[0];
    const int l = (int)rel[1];
    c.l = l;
    int bad = 0;
    for (int k = tid; k < 2 * W.nobs; k += NT) bad |= !isfinite(c.pts[k]);
    if (status == VIO_OK && tid < 12) bad |= !isfinite(rel[6 + tid]);
    bad = __syncthreads_or(bad);
    if (bad) status = VIO_ERR_NOT_FINITE;
    if (status != VIO_OK) {
        if (tid == 0) { o[0] = status; o[1] = -1; o[5] = NAN; o[6] = NAN; }
        return;
    }
    if (tid == 0) {
        for (int f = 0; f < F; ++f) {
            for (int k = 0; k < 9; ++k) c.camR[9 * f + k] = 0.0;
            for (int k = 0; k < 3; ++k) c.camt[3 * f + k] = 0.0;
        }
        c.camR[9 * l] = 1.0; c.camR[9 * l + 4] = 1.0; c.camR[9 * l + 8] = 1.0;
        double q[4], Rq[9];
        rot_to_quat(rel + 6, q);
        quat_to_rot(q, Rq);
        double *R = c.camR + 9 * (F - 1), *t = c.camt + 3 * (F - 1);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) R[3 * r + k] = Rq[3 * k + r];
        for (int r = 0; r < 3; ++r) t[r] = -((R[3 * r] * rel[15] + R[3 * r + 1] * rel[16]) + R[3 * r + 2] * rel[17]);
    }
    __syncthreads();
    // the chains (initial_sfm.cpp:161-210)
    int fail = -1;
    for (int i = l; i < F - 1 && fail < 0; ++i) {
        if (i > l && !pnp(c, i, i - 1, o + 7 + 7 * MAXF + i)) { fail = i; break; }
        tri_two(c, i, F - 1);
    }
    for (int i = l + 1; i < F - 1 && fail < 0; ++i) tri_two(c, l, i);
    for (int i = l - 1; i >= 0 && fail < 0; --i) {
        if (!pnp(c, i, i + 1, o + 7 + 7 * MAXF + i)) { fail = i; break; }
        tri_two(c, i, l);
    }
    if (fail >= 0) {
        if (tid == 0) { o[0] = VIO_SFM_FAIL_PNP; o[1] = fail; o[5] = NAN; o[6] = NAN; }
        return;
    }
    for (int j = tid; j < nt; j += NT) {
        const int len = c.off[j + 1] - c.off[j];
        if (!c.state[j] && len >= 2) {
            const int f0 = c.sf[j], f1 = c.sf[j] + len - 1;
            triangulate(c.camR + 9 * f0, c.camt + 3 * f0, c.camR + 9 * f1, c.camt + 3 * f1, c.pts + 2 * (int64_t)c.off[j],
                        c.pts + 2 * (int64_t)(c.off[j + 1] - 1), c.X + 3 * (int64_t)j);
            c.state[j] = 1;
        }
    }
    __syncthreads();                // (every track has read the chains' rotations before they are re-normalised)
    if (tid < F) {                  // c_Quat = c_Rotation: the BA starts from the quaternions' rotations
        double q[4];
        rot_to_quat(c.camR + 9 * tid, q);
        const double nq = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        for (int k = 0; k < 4; ++k) q[k] = q[k] / nq;
        quat_to_rot(q, c.camR + 9 * tid);
    }
    __syncthreads();

    // ---- bundle adjustment ----
    ba_eval(c, c.camR, c.camt, c.X, true, &lm->cost, &s_gmax);
    if (tid == 0) {
        lm->c0 = lm->cost;
        lm->radius = VIO_SFM_LM_INITIAL_RADIUS; lm->v = 2.0; lm->it = 0; lm->stop = 0; lm->converged = 0;
        if (!isfinite(lm->cost)) lm->stop = 1;
        else if (s_gmax <= VIO_SFM_BA_GRADIENT_TOL) { lm->stop = 1; lm->converged = 1; }
    }
    __syncthreads();
    for (;;) {
        const bool go = !lm->stop && lm->it < VIO_SFM_BA_MAX_ITER;
        __syncthreads();             // (every thread has read the flags before thread 0 moves them)
        if (!go) break;
        if (tid == 0) { lm->it += 1; lm->lam = 1.0 / lm->radius; lm->ok = 1; }
        __syncthreads();
        const double lam = lm->lam;
        // point blocks: Hinv = (Hpp + lam Dp)^-1, Y = W Hinv
        for (int j = tid; j < nt; j += NT) {
            if (!c.state[j]) continue;
            double *T = c.trk + (int64_t)TR * j;
            double H[9];
            for (int k = 0; k < 9; ++k) H[k] = T[k];
            for (int k = 0; k < 3; ++k) {
                const double d = fmin(fmax(H[4 * k], LM_DIAG_MIN), LM_DIAG_MAX);
                T[21 + k] = d;
                H[4 * k] = H[4 * k] + lam * d;
            }
            const double A = H[0], B = H[1], C = H[2], D = H[4], E = H[5], G = H[8];
            const double c00 = D * G - E * E, c01 = C * E - B * G, c02 = B * E - C * D, c11 = A * G - C * C, c12 = B * C - A * E,
                         c22 = A * D - B * B;
            const double idet = 1.0 / ((A * c00 + B * c01) + C * c02);
            const double Hi[9] = {c00 * idet, c01 * idet, c02 * idet, c01 * idet, c11 * idet, c12 * idet, c02 * idet, c12 * idet, c22 * idet};
            for (int k = 0; k < 9; ++k) T[9 + k] = Hi[k];
            for (int ob = c.off[j]; ob < c.off[j + 1]; ++ob) {
                double *O = c.obs + (int64_t)OB * ob;
                for (int x = 0; x < 6; ++x)
                    for (int y = 0; y < 3; ++y)
                        O[38 + 3 * x + y] = (O[20 + 3 * x] * Hi[y] + O[20 + 3 * x + 1] * Hi[3 + y]) + O[20 + 3 * x + 2] * Hi[6 + y];
            }
        }
        if (tid < n) c.Dc[tid] = fmin(fmax(c.Hcc[36 * (tid / 6) + 7 * (tid % 6)], LM_DIAG_MIN), LM_DIAG_MAX);
        __syncthreads();
        // the reduced system: lower triangle and right-hand side, each entry over its tracks in track order
        for (int e = tid; e < n * n + n; e += NT) {
            if (e < n * n) {
                const int row = e / n, col = e % n;
                if (col > row) continue;
                const int f1 = row / 6, x = row % 6, f2 = col / 6, y = col % 6;
                const bool c1 = f1 == l || (f1 == F - 1 && x >= 3), c2 = f2 == l || (f2 == F - 1 && y >= 3);
                double s;
                if (c1 || c2) s = row == col ? 1.0 : 0.0;
                else {
                    s = f1 == f2 ? c.Hcc[36 * f1 + 6 * x + y] : 0.0;
                    if (row == col) s = s + lam * c.Dc[row];
                    for (int j = 0; j < nt; ++j) {
                        const int len = c.off[j + 1] - c.off[j];
                        if (!c.state[j] || !has_frame(c.sf[j], len, f1) || !has_frame(c.sf[j], len, f2)) continue;
                        const double *Y = c.obs + (int64_t)OB * (c.off[j] + f1 - c.sf[j]) + 38 + 3 * x;
                        const double *Wm = c.obs + (int64_t)OB * (c.off[j] + f2 - c.sf[j]) + 20 + 3 * y;
                        s = s - ((Y[0] * Wm[0] + Y[1] * Wm[1]) + Y[2] * Wm[2]);
                    }
                }
                c.S[tri(row) + col] = s;
            } else {
                const int row = e - n * n, f1 = row / 6, x = row % 6;
                const bool c1 = f1 == l || (f1 == F - 1 && x >= 3);
                double s = 0.0;
                if (!c1) {
                    s = -c.gc[row];
                    for (int j = 0; j < nt; ++j) {
                        if (!c.state[j] || !has_frame(c.sf[j], c.off[j + 1] - c.off[j], f1)) continue;
                        const double *Y = c.obs + (int64_t)OB * (c.off[j] + f1 - c.sf[j]) + 38 + 3 * x;
                        const double *gp = c.trk + (int64_t)TR * j + 18;
                        s = s + ((Y[0] * gp[0] + Y[1] * gp[1]) + Y[2] * gp[2]);
                    }
                }
                c.rhs[row] = s;
            }
        }
        __syncthreads();
        // Cholesky, column by column
        for (int j = 0; j < n; ++j) {
            if (tid == 0) {
                double d = 0.0;
                for (int k = 0; k < j; ++k) d += c.S[tri(j) + k] * c.S[tri(j) + k];
                d = c.S[tri(j) + j] - d;
                if (!(d > 0.0)) lm->ok = 0;
                c.S[tri(j) + j] = sqrt(d);
            }
            __syncthreads();
            if (!lm->ok) break;
            for (int i = j + 1 + tid; i < n; i += NT) {
                double s = 0.0;
                for (int k = 0; k < j; ++k) s += c.S[tri(i) + k] * c.S[tri(j) + k];
                c.S[tri(i) + j] = (c.S[tri(i) + j] - s) / c.S[tri(j) + j];
            }
            __syncthreads();
        }
        if (lm->ok) {
            if (tid == 0) {
                for (int i = 0; i < n; ++i) {           // y into dc, then x in place
                    double s = 0.0;
                    for (int k = 0; k < i; ++k) s += c.S[tri(i) + k] * c.dc[k];
                    c.dc[i] = (c.rhs[i] - s) / c.S[tri(i) + i];
                }
                for (int i = n - 1; i >= 0; --i) {
                    double s = 0.0;
                    for (int k = i + 1; k < n; ++k) s += c.S[tri(k) + i] * c.dc[k];
                    c.dc[i] = (c.dc[i] - s) / c.S[tri(i) + i];
                }
            }
            __syncthreads();
            // back substitution of the points, the trial state and the per-track terms of the step's norms
            for (int j = tid; j < nt; j += NT) {
                if (!c.state[j]) continue;
                double *T = c.trk + (int64_t)TR * j;
                double acc[3] = {0, 0, 0};
                for (int ob = c.off[j]; ob < c.off[j + 1]; ++ob) {
                    const double *Wm = c.obs + (int64_t)OB * ob + 20;
                    const double *d = c.dc + 6 * (c.sf[j] + ob - c.off[j]);
                    for (int y = 0; y < 3; ++y) {
                        double s = 0.0;
                        for (int x = 0; x < 6; ++x) s += Wm[3 * x + y] * d[x];
                        acc[y] += s;
                    }
                }
                double dp[3];
                for (int x = 0; x < 3; ++x) {
                    const double *Hi = T + 9 + 3 * x;
                    dp[x] = (Hi[0] * (-T[18] - acc[0]) + Hi[1] * (-T[19] - acc[1])) + Hi[2] * (-T[20] - acc[2]);
                }
                const double *Xj = c.X + 3 * (int64_t)j;
                for (int k = 0; k < 3; ++k) { T[24 + k] = dp[k]; c.X2[3 * (int64_t)j + k] = Xj[k] + dp[k]; }
                T[29] = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2];
                T[30] = (Xj[0] * Xj[0] + Xj[1] * Xj[1]) + Xj[2] * Xj[2];
                T[31] = (dp[0] * T[18] + dp[1] * T[19]) + dp[2] * T[20];
                T[32] = ((dp[0] * T[21]) * dp[0] + (dp[1] * T[22]) * dp[1]) + (dp[2] * T[23]) * dp[2];
            }
            if (tid < F) {
                double E[9];
                exp_so3(c.dc + 6 * tid, E);
                mm3(E, c.camR + 9 * tid, c.camR2 + 9 * tid);
                for (int k = 0; k < 3; ++k) c.camt2[3 * tid + k] = c.camt[3 * tid + k] + c.dc[6 * tid + 3 + k];
            }
            __syncthreads();
            if (tid < 4) {          // d2, x2, gdot, ddd over the tracks, in track order
                double s = 0.0;
                for (int j = 0; j < nt; ++j)
                    if (c.state[j]) s = s + c.trk[(int64_t)TR * j + 29 + tid];
                s_sum[tid] = s;
            }
            __syncthreads();
            if (tid == 0) {
                double xq = 0.0, xt = 0.0;
                for (int f = 0; f < F; ++f) {
                    double q[4];
                    rot_to_quat(c.camR + 9 * f, q);
                    xq = xq + (((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
                    xt = xt + ((c.camt[3 * f] * c.camt[3 * f] + c.camt[3 * f + 1] * c.camt[3 * f + 1]) + c.camt[3 * f + 2] * c.camt[3 * f + 2]);
                }
                const double x2 = (xq + xt) + s_sum[1];
                double dcc = 0.0, gd = 0.0, ddd = 0.0;
                for (int k = 0; k < n; ++k) { dcc += c.dc[k] * c.dc[k]; gd += c.dc[k] * c.gc[k]; ddd += (c.dc[k] * c.Dc[k]) * c.dc[k]; }
                const double d2 = dcc + s_sum[0];
                if (sqrt(d2) <= VIO_SFM_BA_PARAMETER_TOL * (sqrt(x2) + VIO_SFM_BA_PARAMETER_TOL)) { lm->stop = 1; lm->converged = 1; }
                lm->rho = 0.5 * (lam * (ddd + s_sum[3]) - (gd + s_sum[2]));     // the model's decrease
            }
            __syncthreads();
            if (lm->stop) break;
            ba_eval(c, c.camR2, c.camt2, c.X2, false, &lm->cost2, &s_gmax);
        }
        if (tid == 0) {
            bool take = false;
            if (lm->ok) {
                const double model = lm->rho;
                lm->rho = (isfinite(lm->cost2) && model > 0) ? (lm->cost - lm->cost2) / model : -1.0;
                take = lm->rho > LM_MIN_RHO;
            }
            lm->ok = take;
            if (!take) {
                lm->radius = lm->radius / lm->v;
                lm->v = lm->v * 2.0;
                if (lm->radius < LM_RADIUS_MIN) lm->stop = 1;
            }
        }
        __syncthreads();
        if (lm->ok) {
            for (int k = tid; k < 9 * F; k += NT) c.camR[k] = c.camR2[k];
            for (int k = tid; k < 3 * F; k += NT) c.camt[k] = c.camt2[k];
            for (int j = tid; j < nt; j += NT)
                if (c.state[j])
                    for (int k = 0; k < 3; ++k) c.X[3 * (int64_t)j + k] = c.X2[3 * (int64_t)j + k];
            __syncthreads();
            if (tid == 0) lm->prev = lm->cost;
            ba_eval(c, c.camR, c.camt, c.X, true, &lm->cost, &s_gmax);
            if (tid == 0) {
                if (s_gmax <= VIO_SFM_BA_GRADIENT_TOL) { lm->stop = 1; lm->converged = 1; }
                else if (fabs(lm->prev - lm->cost) <= VIO_SFM_BA_FUNCTION_TOL * lm->prev) { lm->stop = 1; lm->converged = 1; }
                else { lm->radius = lm_radius(lm->radius, lm->rho); lm->v = 2.0; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // outputs
    int fin = isfinite(lm->cost) != 0;
    for (int k = tid; k < 9 * F; k += NT) fin &= isfinite(c.camR[k]) != 0;
    for (int k = tid; k < 3 * F; k += NT) fin &= isfinite(c.camt[k]) != 0;
    fin = !__syncthreads_or(!fin);
    const bool good = fin && (lm->converged || lm->cost < BA_COST_OK);
    if (tid == 0) {
        int ntri = 0;
        for (int j = 0; j < nt; ++j) ntri += c.state[j];
        o[0] = !fin ? VIO_ERR_NOT_FINITE : (good ? VIO_OK : VIO_SFM_FAIL_BA);
        o[1] = -1; o[2] = lm->it; o[3] = lm->converged; o[4] = ntri; o[5] = lm->c0; o[6] = lm->cost;
    }
    for (int j = tid; j < nt; j += NT) {
        po[4 * j + 3] = c.state[j];
        if (good && c.state[j])
            for (int k = 0; k < 3; ++k) po[4 * j + k] = c.X[3 * (int64_t)j + k];
    }
    if (good && tid < F) {          // q[i] = c_Quat.inverse(), T[i] = -(q[i] * c_translation[i]) (initial_sfm.cpp:288-300)
        const double *R = c.camR + 9 * tid, *t = c.camt + 3 * tid;
        const double Rt[9] = {R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]};
        rot_to_quat(Rt, o + 7 + 4 * tid);
        for (int r = 0; r < 3; ++r) o[7 + 4 * MAXF + 3 * tid + r] = -((Rt[3 * r] * t[0] + Rt[3 * r + 1] * t[1]) + Rt[3 * r + 2] * t[2]);
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_sfm {
    int device = 0;
    ErrText err = {0};
    vio_sfm_config cfg = {0u, VIO_SFM_DEFAULT_HYPOTHESES};
    Twin<char> staging;                                  // descriptors | int32 | doubles
    DevBuf<double> scr;
    DevBuf<int32_t> iscr;
    Twin<double> rel, out, pts_out;
    Twin<int32_t> mask;
    StreamEvents<4> q;                                   // events: upload start, stage 1 start, stage 2 start, end
    double timing[4] = {NAN, NAN, NAN, NAN};
};

namespace {

size_t lds_bytes(int F) {
    const size_t n = 6 * (size_t)F;
    return sizeof(double) * (n * (n + 1) / 2 + 4 * n + 36 * (size_t)F + 24 * (size_t)F);     // S | rhs, dc, Dc, gc | Hcc | camR, camt, camR2, camt2
}

vio_status check_item(vio_sfm *h, int i, const vio_sfm_item &it) {
    if (it.n_frames < 3 || it.n_frames > VIO_SFM_MAX_FRAMES)
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: n_frames must be in [3, %d]", i, VIO_SFM_MAX_FRAMES);
    if (it.n_tracks < 0 || it.n_tracks > VIO_SFM_MAX_TRACKS)
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: n_tracks must be in [0, %d]", i, VIO_SFM_MAX_TRACKS);
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
    size_t b_desc = 0, b_int = 0, bytes = 0;
    int64_t scr = 0, iscr = 0, tracks = 0;
    int fmax = 3;
};

vio_status stage(vio_sfm *h, int count, const vio_sfm_item *items, Staged &s) {
    for (int i = 0; i < count; ++i) {
        const vio_status st = check_item(h, i, items[i]);
        if (st != VIO_OK) return st;
    }
    s.b_desc = align256(sizeof(SfmWin) * (size_t)count);
    int64_t ni = 0, nd = 0;
    std::vector<SfmWin> wins((size_t)count);
    for (int i = 0; i < count; ++i) {
        SfmWin &w = wins[(size_t)i];
        std::memset(&w, 0, sizeof(w));
        w.F = items[i].n_frames; w.nt = items[i].n_tracks; w.nobs = (int32_t)items[i].obs_offset[w.nt];
        w.o_int = ni; ni += 2 * (int64_t)w.nt + 1;
        w.o_pts = nd; nd += 2 * (int64_t)w.nobs;
        w.o_scr = s.scr; s.scr += (int64_t)(4 + 3 + 3 + TR + PC) * w.nt + (int64_t)OB * w.nobs;
        w.o_iscr = s.iscr; s.iscr += 3 * (int64_t)w.nt;
        w.o_trk = s.tracks; s.tracks += w.nt;
        if (w.F > s.fmax) s.fmax = w.F;
    }
    s.b_int = align256(sizeof(int32_t) * (size_t)ni);
    s.bytes = s.b_desc + s.b_int + sizeof(double) * (size_t)nd;
    const vio_status st = h->staging.ensure(h->err, s.bytes);
    if (st != VIO_OK) return st;
    std::memcpy(h->staging.h, wins.data(), sizeof(SfmWin) * (size_t)count);
    int32_t *hi = (int32_t *)(h->staging.h + s.b_desc);
    double *hd = (double *)(h->staging.h + s.b_desc + s.b_int);
    for (int i = 0; i < count; ++i) {
        const vio_sfm_item &it = items[i];
        const SfmWin &w = wins[(size_t)i];
        for (int j = 0; j < w.nt; ++j) hi[w.o_int + j] = it.start_frame[j];
        for (int j = 0; j <= w.nt; ++j) hi[w.o_int + w.nt + j] = (int32_t)it.obs_offset[j];
        if (w.nobs) std::memcpy(hd + w.o_pts, it.pts, sizeof(double) * 2 * (size_t)w.nobs);
    }
    return VIO_OK;
}

void unpack_rel(const double *o, vio_sfm_rel_result &r) {
    r.status = (int32_t)o[0]; r.l = (int32_t)o[1]; r.hyp = (int32_t)o[2]; r.n_corres = (int32_t)o[3];
    r.n_inliers = (int32_t)o[4]; r.n_front = (int32_t)o[5];
    for (int k = 0; k < 9; ++k) r.R[k] = o[6 + k];
    for (int k = 0; k < 3; ++k) r.T[k] = o[15 + k];
    for (int k = 0; k < MAXF; ++k) { r.corres[k] = (int32_t)o[18 + k]; r.parallax[k] = o[18 + MAXF + k]; }
}

void pack_rel(const vio_sfm_rel_result &r, double *o) {
    o[0] = r.status; o[1] = r.l; o[2] = r.hyp; o[3] = r.n_corres; o[4] = r.n_inliers; o[5] = r.n_front;
    for (int k = 0; k < 9; ++k) o[6 + k] = r.R[k];
    for (int k = 0; k < 3; ++k) o[15 + k] = r.T[k];
    for (int k = 0; k < MAXF; ++k) { o[18 + k] = r.corres[k]; o[18 + MAXF + k] = r.parallax[k]; }
}

// the three entry points: stage 1 (do1), stage 2 (do2) or both
vio_status run(vio_sfm *h, const char *name, int32_t count, const vio_sfm_item *items, bool do1, bool do2, const vio_sfm_rel_result *rel_in,
               vio_sfm_rel_result *rel_out, uint8_t *mask, vio_sfm_result *res, double *points, uint8_t *state) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || (count > 0 && (!items || (do1 && !do2 && !rel_out) || (do2 && !do1 && !rel_in) || (do2 && !res))))
        return fail(h->err, VIO_ERR_BAD_ARG, "%s: negative count or a NULL array", name);
    if (count == 0) return VIO_OK;
    if (rel_in)
        for (int i = 0; i < count; ++i)
            if (rel_in[i].status == VIO_OK && (rel_in[i].l < 0 || rel_in[i].l >= items[i].n_frames - 1))
                return fail(h->err, VIO_ERR_BAD_ARG, "window %d: l must be in [0, n_frames - 2]", i);
    const auto t0 = std::chrono::steady_clock::now();
    DeviceScope dev(h->device);                     // before stage(): its buffers belong on the handle's device
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    Staged s;
    vio_status st = stage(h, count, items, s);
    if (st != VIO_OK) return st;
    const size_t relb = sizeof(double) * REL * (size_t)count, outb = sizeof(double) * OUTC * (size_t)count;
    const size_t ptsb = sizeof(double) * 4 * (size_t)(s.tracks + 1), maskb = sizeof(int32_t) * (size_t)(s.iscr + 1);
    if ((st = h->rel.ensure(h->err, relb)) != VIO_OK || (st = h->out.ensure(h->err, outb)) != VIO_OK ||
        (st = h->pts_out.ensure(h->err, ptsb)) != VIO_OK || (st = h->mask.ensure(h->err, maskb)) != VIO_OK ||
        (st = h->scr.ensure(h->err, sizeof(double) * (size_t)(s.scr + 1))) != VIO_OK ||
        (st = h->iscr.ensure(h->err, sizeof(int32_t) * (size_t)(s.iscr + 1))) != VIO_OK)
        return st;
    if (rel_in)
        for (int i = 0; i < count; ++i) pack_rel(rel_in[i], h->rel.h + (size_t)REL * i);
    SfmArgs a;
    a.wins = (const SfmWin *)h->staging.d;
    a.ints = (const int32_t *)(h->staging.d + s.b_desc);
    a.dd = (const double *)(h->staging.d + s.b_desc + s.b_int);
    a.scr = h->scr.d; a.iscr = h->iscr.d; a.rel = h->rel.d; a.out = h->out.d; a.pts_out = h->pts_out.d;
    a.seed = h->cfg.seed; a.hyps = h->cfg.ransac_hypotheses;
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->staging.d, h->staging.h, s.bytes, hipMemcpyHostToDevice, q) != hipSuccess ||
        (rel_in && hipMemcpyAsync(h->rel.d, h->rel.h, relb, hipMemcpyHostToDevice, q) != hipSuccess))
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    if (do1) hipLaunchKernelGGL(k_sfm_relpose, dim3(count), dim3(NT), 0, q, a);
    (void)hipEventRecord(h->q.ev[2], q);
    if (do2) hipLaunchKernelGGL(k_sfm_construct, dim3(count), dim3(NT), lds_bytes(s.fmax), q, a);
    (void)hipEventRecord(h->q.ev[3], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    bool okc = true;
    if (do1) {
        okc = okc && hipMemcpyAsync(h->rel.h, h->rel.d, relb, hipMemcpyDeviceToHost, q) == hipSuccess;
        if (mask) okc = okc && hipMemcpyAsync(h->mask.h, h->iscr.d, sizeof(int32_t) * (size_t)s.iscr, hipMemcpyDeviceToHost, q) == hipSuccess;
    }
    if (do2) {
        okc = okc && hipMemcpyAsync(h->out.h, h->out.d, outb, hipMemcpyDeviceToHost, q) == hipSuccess;
        okc = okc && hipMemcpyAsync(h->pts_out.h, h->pts_out.d, sizeof(double) * 4 * (size_t)s.tracks, hipMemcpyDeviceToHost, q) == hipSuccess;
    }
    if (!okc || hipStreamSynchronize(q) != hipSuccess) return fail_synced(h, "kernel or read-back failed");
    vio_status ret = VIO_OK;
    int64_t trk = 0, isc = 0;
    for (int i = 0; i < count; ++i) {
        const int nt = items[i].n_tracks;
        if (do1) {
            vio_sfm_rel_result r;
            unpack_rel(h->rel.h + (size_t)REL * i, r);
            if (rel_out) rel_out[i] = r;
            if (mask)
                for (int j = 0; j < nt; ++j) mask[trk + j] = (uint8_t)(h->mask.h[isc + 2 * (int64_t)nt + j] != 0);
            if (r.status == VIO_ERR_NOT_FINITE) ret = VIO_ERR_NOT_FINITE;
        }
        if (do2) {
            const double *o = h->out.h + (size_t)OUTC * i;
            vio_sfm_result &r = res[i];
            r.status = (int32_t)o[0]; r.fail_frame = (int32_t)o[1]; r.ba_iterations = (int32_t)o[2]; r.ba_converged = (int32_t)o[3];
            r.n_triangulated = (int32_t)o[4]; r.initial_cost = o[5]; r.final_cost = o[6];
            std::memcpy(r.Q, o + 7, sizeof(double) * 4 * MAXF);
            std::memcpy(r.T, o + 7 + 4 * MAXF, sizeof(double) * 3 * MAXF);
            for (int k = 0; k < MAXF; ++k) r.pnp_iterations[k] = (int32_t)o[7 + 7 * MAXF + k];
            for (int j = 0; j < nt; ++j) {
                const double *p = h->pts_out.h + 4 * (size_t)(trk + j);
                if (points) std::memcpy(points + 3 * (size_t)(trk + j), p, sizeof(double) * 3);
                if (state) state[trk + j] = (uint8_t)(p[3] != 0.0);
            }
            if (r.status == VIO_ERR_NOT_FINITE) ret = VIO_ERR_NOT_FINITE;
        }
        if (ret == VIO_ERR_NOT_FINITE && !h->err[0]) fail(h->err, ret, "window %d: non-finite input or result", i);
        trk += nt;
        isc += 3 * (int64_t)nt;
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

int32_t vio_sfm_version(void) { return VIO_SFM_VERSION; }

const char *vio_sfm_last_error(const vio_sfm *h) { return h ? h->err : "NULL handle"; }

vio_status vio_sfm_create(int32_t device, void *stream, vio_sfm **out) {
    return create_handle(device, stream, out, vio_sfm_destroy, [](vio_sfm *) {
        return hipFuncSetAttribute((const void *)k_sfm_construct, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(MAXF)) == hipSuccess;
    });
}

void vio_sfm_destroy(vio_sfm *h) { destroy_handle(h); }

vio_status vio_sfm_set_config(vio_sfm *h, const vio_sfm_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg || cfg->ransac_hypotheses < 1 || cfg->ransac_hypotheses > VIO_SFM_MAX_HYPOTHESES)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_sfm_set_config: ransac_hypotheses must be in [1, %d]", VIO_SFM_MAX_HYPOTHESES);
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_sfm_timing(const vio_sfm *h, double *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_sfm_relative_pose_batch(vio_sfm *h, int32_t count, const vio_sfm_item *items, vio_sfm_rel_result *rel, uint8_t *mask) {
    return run(h, "vio_sfm_relative_pose_batch", count, items, true, false, nullptr, rel, mask, nullptr, nullptr, nullptr);
}

vio_status vio_sfm_construct_batch(vio_sfm *h, int32_t count, const vio_sfm_item *items, const vio_sfm_rel_result *rel,
                                   vio_sfm_result *res, double *points, uint8_t *state) {
    return run(h, "vio_sfm_construct_batch", count, items, false, true, rel, nullptr, nullptr, res, points, state);
}

vio_status vio_sfm_batch(vio_sfm *h, int32_t count, const vio_sfm_item *items, vio_sfm_rel_result *rel_out, uint8_t *mask,
                         vio_sfm_result *res, double *points, uint8_t *state) {
    return run(h, "vio_sfm_batch", count, items, true, true, nullptr, rel_out, mask, res, points, state);
}

}  // extern "C"
