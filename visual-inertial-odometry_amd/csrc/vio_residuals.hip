// vio_residuals.hip — per-edge residuals, the chi2 breakdown and landmark outlier flags (include/vio_residuals.h; DESIGN.md
// section 11).
//
// A companion of libvio_hip.so that uses nothing but its C ABI: the states are read back through the getters, and the three kernels
// below run on the context's stream.
//   k_res_obs<D>  one thread per edge, in the caller's order: the reprojection residual, e2 and rho0, stored as one row of obs.
//   k_res_lm      one thread per landmark: its edges walked in CSR order -> mean / max pixel error, sum of rho0, flags; per-workgroup
//                 partials of the visual totals, the 11 frame sums and the flag counts (DPP wave sums, waves in order).
//   k_res_tail    one workgroup: the ten IMU residuals (the solver's d_imu_residual) and r^T Sigma^-1 r, the partials added in
//                 workgroup order, ||err_prior||, chi2.
// No atomics: every output is written by one thread, every sum has a fixed order, so a call is bitwise reproducible.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vio_device_math.h"
#include "vio_imu_math.h"
#include "vio_obs_csr.h"
#include "../../include/vio_residuals.h"

#define NF VIO_NUM_FRAMES                  // 11
#define NW VIO_WINDOW_SIZE                 // 10 IMU edges
#define PRD VIO_PRIOR_DIM                  // 156

#define OBS_NT 256
#define LM_NT 256
#define TAIL_NT 256

// per-workgroup partials of k_res_lm (doubles): visual_robust, visual_plain, frame_robust[11], frame_edges[11], flag counts[3]
#define P_VR 0
#define P_VP 1
#define P_FR 2
#define P_FE (P_FR + NF)
#define P_FL (P_FE + NF)
#define P_N (P_FL + 3)                     // 27
#define P_STRIDE 32
// the device summary (doubles): chi2, visual_robust, visual_plain, imu, prior, imu_edge[10], frame_robust[11], frame_edges[11], flags[3]
#define S_CHI 0
#define S_VR 1
#define S_VP 2
#define S_IMU 3
#define S_PRIOR 4
#define S_IMUE 5
#define S_FR (S_IMUE + NW)
#define S_FE (S_FR + NF)
#define S_FL (S_FE + NF)
#define S_N (S_FL + 3)                     // 43

// ---------------------------------------------------------------------------------------------------------------------------------
// k_res_obs<D>: D = 1 inverse depth (EdgeReprojection), D = 3 world point (EdgeReprojectionXYZ).
// ---------------------------------------------------------------------------------------------------------------------------------
struct ResArgs {
    const double *poses;       // [11][7]
    const double *sb;          // [11][9]
    const double *ext;         // [7]
    const double *errp;        // [156] err_prior
    const double *pre;         // [10][PRE_STRIDE] (PRE_INFO: the information, formed on the host)
    const int *pre_ok;         // [10] 1: the edge exists
    const double *val;         // [n][D] inverse depths / world points
    const double *pts_i;       // [m][2] (D = 1)
    const double *pts_j;       // [m][2] caller's order
    const int *lm;             // [m]
    const int *host;           // [m] (D = 1)
    const int *fr;             // [m] target frame (D = 1) / observing frame (D = 3)
    const int *off;            // [n + 1] CSR over the landmarks
    const int *eidx;           // [m] CSR slot -> edge
    long long m;
    int n;
    int n_wg;                  // workgroups of k_res_lm
    int loss_type;
    int have_pre;              // 0: the IMU terms (and chi2) are NaN
    double loss_delta;
    double sqrt_info;
    double focal;
    double outlier_px;
    double gravity[3];
    double *obs;               // [m][4] r_x, r_y, e2, rho0
    unsigned char *dneg;       // [m] 1: the point is at depth <= 0 in the observing camera
    double *lm_out;            // [n][3] mean px, max px, sum rho0
    unsigned char *flags;      // [n]
    double *part;              // [n_wg][P_STRIDE]
    double *sum;               // [S_N]
};

template <int D>
__global__ void __launch_bounds__(OBS_NT) k_res_obs(ResArgs a) {
    __shared__ double sR[(NF + 1) * 9];         // rotations of the 11 poses and (slot 11) of the extrinsic
    const int tid = threadIdx.x;
    for (int f = tid; f <= NF; f += OBS_NT) d_quat_to_R(f < NF ? a.poses + 7 * f + 3 : a.ext + 3, sR + 9 * f);
    __syncthreads();
    const long long e = (long long)blockIdx.x * OBS_NT + tid;
    if (e >= a.m) return;
    const int l = a.lm[e], fj = a.fr[e];
    double r[2], dep;
    if (D == 1) {
        const int fi = a.host[e];
        dep = d_reproj_residual(sR + 9 * fi, a.poses + 7 * fi, sR + 9 * fj, a.poses + 7 * fj, sR + 9 * NF, a.ext, a.val[l],
                                a.pts_i + 2 * e, a.pts_j + 2 * e, r);
    } else {
        dep = d_reproj_xyz_residual(sR + 9 * fj, a.poses + 7 * fj, sR + 9 * NF, a.ext, a.val + 3 * (size_t)l, a.pts_j + 2 * e, r);
    }
    const double info = a.sqrt_info * a.sqrt_info;
    const double e2 = r[0] * (info * r[0]) + r[1] * (info * r[1]);          // Edge::Chi2 (edge.cc:33-37)
    double r0, r1, r2;
    d_loss(a.loss_type, a.loss_delta, e2, r0, r1, r2);                       // RobustChi2: rho[0] (e2 itself without a loss)
    double2 *o = (double2 *)(a.obs + 4 * e);
    o[0] = make_double2(r[0], r[1]);
    o[1] = make_double2(e2, r0);
    a.dneg[e] = dep <= 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k_res_lm: per landmark statistics and flags; per-workgroup partials.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(LM_NT) k_res_lm(ResArgs a) {
    __shared__ double red[P_N * (LM_NT / 64)];
    const int tid = threadIdx.x;
    const int l = blockIdx.x * LM_NT + tid;
    double vr = 0.0, vp = 0.0, fr[NF], fe[NF], fl[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int f = 0; f < NF; ++f) { fr[f] = 0.0; fe[f] = 0.0; }
    if (l < a.n) {
        double spx = 0.0, mpx = 0.0, srho = 0.0;
        unsigned flag = 0;
        const int q0 = a.off[l], q1 = a.off[l + 1];
        for (int q = q0; q < q1; ++q) {
            const int e = a.eidx[q];
            const double2 *o = (const double2 *)(a.obs + 4 * (size_t)e);
            const double2 rr = o[0], er = o[1];
            const double px = a.focal * sqrt(rr.x * rr.x + rr.y * rr.y);
            spx += px;
            if (!isnan(mpx) && !(px <= mpx)) mpx = px;                      // max; a NaN sticks
            srho += er.y;
            vr += er.y;
            vp += er.x;
            const int f = a.fr[e];
#pragma unroll
            for (int k = 0; k < NF; ++k) {                       // (selects, not a register array indexed at run time)
                fr[k] += (f == k) ? er.y : 0.0;
                fe[k] += (f == k) ? 1.0 : 0.0;
            }
            if (a.dneg[e]) flag |= VIO_RES_FLAG_DEPTH;
        }
        const int cnt = q1 - q0;
        const double mean = cnt ? spx / cnt : 0.0;
        if (cnt && !(mean <= a.outlier_px)) flag |= VIO_RES_FLAG_REPROJ;
        if (D == 1) {
            const double lam = a.val[l];
            if (!(lam > 0.0) || !isfinite(lam)) flag |= VIO_RES_FLAG_STATE;
        } else {
            const double *p = a.val + 3 * (size_t)l;
            if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) flag |= VIO_RES_FLAG_STATE;
        }
        a.lm_out[3 * (size_t)l] = mean;
        a.lm_out[3 * (size_t)l + 1] = mpx;
        a.lm_out[3 * (size_t)l + 2] = srho;
        a.flags[l] = (unsigned char)flag;
#pragma unroll
        for (int k = 0; k < 3; ++k) fl[k] = (flag >> k) & 1u ? 1.0 : 0.0;
    }
    // workgroup partials: DPP sum inside each wave, the waves added in order
    const int w = tid >> 6;
    double v;
#define RES_WAVE_SUM(slot, x) v = d_wave_sum_to_lane63(x); if ((tid & 63) == 63) red[(slot) * (LM_NT / 64) + w] = v;
    RES_WAVE_SUM(P_VR, vr)
    RES_WAVE_SUM(P_VP, vp)
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        RES_WAVE_SUM(P_FR + k, fr[k])
        RES_WAVE_SUM(P_FE + k, fe[k])
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { RES_WAVE_SUM(P_FL + k, fl[k]) }
#undef RES_WAVE_SUM
    __syncthreads();
    if (tid < P_N) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < LM_NT / 64; ++k) s += red[tid * (LM_NT / 64) + k];
        a.part[(size_t)blockIdx.x * P_STRIDE + tid] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k_res_tail: one workgroup.  Wave 0 lanes 0..9: the IMU edges; every wave: some of the partial columns (lanes stride over the
// workgroups, then a DPP sum); wave 3: ||err_prior||.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TAIL_NT) k_res_tail(ResArgs a) {
    __shared__ double simu[NW];
    __shared__ double scol[P_N];
    __shared__ double sprior;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if (tid < NW) {
        const int k = tid;
        double chi = 0.0;
        if (!a.have_pre) chi = NAN;
        else if (a.pre_ok[k]) {
            const double *pre = a.pre + k * PRE_STRIDE;
            const double *pi = a.poses + 7 * k, *pj = pi + 7, *si = a.sb + 9 * k, *sj = si + 9;
            ImuCommon c;
            d_imu_common(pre, pi, si, pj, c);
            double r[15];
            d_imu_residual(pre, a.gravity, pi, si, pj, sj, c, r);
            for (int i = 0; i < 15; ++i) {                 // r^T Info r in the order of the solver's chi2 (d_backsub_imu_block)
                double t = 0;
                for (int j = 0; j < 15; ++j) t += pre[PRE_INFO + 15 * i + j] * r[j];
                chi += r[i] * t;
            }
        }
        simu[k] = chi;
    }
    for (int col = w; col < P_N; col += TAIL_NT / 64) {
        double s = 0.0;
        for (int b = lane; b < a.n_wg; b += 64) s += a.part[(size_t)b * P_STRIDE + col];
        s = d_wave_sum_to_lane63(s);
        if (lane == 63) scol[col] = s;
    }
    if (w == TAIL_NT / 64 - 1) {
        double s = 0.0;
        for (int i = lane; i < PRD; i += 64) s += a.errp[i] * a.errp[i];
        s = d_wave_sum_to_lane63(s);
        if (lane == 63) sprior = sqrt(s);
    }
    __syncthreads();
    if (tid == 0) {
        double imu = 0.0;
        for (int k = 0; k < NW; ++k) { imu += simu[k]; a.sum[S_IMUE + k] = simu[k]; }
        a.sum[S_VR] = scol[P_VR];
        a.sum[S_VP] = scol[P_VP];
        a.sum[S_IMU] = imu;
        a.sum[S_PRIOR] = sprior;
        a.sum[S_CHI] = 0.5 * (scol[P_VR] + (imu + sprior));         // vio_chi2: 0.5 * (visual + (imu + prior))
        for (int f = 0; f < NF; ++f) { a.sum[S_FR + f] = scol[P_FR + f]; a.sum[S_FE + f] = scol[P_FE + f]; }
        for (int k = 0; k < 3; ++k) a.sum[S_FL + k] = scol[P_FL + k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
struct vio_res {
    vio_ctx *ctx = nullptr;
    vio_config cfg;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    char err[512] = {0};
    // device: poses | sb | ext | errp | pre | val | pts_i | pts_j (doubles), then pre_ok | lm | host | fr | off | eidx (ints): one upload
    char *d_in = nullptr, *h_in = nullptr;          // (h_in: pinned, grows only)
    size_t in_cap = 0;
    // device: obs | lm_out | part | sum (doubles), then dneg | flags (bytes); the requested parts come back through h_out (pinned)
    char *d_out = nullptr, *h_out = nullptr;
    size_t out_cap = 0;
    double timing[5] = {0, 0, 0, 0, 0};
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

static vio_status fail(vio_res *rs, vio_status st, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(rs->err, sizeof(rs->err), fmt, ap);
    va_end(ap);
    return st;
}

static vio_status hip_ck(vio_res *rs, hipError_t e, const char *what) {
    if (e == hipSuccess) return VIO_OK;
    return fail(rs, VIO_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// grow a pinned host buffer and its device twin to hold `bytes` (never shrinks)
static vio_status ensure(vio_res *rs, char **d, char **h, size_t *cap, size_t bytes) {
    if (bytes <= *cap) return VIO_OK;
    if (*d) hipFree(*d);
    if (*h) hipHostFree(*h);
    *d = nullptr; *h = nullptr; *cap = 0;
    size_t want = bytes + bytes / 4 + 4096;
    vio_status st = hip_ck(rs, hipMalloc((void **)d, want), "hipMalloc");
    if (st != VIO_OK) return st;
    st = hip_ck(rs, hipHostMalloc((void **)h, want, hipHostMallocDefault), "hipHostMalloc");
    if (st != VIO_OK) return st;
    *cap = want;
    return VIO_OK;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// covariance.inverse() (edge_imu.cc:35): LU with partial pivoting of the 15 x 15, then the two triangular solves of the identity
static void inverse15(const double *cov, double *info) {
    double A[225];
    int piv[15];
    std::memcpy(A, cov, sizeof(A));
    for (int k = 0; k < 15; ++k) piv[k] = k;
    for (int k = 0; k < 15; ++k) {
        int p = k;
        for (int i = k + 1; i < 15; ++i)
            if (std::fabs(A[15 * i + k]) > std::fabs(A[15 * p + k])) p = i;
        if (p != k) {
            for (int j = 0; j < 15; ++j) std::swap(A[15 * k + j], A[15 * p + j]);
            std::swap(piv[k], piv[p]);
        }
        const double d = A[15 * k + k];
        if (d != 0.0)
            for (int i = k + 1; i < 15; ++i) A[15 * i + k] /= d;
        for (int i = k + 1; i < 15; ++i)
            for (int j = k + 1; j < 15; ++j) A[15 * i + j] -= A[15 * i + k] * A[15 * k + j];
    }
    for (int c = 0; c < 15; ++c) {                 // column c of the inverse: L U x = P e_c
        double x[15];
        for (int i = 0; i < 15; ++i) {
            double s = piv[i] == c ? 1.0 : 0.0;
            for (int j = 0; j < i; ++j) s -= A[15 * i + j] * x[j];
            x[i] = s;
        }
        for (int i = 14; i >= 0; --i) {
            double s = x[i];
            for (int j = i + 1; j < 15; ++j) s -= A[15 * i + j] * x[j];
            x[i] = s / A[15 * i + i];
        }
        for (int i = 0; i < 15; ++i) info[15 * i + c] = x[i];
    }
}

// D = 1: obs (host, target, pts_i, pts_j); D = 3: obs (frame, pts) in `target` / `pts_j`
static vio_status compute(vio_res *rs, int D, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                          const double *pts_i, const double *pts_j, int64_t n, const vio_preint *const *pre, double focal,
                          double outlier_px, double *obs_out, double *lm_out, uint8_t *lm_flags, vio_res_summary *summary) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    if (m < 0 || n < 0 || n >= INT32_MAX || m >= INT32_MAX) return fail(rs, VIO_ERR_BAD_ARG, "bad sizes m=%lld n=%lld", (long long)m, (long long)n);
    if (!(focal > 0.0)) return fail(rs, VIO_ERR_BAD_ARG, "focal %g is not positive", focal);
    if (m > 0 && (!lm || !target || !pts_j || (D == 1 && (!host || !pts_i)))) return fail(rs, VIO_ERR_BAD_ARG, "observation array is NULL");
    for (int64_t e = 0; e < m; ++e) {
        if (lm[e] < 0 || lm[e] >= n || target[e] < 0 || target[e] >= NF || (D == 1 && (host[e] < 0 || host[e] >= NF)))
            return fail(rs, VIO_ERR_BAD_ARG, "observation %lld refers to landmark %d / a frame out of range", (long long)e, lm[e]);
    }
    DeviceScope dev(rs->cfg.device);
    if (!dev.ok) return fail(rs, VIO_ERR_HIP, "hipSetDevice(%d)", rs->cfg.device);
    vio_status st = VIO_OK;

    // layout of the upload (bytes; every array 256-aligned)
    const size_t oP = 0, oS = align256(oP + 8 * NF * 7), oE = align256(oS + 8 * NF * 9), oErr = align256(oE + 8 * 7),
                 oPre = align256(oErr + 8 * PRD), oV = align256(oPre + 8 * (size_t)NW * PRE_STRIDE), oPi = align256(oV + 8 * (size_t)n * D),
                 oPj = align256(oPi + (D == 1 ? 16 * (size_t)m : 0)), oOk = align256(oPj + 16 * (size_t)m), oLm = align256(oOk + 4 * NW),
                 oH = align256(oLm + 4 * (size_t)m), oF = align256(oH + (D == 1 ? 4 * (size_t)m : 0)), oOff = align256(oF + 4 * (size_t)m),
                 oEi = align256(oOff + 4 * ((size_t)n + 1)), nin = align256(oEi + 4 * (size_t)m);
    if ((st = ensure(rs, &rs->d_in, &rs->h_in, &rs->in_cap, nin)) != VIO_OK) return st;
    char *hb = rs->h_in;

    // the states (n is checked against the context here: vio_get_landmarks refuses another count, before anything is written)
    if ((st = vio_get_window(rs->ctx, (double *)(hb + oP), (double *)(hb + oS), (double *)(hb + oE))) != VIO_OK)
        return fail(rs, st, "vio_get_window: %s", vio_last_error(rs->ctx));
    st = D == 1 ? vio_get_landmarks(rs->ctx, n, (double *)(hb + oV)) : vio_get_landmarks_xyz(rs->ctx, n, (double *)(hb + oV));
    if (st == VIO_ERR_BAD_ARG)
        return fail(rs, st, "n=%lld is not the context's %s landmark count", (long long)n, D == 1 ? "inverse-depth" : "XYZ");
    if (st != VIO_OK) return fail(rs, st, "vio_get_landmarks%s: %s", D == 1 ? "" : "_xyz", vio_last_error(rs->ctx));
    if ((st = vio_get_prior(rs->ctx, nullptr, (double *)(hb + oErr))) != VIO_OK) return fail(rs, st, "vio_get_prior: %s", vio_last_error(rs->ctx));

    // IMU edges: the pre-integration packed as the solver packs it (vio_types.h PRE_*), the information formed here
    int *ok = (int *)(hb + oOk);
    double *hp = (double *)(hb + oPre);
    for (int k = 0; k < NW; ++k) {
        const vio_preint *p = pre ? pre[k] : nullptr;
        ok[k] = p != nullptr;
        double *o = hp + (size_t)k * PRE_STRIDE;
        std::memset(o, 0, 8 * PRE_STRIDE);
        if (!p) continue;
        o[PRE_SUMDT] = p->sum_dt;
        for (int i = 0; i < 3; ++i) { o[PRE_DP + i] = p->delta_p[i]; o[PRE_DV + i] = p->delta_v[i]; o[PRE_BA + i] = p->linearized_ba[i]; o[PRE_BG + i] = p->linearized_bg[i]; }
        for (int i = 0; i < 4; ++i) o[PRE_DQ + i] = p->delta_q[i];
        std::memcpy(o + PRE_JAC, p->jacobian, 225 * 8);
        inverse15(p->covariance, o + PRE_INFO);
    }
    // the observations as given, and the CSR over the landmarks
    if (m > 0) {
        std::memcpy(hb + oPj, pts_j, 16 * (size_t)m);
        std::memcpy(hb + oLm, lm, 4 * (size_t)m);
        std::memcpy(hb + oF, target, 4 * (size_t)m);
        if (D == 1) {
            std::memcpy(hb + oPi, pts_i, 16 * (size_t)m);
            std::memcpy(hb + oH, host, 4 * (size_t)m);
        }
    }
    int *eidx = (int *)(hb + oEi);
    obs_csr(m, lm, n, (int *)(hb + oOff), [&](int64_t e, int, int q) { eidx[q] = (int)e; return true; });

    void *sp = nullptr;
    if ((st = vio_get_stream(rs->ctx, &sp)) != VIO_OK) return fail(rs, st, "vio_get_stream");
    rs->stream = (hipStream_t)sp;

    const int n_wg = (int)((n + LM_NT - 1) / LM_NT);
    const size_t qObs = 0, qLm = align256(qObs + 32 * (size_t)m), qPart = align256(qLm + 24 * (size_t)n),
                 qSum = align256(qPart + 8 * (size_t)P_STRIDE * (n_wg > 0 ? n_wg : 1)), qDn = align256(qSum + 8 * S_N),
                 qFl = align256(qDn + (size_t)m), nout = align256(qFl + (size_t)n);
    if ((st = ensure(rs, &rs->d_out, &rs->h_out, &rs->out_cap, nout)) != VIO_OK) return st;

    if ((st = hip_ck(rs, hipMemcpyAsync(rs->d_in, rs->h_in, nin, hipMemcpyHostToDevice, rs->stream), "upload")) != VIO_OK) return st;
    const double t_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();

    ResArgs a;
    char *di = rs->d_in, *dq = rs->d_out;
    a.poses = (const double *)(di + oP); a.sb = (const double *)(di + oS); a.ext = (const double *)(di + oE);
    a.errp = (const double *)(di + oErr); a.pre = (const double *)(di + oPre); a.pre_ok = (const int *)(di + oOk);
    a.val = (const double *)(di + oV); a.pts_i = (const double *)(di + oPi); a.pts_j = (const double *)(di + oPj);
    a.lm = (const int *)(di + oLm); a.host = (const int *)(di + oH); a.fr = (const int *)(di + oF);
    a.off = (const int *)(di + oOff); a.eidx = (const int *)(di + oEi);
    a.m = m; a.n = (int)n; a.n_wg = n_wg;
    a.loss_type = rs->cfg.loss_type; a.have_pre = pre != nullptr; a.loss_delta = rs->cfg.loss_delta;
    a.sqrt_info = rs->cfg.reproj_sqrt_info; a.focal = focal; a.outlier_px = outlier_px;
    for (int k = 0; k < 3; ++k) a.gravity[k] = rs->cfg.gravity[k];
    a.obs = (double *)(dq + qObs); a.dneg = (unsigned char *)(dq + qDn); a.lm_out = (double *)(dq + qLm);
    a.flags = (unsigned char *)(dq + qFl); a.part = (double *)(dq + qPart); a.sum = (double *)(dq + qSum);

    if ((st = hip_ck(rs, hipEventRecord(rs->ev[0], rs->stream), "hipEventRecord")) != VIO_OK) return st;
    if (m > 0) {
        const unsigned g = (unsigned)((m + OBS_NT - 1) / OBS_NT);
        if (D == 1) k_res_obs<1><<<g, OBS_NT, 0, rs->stream>>>(a);
        else k_res_obs<3><<<g, OBS_NT, 0, rs->stream>>>(a);
        if ((st = hip_ck(rs, hipGetLastError(), "k_res_obs launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(rs, hipEventRecord(rs->ev[1], rs->stream), "hipEventRecord")) != VIO_OK) return st;
    if (n_wg > 0) {
        if (D == 1) k_res_lm<1><<<(unsigned)n_wg, LM_NT, 0, rs->stream>>>(a);
        else k_res_lm<3><<<(unsigned)n_wg, LM_NT, 0, rs->stream>>>(a);
        if ((st = hip_ck(rs, hipGetLastError(), "k_res_lm launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(rs, hipEventRecord(rs->ev[2], rs->stream), "hipEventRecord")) != VIO_OK) return st;
    k_res_tail<<<1, TAIL_NT, 0, rs->stream>>>(a);
    if ((st = hip_ck(rs, hipGetLastError(), "k_res_tail launch")) != VIO_OK) return st;
    if ((st = hip_ck(rs, hipEventRecord(rs->ev[3], rs->stream), "hipEventRecord")) != VIO_OK) return st;
    // read back what was asked for
    struct Part { bool want; size_t off, bytes; } parts[4] = {
        {obs_out != nullptr && m > 0, qObs, 32 * (size_t)m}, {lm_out != nullptr && n > 0, qLm, 24 * (size_t)n},
        {lm_flags != nullptr && n > 0, qFl, (size_t)n}, {summary != nullptr, qSum, 8 * S_N}};
    for (const Part &p : parts)
        if (p.want && (st = hip_ck(rs, hipMemcpyAsync(rs->h_out + p.off, dq + p.off, p.bytes, hipMemcpyDeviceToHost, rs->stream), "read-back")) != VIO_OK)
            return st;
    if ((st = hip_ck(rs, hipStreamSynchronize(rs->stream), "hipStreamSynchronize")) != VIO_OK) return st;

    if (parts[0].want) std::memcpy(obs_out, rs->h_out + qObs, parts[0].bytes);
    if (parts[1].want) std::memcpy(lm_out, rs->h_out + qLm, parts[1].bytes);
    if (parts[2].want) std::memcpy(lm_flags, rs->h_out + qFl, parts[2].bytes);
    if (summary) {
        const double *s = (const double *)(rs->h_out + qSum);
        vio_res_summary o;
        std::memset(&o, 0, sizeof(o));
        o.chi2 = s[S_CHI]; o.visual_robust = s[S_VR]; o.visual_plain = s[S_VP]; o.imu = s[S_IMU]; o.prior = s[S_PRIOR];
        for (int k = 0; k < NW; ++k) o.imu_edge[k] = s[S_IMUE + k];
        for (int f = 0; f < NF; ++f) { o.frame_robust[f] = s[S_FR + f]; o.frame_edges[f] = (int64_t)s[S_FE + f]; }
        for (int k = 0; k < 3; ++k) o.n_flagged[k] = (int64_t)s[S_FL + k];
        *summary = o;
    }
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k)
        if (hipEventElapsedTime(&ms[k], rs->ev[k], rs->ev[k + 1]) != hipSuccess) {
            for (double &t : rs->timing) t = NAN;   // (the outputs are written: only the timings are unknown)
            return VIO_OK;
        }
    rs->timing[0] = t_host;
    for (int k = 0; k < 3; ++k) rs->timing[1 + k] = ms[k];
    rs->timing[4] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    return VIO_OK;
}

extern "C" {

vio_status vio_res_create(struct vio_ctx *ctx, const vio_config *cfg, vio_res **out) {
    if (!out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    if (!ctx || !cfg) return VIO_ERR_BAD_ARG;
    if (cfg->shard_count > 1) return VIO_ERR_UNSUPPORTED;       // a shard holds part of the landmarks and of the chi2
    vio_res *rs = new (std::nothrow) vio_res;
    if (!rs) return VIO_ERR_BAD_ARG;
    rs->ctx = ctx;
    rs->cfg = *cfg;
    DeviceScope dev(cfg->device);
    if (!dev.ok) { delete rs; return VIO_ERR_HIP; }
    for (int k = 0; k < 4; ++k)
        if (hipEventCreate(&rs->ev[k]) != hipSuccess) { vio_res_destroy(rs); return VIO_ERR_HIP; }
    *out = rs;
    return VIO_OK;
}

void vio_res_destroy(vio_res *rs) {
    if (!rs) return;
    DeviceScope dev(rs->cfg.device);
    if (rs->stream) hipStreamSynchronize(rs->stream);
    for (int k = 0; k < 4; ++k) if (rs->ev[k]) hipEventDestroy(rs->ev[k]);
    if (rs->d_in) hipFree(rs->d_in);
    if (rs->d_out) hipFree(rs->d_out);
    if (rs->h_in) hipHostFree(rs->h_in);
    if (rs->h_out) hipHostFree(rs->h_out);
    delete rs;
}

vio_status vio_res_set_config(vio_res *rs, const vio_config *cfg) {
    if (!rs || !cfg) return VIO_ERR_BAD_ARG;
    if (cfg->device != rs->cfg.device) return fail(rs, VIO_ERR_BAD_ARG, "device %d: the handle was made for device %d", cfg->device, rs->cfg.device);
    if (cfg->shard_count > 1) return fail(rs, VIO_ERR_UNSUPPORTED, "sharded context");
    rs->cfg = *cfg;
    return VIO_OK;
}

const char *vio_res_last_error(const vio_res *rs) { return rs ? rs->err : "null handle"; }

int32_t vio_res_version(void) { return VIO_RES_VERSION; }

vio_status vio_res_compute(vio_res *rs, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                           const double *pts_i, const double *pts_j, int64_t n, const vio_preint *const *pre, double focal,
                           double outlier_px, double *obs_out, double *lm_out, uint8_t *lm_flags, vio_res_summary *summary) {
    if (!rs) return VIO_ERR_BAD_ARG;
    rs->err[0] = 0;
    return compute(rs, 1, m, lm, host, target, pts_i, pts_j, n, pre, focal, outlier_px, obs_out, lm_out, lm_flags, summary);
}

vio_status vio_res_compute_xyz(vio_res *rs, int64_t m, const int32_t *lm, const int32_t *frame, const double *pts, int64_t n,
                               const vio_preint *const *pre, double focal, double outlier_px, double *obs_out, double *lm_out,
                               uint8_t *lm_flags, vio_res_summary *summary) {
    if (!rs) return VIO_ERR_BAD_ARG;
    rs->err[0] = 0;
    return compute(rs, 3, m, lm, nullptr, frame, nullptr, pts, n, pre, focal, outlier_px, obs_out, lm_out, lm_flags, summary);
}

vio_status vio_res_timing(vio_res *rs, double *out5) {
    if (!rs || !out5) return VIO_ERR_BAD_ARG;
    memcpy(out5, rs->timing, sizeof(rs->timing));
    return VIO_OK;
}

}   // extern "C"
