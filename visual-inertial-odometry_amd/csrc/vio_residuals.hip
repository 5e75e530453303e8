// vio_residuals.hip — per-edge residuals, the chi2 breakdown and landmark outlier flags (include/vio_residuals.h; DESIGN.md
// sections 11 and 13).
//
// A companion of libvio_hip.so that uses nothing but its C ABI: the states are read back through the getters, and the three kernels
// below run on the context's stream.  vio_res_compute_batch runs each of them once for many windows (k_res_*_batch: the same bodies,
// vio_res_*_body.inc; every window's edges and landmarks tiled from a workgroup boundary, one tail workgroup per window).
//   k_res_obs<D>  one thread per edge, in the caller's order: the reprojection residual, e2 and rho0, stored as one row of obs.
//   k_res_lm      one thread per landmark: its edges walked in CSR order -> mean / max pixel error, sum of rho0, flags; per-workgroup
//                 partials of the visual totals, the 11 frame sums and the flag counts (DPP wave sums, waves in order).
//   k_res_tail    one workgroup: the ten IMU residuals (the solver's d_imu_residual) and r^T Sigma^-1 r, the partials added in
//                 workgroup order, ||err_prior||, chi2.
// No atomics: every output is written by one thread, every sum has a fixed order, so a call is bitwise reproducible.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vio_batch_grid.h"
#include "vio_companion.h"
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
    const unsigned blk = blockIdx.x;
#include "vio_res_obs_body.inc"
}

// k_res_obs for a batch: window w owns the workgroups [blk0[w], blk0[w + 1]) (vio_batch_grid.h), which restart at its edge 0.
template <int D>
__global__ void __launch_bounds__(OBS_NT) k_res_obs_batch(const ResArgs *__restrict__ items, const int *__restrict__ blk0, int count) {
    const int win = batch_window(blk0, count, blockIdx.x);
    const ResArgs a = items[win];
    const unsigned blk = blockIdx.x - (unsigned)blk0[win];
#include "vio_res_obs_body.inc"
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k_res_lm: per landmark statistics and flags; per-workgroup partials.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(LM_NT) k_res_lm(ResArgs a) {
    const unsigned blk = blockIdx.x;
#include "vio_res_lm_body.inc"
}

// k_res_lm for a batch: window w owns the workgroups [blk0[w], blk0[w + 1]), which restart at its landmark 0 and write its partial
// rows 0 .. n_wg - 1, so its DPP sums see the segments they see in k_res_lm.
template <int D>
__global__ void __launch_bounds__(LM_NT) k_res_lm_batch(const ResArgs *__restrict__ items, const int *__restrict__ blk0, int count) {
    const int win = batch_window(blk0, count, blockIdx.x);
    const ResArgs a = items[win];
    const unsigned blk = blockIdx.x - (unsigned)blk0[win];
#include "vio_res_lm_body.inc"
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k_res_tail: one workgroup.  Wave 0 lanes 0..9: the IMU edges; every wave: some of the partial columns (lanes stride over the
// workgroups, then a DPP sum); wave 3: ||err_prior||.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TAIL_NT) k_res_tail(ResArgs a) {
#include "vio_res_tail_body.inc"
}

// k_res_tail for a batch: workgroup w is window w's tail.
__global__ void __launch_bounds__(TAIL_NT) k_res_tail_batch(const ResArgs *__restrict__ items) {
    const ResArgs a = items[blockIdx.x];
#include "vio_res_tail_body.inc"
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
struct vio_res {
    vio_ctx *ctx = nullptr;
    vio_config cfg;
    StreamEvents<4> q;                              // the context's stream (borrowed, set by stage()) and the timing events
    ErrText err = {0};
    // poses | sb | ext | errp | pre | val | pts_i | pts_j (doubles), then pre_ok | lm | host | fr | off | eidx (ints): one upload
    Twin<char> in;
    // obs | lm_out | part | sum (doubles), then dneg | flags (bytes); the requested parts come back through out.h
    Twin<char> out;
    // the batch tables of a vio_res_compute_batch whose first handle this is (ResArgs | workgroup starts)
    Twin<char> tab;
    double timing[5] = {0, 0, 0, 0, 0};
};

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

// One window staged for the kernels: its upload enqueued on the context's stream, its kernel arguments, its read-back layout.
struct Staged {
    ResArgs a;
    int64_t m = 0, n = 0;
    int D = 1;
    size_t qObs = 0, qLm = 0, qSum = 0, qFl = 0, nout = 0;      // bytes of d_out
};

// Validation, read-back of the states, packing, and the upload (enqueued on the context's stream).  Nothing is launched and no output
// is written.  The caller holds the context's device.
// D = 1: obs (host, target, pts_i, pts_j); D = 3: obs (frame, pts) in `target` / `pts_j`
static vio_status stage(vio_res *rs, int D, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                        const double *pts_i, const double *pts_j, int64_t n, const vio_preint *const *pre, double focal,
                        double outlier_px, Staged &sg) {
    if (m < 0 || n < 0 || n >= INT32_MAX || m >= INT32_MAX) return fail(rs->err, VIO_ERR_BAD_ARG, "bad sizes m=%lld n=%lld", (long long)m, (long long)n);
    if (!(focal > 0.0)) return fail(rs->err, VIO_ERR_BAD_ARG, "focal %g is not positive", focal);
    if (m > 0 && (!lm || !target || !pts_j || (D == 1 && (!host || !pts_i)))) return fail(rs->err, VIO_ERR_BAD_ARG, "observation array is NULL");
    for (int64_t e = 0; e < m; ++e) {
        if (lm[e] < 0 || lm[e] >= n || target[e] < 0 || target[e] >= NF || (D == 1 && (host[e] < 0 || host[e] >= NF)))
            return fail(rs->err, VIO_ERR_BAD_ARG, "observation %lld refers to landmark %d / a frame out of range", (long long)e, lm[e]);
    }
    vio_status st = VIO_OK;

    // layout of the upload (bytes; every array 256-aligned)
    const size_t oP = 0, oS = align256(oP + 8 * NF * 7), oE = align256(oS + 8 * NF * 9), oErr = align256(oE + 8 * 7),
                 oPre = align256(oErr + 8 * PRD), oV = align256(oPre + 8 * (size_t)NW * PRE_STRIDE), oPi = align256(oV + 8 * (size_t)n * D),
                 oPj = align256(oPi + (D == 1 ? 16 * (size_t)m : 0)), oOk = align256(oPj + 16 * (size_t)m), oLm = align256(oOk + 4 * NW),
                 oH = align256(oLm + 4 * (size_t)m), oF = align256(oH + (D == 1 ? 4 * (size_t)m : 0)), oOff = align256(oF + 4 * (size_t)m),
                 oEi = align256(oOff + 4 * ((size_t)n + 1)), nin = align256(oEi + 4 * (size_t)m);
    if ((st = rs->in.ensure(rs->err, nin)) != VIO_OK) return st;
    char *hb = rs->in.h;

    // the states (n is checked against the context here: vio_get_landmarks refuses another count, before anything is written)
    if ((st = vio_get_window(rs->ctx, (double *)(hb + oP), (double *)(hb + oS), (double *)(hb + oE))) != VIO_OK)
        return fail(rs->err, st, "vio_get_window: %s", vio_last_error(rs->ctx));
    st = D == 1 ? vio_get_landmarks(rs->ctx, n, (double *)(hb + oV)) : vio_get_landmarks_xyz(rs->ctx, n, (double *)(hb + oV));
    if (st == VIO_ERR_BAD_ARG)
        return fail(rs->err, st, "n=%lld is not the context's %s landmark count", (long long)n, D == 1 ? "inverse-depth" : "XYZ");
    if (st != VIO_OK) return fail(rs->err, st, "vio_get_landmarks%s: %s", D == 1 ? "" : "_xyz", vio_last_error(rs->ctx));
    if ((st = vio_get_prior(rs->ctx, nullptr, (double *)(hb + oErr))) != VIO_OK) return fail(rs->err, st, "vio_get_prior: %s", vio_last_error(rs->ctx));

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
    if ((st = vio_get_stream(rs->ctx, &sp)) != VIO_OK) return fail(rs->err, st, "vio_get_stream");
    rs->q.stream = (hipStream_t)sp;

    const int n_wg = (int)((n + LM_NT - 1) / LM_NT);
    const size_t qObs = 0, qLm = align256(qObs + 32 * (size_t)m), qPart = align256(qLm + 24 * (size_t)n),
                 qSum = align256(qPart + 8 * (size_t)P_STRIDE * (n_wg > 0 ? n_wg : 1)), qDn = align256(qSum + 8 * S_N),
                 qFl = align256(qDn + (size_t)m), nout = align256(qFl + (size_t)n);
    if ((st = rs->out.ensure(rs->err, nout)) != VIO_OK) return st;

    if ((st = hip_ck(rs->err, hipMemcpyAsync(rs->in.d, rs->in.h, nin, hipMemcpyHostToDevice, rs->q.stream), "upload")) != VIO_OK) return st;

    ResArgs &a = sg.a;
    char *di = rs->in.d, *dq = rs->out.d;
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
    sg.m = m; sg.n = n; sg.D = D;
    sg.qObs = qObs; sg.qLm = qLm; sg.qSum = qSum; sg.qFl = qFl; sg.nout = nout;
    return VIO_OK;
}

// After the read-back has completed: the requested outputs, from h_out at the offsets the device used
static void finish(vio_res *rs, const Staged &sg, double *obs_out, double *lm_out, uint8_t *lm_flags, vio_res_summary *summary) {
    if (obs_out && sg.m > 0) std::memcpy(obs_out, rs->out.h + sg.qObs, 32 * (size_t)sg.m);
    if (lm_out && sg.n > 0) std::memcpy(lm_out, rs->out.h + sg.qLm, 24 * (size_t)sg.n);
    if (lm_flags && sg.n > 0) std::memcpy(lm_flags, rs->out.h + sg.qFl, (size_t)sg.n);
    if (summary) {
        const double *s = (const double *)(rs->out.h + sg.qSum);
        vio_res_summary o;
        std::memset(&o, 0, sizeof(o));
        o.chi2 = s[S_CHI]; o.visual_robust = s[S_VR]; o.visual_plain = s[S_VP]; o.imu = s[S_IMU]; o.prior = s[S_PRIOR];
        for (int k = 0; k < NW; ++k) o.imu_edge[k] = s[S_IMUE + k];
        for (int f = 0; f < NF; ++f) { o.frame_robust[f] = s[S_FR + f]; o.frame_edges[f] = (int64_t)s[S_FE + f]; }
        for (int k = 0; k < 3; ++k) o.n_flagged[k] = (int64_t)s[S_FL + k];
        *summary = o;
    }
}

static vio_status compute(vio_res *rs, int D, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                          const double *pts_i, const double *pts_j, int64_t n, const vio_preint *const *pre, double focal,
                          double outlier_px, double *obs_out, double *lm_out, uint8_t *lm_flags, vio_res_summary *summary) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    DeviceScope dev(rs->cfg.device);
    if (!dev.ok) return fail(rs->err, VIO_ERR_HIP, "hipSetDevice(%d)", rs->cfg.device);
    Staged sg;
    vio_status st = stage(rs, D, m, lm, host, target, pts_i, pts_j, n, pre, focal, outlier_px, sg);
    if (st != VIO_OK) return st;
    const double t_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    const ResArgs &a = sg.a;
    const int n_wg = a.n_wg;
    char *dq = rs->out.d;

    if ((st = hip_ck(rs->err, hipEventRecord(rs->q.ev[0], rs->q.stream), "hipEventRecord")) != VIO_OK) return st;
    if (m > 0) {
        const unsigned g = (unsigned)((m + OBS_NT - 1) / OBS_NT);
        if (D == 1) k_res_obs<1><<<g, OBS_NT, 0, rs->q.stream>>>(a);
        else k_res_obs<3><<<g, OBS_NT, 0, rs->q.stream>>>(a);
        if ((st = hip_ck(rs->err, hipGetLastError(), "k_res_obs launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(rs->err, hipEventRecord(rs->q.ev[1], rs->q.stream), "hipEventRecord")) != VIO_OK) return st;
    if (n_wg > 0) {
        if (D == 1) k_res_lm<1><<<(unsigned)n_wg, LM_NT, 0, rs->q.stream>>>(a);
        else k_res_lm<3><<<(unsigned)n_wg, LM_NT, 0, rs->q.stream>>>(a);
        if ((st = hip_ck(rs->err, hipGetLastError(), "k_res_lm launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(rs->err, hipEventRecord(rs->q.ev[2], rs->q.stream), "hipEventRecord")) != VIO_OK) return st;
    k_res_tail<<<1, TAIL_NT, 0, rs->q.stream>>>(a);
    if ((st = hip_ck(rs->err, hipGetLastError(), "k_res_tail launch")) != VIO_OK) return st;
    if ((st = hip_ck(rs->err, hipEventRecord(rs->q.ev[3], rs->q.stream), "hipEventRecord")) != VIO_OK) return st;
    // read back what was asked for
    struct Part { bool want; size_t off, bytes; } parts[4] = {
        {obs_out != nullptr && m > 0, sg.qObs, 32 * (size_t)m}, {lm_out != nullptr && n > 0, sg.qLm, 24 * (size_t)n},
        {lm_flags != nullptr && n > 0, sg.qFl, (size_t)n}, {summary != nullptr, sg.qSum, 8 * S_N}};
    for (const Part &p : parts)
        if (p.want && (st = hip_ck(rs->err, hipMemcpyAsync(rs->out.h + p.off, dq + p.off, p.bytes, hipMemcpyDeviceToHost, rs->q.stream), "read-back")) != VIO_OK)
            return st;
    if ((st = hip_ck(rs->err, hipStreamSynchronize(rs->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;

    finish(rs, sg, obs_out, lm_out, lm_flags, summary);
    float ms[3];
    for (int k = 0; k < 3; ++k)
        if (std::isnan(ms[k] = elapsed_ms(rs->q.ev[k], rs->q.ev[k + 1]))) {
            for (double &t : rs->timing) t = NAN;   // (the outputs are written: only the timings are unknown)
            return VIO_OK;
        }
    rs->timing[0] = t_host;
    for (int k = 0; k < 3; ++k) rs->timing[1 + k] = ms[k];
    rs->timing[4] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    return VIO_OK;
}

// a window's error, reported on the batch's first handle as well
static vio_status batch_fail(vio_res *r0, vio_status st, int i, const vio_res *rs) {
    char msg[sizeof(rs->err)];
    memcpy(msg, rs->err, sizeof(msg));
    return fail(r0->err, st, "vio_res_compute_batch: window %d: %s", i, msg);
}

// The batch: every window staged in its own handle's buffers (one upload each), one table upload, k_res_obs_batch, k_res_lm_batch
// and k_res_tail_batch once for all windows, one read-back per window (its whole output block), one synchronisation.
static vio_status compute_batch(vio_res *const *rss, int32_t count, int32_t xyz, const vio_res_batch_item *items, double focal,
                                double outlier_px) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    vio_res *r0 = rss[0];
    const int D = xyz ? 3 : 1;
    void *s0 = nullptr;
    for (int32_t i = 0; i < count; ++i) {
        vio_res *rs = rss[i];
        if (!rs) return fail(r0->err, VIO_ERR_BAD_ARG, "vio_res_compute_batch: window %d: null handle", i);
        rs->err[0] = 0;
        if (rs->cfg.shard_count > 1) return fail(r0->err, VIO_ERR_UNSUPPORTED, "vio_res_compute_batch: window %d: sharded context", i);
        if (rs->cfg.device != r0->cfg.device)
            return fail(r0->err, VIO_ERR_BAD_ARG, "vio_res_compute_batch: window %d is on device %d, window 0 on %d: the contexts must share one device and one stream", i, rs->cfg.device, r0->cfg.device);
        for (int32_t j = 0; j < i; ++j)
            if (rss[j] == rs) return fail(r0->err, VIO_ERR_BAD_ARG, "vio_res_compute_batch: windows %d and %d are the same handle", j, i);
    }
    DeviceScope dev(r0->cfg.device);
    if (!dev.ok) return fail(r0->err, VIO_ERR_HIP, "hipSetDevice(%d)", r0->cfg.device);
    for (int32_t i = 0; i < count; ++i) {
        void *sp = nullptr;
        if (vio_get_stream(rss[i]->ctx, &sp) != VIO_OK) return fail(r0->err, VIO_ERR_BAD_ARG, "vio_res_compute_batch: window %d: vio_get_stream", i);
        if (i == 0) s0 = sp;
        else if (sp != s0) return fail(r0->err, VIO_ERR_BAD_ARG, "vio_res_compute_batch: window %d is on another stream than window 0: the contexts must share one device and one stream", i);
    }
    vio_status st = VIO_OK;
    std::vector<Staged> sg(count);
    for (int32_t i = 0; i < count; ++i) {
        const vio_res_batch_item &it = items[i];
        st = stage(rss[i], D, it.m, it.lm, D == 1 ? it.host : nullptr, it.target, D == 1 ? it.pts_i : nullptr, it.pts_j, it.n, it.pre,
                   focal, outlier_px, sg[i]);
        if (st != VIO_OK) return batch_fail(r0, st, i, rss[i]);
    }
    // the tables: ResArgs[count] | obs workgroup starts[count + 1] | lm workgroup starts[count + 1]
    const size_t bArgs = 0, bObs = align256(sizeof(ResArgs) * count), bLm = bObs + sizeof(int) * ((size_t)count + 1),
                 nbytes = bLm + sizeof(int) * ((size_t)count + 1);
    if ((st = r0->tab.ensure(r0->err, nbytes)) != VIO_OK) return st;
    char *ht = r0->tab.h;
    ResArgs *ta = (ResArgs *)(ht + bArgs);
    int *blk_obs = (int *)(ht + bObs), *blk_lm = (int *)(ht + bLm);
    int64_t nobs = 0, nlm = 0;
    for (int32_t i = 0; i < count; ++i) {
        ta[i] = sg[i].a;
        blk_obs[i] = (int)nobs;
        blk_lm[i] = (int)nlm;
        nobs += (sg[i].m + OBS_NT - 1) / OBS_NT;
        nlm += sg[i].a.n_wg;
        if (nobs > INT32_MAX || nlm > INT32_MAX) return fail(r0->err, VIO_ERR_BAD_ARG, "vio_res_compute_batch: too many edges in the batch");
    }
    blk_obs[count] = (int)nobs;
    blk_lm[count] = (int)nlm;
    hipStream_t stream = (hipStream_t)s0;
    const char *dt = r0->tab.d;
    if ((st = hip_ck(r0->err, hipMemcpyAsync(r0->tab.d, r0->tab.h, nbytes, hipMemcpyHostToDevice, stream), "table upload")) != VIO_OK) return st;
    const double t_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();

    const ResArgs *da = (const ResArgs *)(dt + bArgs);
    if ((st = hip_ck(r0->err, hipEventRecord(r0->q.ev[0], stream), "hipEventRecord")) != VIO_OK) return st;
    if (nobs > 0) {
        if (D == 1) k_res_obs_batch<1><<<(unsigned)nobs, OBS_NT, 0, stream>>>(da, (const int *)(dt + bObs), count);
        else k_res_obs_batch<3><<<(unsigned)nobs, OBS_NT, 0, stream>>>(da, (const int *)(dt + bObs), count);
        if ((st = hip_ck(r0->err, hipGetLastError(), "k_res_obs_batch launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(r0->err, hipEventRecord(r0->q.ev[1], stream), "hipEventRecord")) != VIO_OK) return st;
    if (nlm > 0) {
        if (D == 1) k_res_lm_batch<1><<<(unsigned)nlm, LM_NT, 0, stream>>>(da, (const int *)(dt + bLm), count);
        else k_res_lm_batch<3><<<(unsigned)nlm, LM_NT, 0, stream>>>(da, (const int *)(dt + bLm), count);
        if ((st = hip_ck(r0->err, hipGetLastError(), "k_res_lm_batch launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(r0->err, hipEventRecord(r0->q.ev[2], stream), "hipEventRecord")) != VIO_OK) return st;
    k_res_tail_batch<<<(unsigned)count, TAIL_NT, 0, stream>>>(da);
    if ((st = hip_ck(r0->err, hipGetLastError(), "k_res_tail_batch launch")) != VIO_OK) return st;
    if ((st = hip_ck(r0->err, hipEventRecord(r0->q.ev[3], stream), "hipEventRecord")) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i)
        if ((st = hip_ck(rss[i]->err, hipMemcpyAsync(rss[i]->out.h, rss[i]->out.d, sg[i].nout, hipMemcpyDeviceToHost, stream), "read-back")) != VIO_OK)
            return batch_fail(r0, st, i, rss[i]);
    if ((st = hip_ck(r0->err, hipStreamSynchronize(stream), "hipStreamSynchronize")) != VIO_OK) return st;

    for (int32_t i = 0; i < count; ++i)
        finish(rss[i], sg[i], items[i].obs_out, items[i].lm_out, items[i].lm_flags, items[i].summary);
    float ms[3];
    double tm[5] = {NAN, NAN, NAN, NAN, NAN};
    bool ev_ok = true;
    for (int k = 0; k < 3; ++k) ev_ok = ev_ok && !std::isnan(ms[k] = elapsed_ms(r0->q.ev[k], r0->q.ev[k + 1]));
    if (ev_ok) {
        tm[0] = t_host;
        for (int k = 0; k < 3; ++k) tm[1 + k] = ms[k];
        tm[4] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    }
    for (int32_t i = 0; i < count; ++i) memcpy(rss[i]->timing, tm, sizeof(tm));
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
    if (rs->q.create_events() != hipSuccess) { vio_res_destroy(rs); return VIO_ERR_HIP; }
    *out = rs;
    return VIO_OK;
}

void vio_res_destroy(vio_res *rs) {
    if (!rs) return;
    DeviceScope dev(rs->cfg.device);
    rs->q.release();
    delete rs;                                      // (the buffers free themselves)
}

vio_status vio_res_set_config(vio_res *rs, const vio_config *cfg) {
    if (!rs || !cfg) return VIO_ERR_BAD_ARG;
    if (cfg->device != rs->cfg.device) return fail(rs->err, VIO_ERR_BAD_ARG, "device %d: the handle was made for device %d", cfg->device, rs->cfg.device);
    if (cfg->shard_count > 1) return fail(rs->err, VIO_ERR_UNSUPPORTED, "sharded context");
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

vio_status vio_res_compute_batch(vio_res *const *rss, int32_t count, int32_t xyz, const vio_res_batch_item *items, double focal,
                                 double outlier_px) {
    if (count < 0 || (count > 0 && (!rss || !items))) return VIO_ERR_BAD_ARG;
    if (count == 0) return VIO_OK;
    if (!rss[0]) return VIO_ERR_BAD_ARG;
    rss[0]->err[0] = 0;
    return compute_batch(rss, count, xyz, items, focal, outlier_px);
}

vio_status vio_res_timing(vio_res *rs, double *out5) {
    if (!rs || !out5) return VIO_ERR_BAD_ARG;
    memcpy(out5, rs->timing, sizeof(rs->timing));
    return VIO_OK;
}

}   // extern "C"

