// vio_covariance.hip — marginal covariances of a solved window (include/vio_covariance.h; DESIGN.md sections 10 and 13).
//
// A companion of libvio_hip.so that uses nothing but its C ABI: the system and the states are read back through the getters, and
// the two kernels below run on the context's stream.  vio_cov_compute_batch runs each of them once for many windows
// (k_cov_pose_batch, k_cov_landmarks_batch: the same bodies, vio_cov_*_body.inc, one window per workgroup).
//   k_cov_pose          one workgroup: the reduced H_pp_schur (fixed variables removed) as a packed lower triangle in LDS, inverted
//                       in place by the symmetric sweep; Sigma written once as a full 171 x 171 and as the 72 x 72 camera block.
//   k_cov_landmarks<D>  one lane per landmark: its observations' reprojection Jacobians and robust weights (d_robust_info2 of
//                       vio_device_math.h, which vio_marg.hip includes too) recomputed, h_l and w_l accumulated in a fixed order,
//                       then the quadratic form against Sigma_cc staged in LDS.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vio_batch_grid.h"
#include "vio_companion.h"
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
#include "vio_cov_pose_body.inc"
}

// one window of k_cov_pose_batch: k_cov_pose's arguments, in the window's own buffers
struct CovPoseItem {
    const double *S;
    const int *keep;
    double *cov;
    double *cc;
    int *status;
    double *ratio;
    int n;
};

// k_cov_pose for a batch: workgroup w inverts window w's system, with k_cov_pose's code (vio_cov_pose_body.inc), so each window gets
// the bits the single call gives it.  117 KB of LDS: one workgroup per CU, the windows side by side.
__global__ void __launch_bounds__(POSE_NT) k_cov_pose_batch(const CovPoseItem *__restrict__ items) {
    const CovPoseItem it = items[blockIdx.x];
    const double *__restrict__ S = it.S;
    const int *__restrict__ keep = it.keep;
    const int n = it.n;
    double *__restrict__ cov = it.cov;
    double *__restrict__ cc = it.cc;
    int *__restrict__ status = it.status;
    double *__restrict__ ratio = it.ratio;
#include "vio_cov_pose_body.inc"
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

template <int D>
__global__ void __launch_bounds__(LmNT<D>::v) k_cov_landmarks(CovLmArgs a) {
    const unsigned blk = blockIdx.x;
#include "vio_cov_landmarks_body.inc"
}

// k_cov_landmarks for a batch: window w owns the workgroups [blk0[w], blk0[w + 1]), which restart at its landmark 0 and stage its
// Sigma_cc and rotations, so each lane runs what it runs in k_cov_landmarks on that window alone.
template <int D>
__global__ void __launch_bounds__(LmNT<D>::v) k_cov_landmarks_batch(const CovLmArgs *__restrict__ items, const int *__restrict__ blk0,
                                                                    int count) {
    const int win = batch_window(blk0, count, blockIdx.x);
    const CovLmArgs a = items[win];
    const unsigned blk = blockIdx.x - (unsigned)blk0[win];
#include "vio_cov_landmarks_body.inc"
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
struct vio_cov {
    vio_ctx *ctx = nullptr;
    vio_config cfg;
    StreamEvents<3> q;                      // the context's stream (borrowed, set by stage()) and the timing events
    ErrText err = {0};
    // S | poses | ext | val | pts_i | pts_j (doubles), then keep | off | ofr | ohost | status (ints): one upload
    Twin<double> in;
    // cov | cc | out | info (doubles), then status (2 ints): one read-back
    Twin<double> out;
    // the batch tables of a vio_cov_compute_batch whose first handle this is (CovPoseItem | CovLmArgs | workgroup starts)
    Twin<char> tab;
    int64_t last_n = -1;
    int last_dim = 0;
    std::vector<double> info;               // of the last successful compute
    double timing[4] = {0, 0, 0, 0};
    double pivot_ratio = 0.0;               // of the last successful compute
    bool relinearize = false;               // vio_cov_set_config changed what the system depends on: the context's linearisation, if it
                                            // holds one, is of the old configuration (vio_set_config keeps it), so linearise first
};

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

// One window staged for the kernels: its upload enqueued on the context's stream, and where everything lies in the handle's buffers.
struct Staged {
    int D = 1;
    int nk = 0;                             // variables kept
    int ext_fixed = 1;
    int64_t n = 0;
    size_t oS = 0, oP = 0, oE = 0, oV = 0, oPi = 0, oPj = 0, nd = 0;            // doubles of d_in
    size_t iKeep = 0, iOff = 0, iOfr = 0, iHost = 0, ni = 0;                   // ints after them
    size_t o_cov = 0, o_cc = 0, o_out = 0, o_info = 0, nout = 0;               // doubles of d_out, then the status ints
};

// Validation, linearisation when needed, read-back of the system and the states, the CSR, and the upload (enqueued on the context's
// stream, with the status words reset).  Nothing is launched and no output is written.  The caller holds the context's device.
// D = 1: obs (host, target, pts_i, pts_j); D = 3: obs (frame, pts) in `target` / `pts_j`
static vio_status stage(vio_cov *cv, int D, int32_t gauge, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                        const double *pts_i, const double *pts_j, int64_t n, Staged &sg) {
    if (gauge != VIO_COV_GAUGE_NONE && gauge != VIO_COV_GAUGE_FIX_OLDEST) return fail(cv->err, VIO_ERR_BAD_ARG, "unknown gauge %d", gauge);
    if (m < 0 || n < 0 || n > INT32_MAX / 9 || m > INT32_MAX) return fail(cv->err, VIO_ERR_BAD_ARG, "bad sizes m=%lld n=%lld", (long long)m, (long long)n);
    if (m > 0 && (!lm || !target || !pts_j || (D == 1 && (!host || !pts_i)))) return fail(cv->err, VIO_ERR_BAD_ARG, "observation array is NULL");
    for (int64_t e = 0; e < m; ++e) {
        if (lm[e] < 0 || lm[e] >= n || target[e] < 0 || target[e] >= NF || (D == 1 && (host[e] < 0 || host[e] >= NF)))
            return fail(cv->err, VIO_ERR_BAD_ARG, "observation %lld refers to landmark %d / frame out of range", (long long)e, lm[e]);
    }
    vio_status st = VIO_OK;

    // layout of the upload
    sg.D = D;
    sg.n = n;
    const size_t oS = 0, oP = oS + PD * PD, oE = oP + NF * 7, oV = align8(oE + 7), oPi = align8(oV + (size_t)n * D),
                 oPj = align8(oPi + (D == 1 ? 2 * (size_t)n : 0)), nd = align8(oPj + 2 * (size_t)m);
    const size_t iKeep = 0, iOff = iKeep + PD + 1, iOfr = iOff + (size_t)n + 1, iHost = iOfr + (size_t)m, ni = iHost + (size_t)n + 2;
    sg.oS = oS; sg.oP = oP; sg.oE = oE; sg.oV = oV; sg.oPi = oPi; sg.oPj = oPj; sg.nd = nd;
    sg.iKeep = iKeep; sg.iOff = iOff; sg.iOfr = iOfr; sg.iHost = iHost; sg.ni = ni;
    if ((st = cv->in.ensure(cv->err, nd * sizeof(double) + ni * sizeof(int))) != VIO_OK) return st;
    double *hd = cv->in.h;
    int *hi = (int *)(cv->in.h + nd);

    // H_pp_schur at the current state: linearise first when the context says it holds none, or holds one of an older configuration
    if (cv->relinearize) {
        if ((st = vio_linearize(cv->ctx)) != VIO_OK) return fail(cv->err, st, "vio_linearize: %s", vio_last_error(cv->ctx));
        cv->relinearize = false;
    }
    st = vio_get_schur_system(cv->ctx, hd + oS, nullptr);
    if (st == VIO_ERR_BAD_ARG) {
        if ((st = vio_linearize(cv->ctx)) != VIO_OK) return fail(cv->err, st, "vio_linearize: %s", vio_last_error(cv->ctx));
        st = vio_get_schur_system(cv->ctx, hd + oS, nullptr);
    }
    if (st != VIO_OK) return fail(cv->err, st, "vio_get_schur_system: %s", vio_last_error(cv->ctx));
    double sb[NF * 9];
    if ((st = vio_get_window(cv->ctx, hd + oP, sb, hd + oE)) != VIO_OK) return fail(cv->err, st, "vio_get_window: %s", vio_last_error(cv->ctx));
    st = D == 1 ? vio_get_landmarks(cv->ctx, n, hd + oV) : vio_get_landmarks_xyz(cv->ctx, n, hd + oV);
    if (st != VIO_OK) return fail(cv->err, st, "vio_get_landmarks%s(n=%lld): %s", D == 1 ? "" : "_xyz", (long long)n, vio_last_error(cv->ctx));

    // variables kept: everything but the extrinsic (fixed, or not a variable of XYZ edges) and frame 0's pose (gauge)
    const int ext_fixed = D == 3 || cv->cfg.ext_fixed;
    int nk = 0;
    for (int v = 0; v < PD; ++v) {
        if (v < 6 && ext_fixed) continue;
        if (gauge == VIO_COV_GAUGE_FIX_OLDEST && v >= 6 && v < 12) continue;
        hi[iKeep + nk++] = v;
    }
    sg.nk = nk;
    sg.ext_fixed = ext_fixed;
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
    if (!ok) return fail(cv->err, VIO_ERR_BAD_ARG, "landmark %d has observations with different host frames", mixed);
    if (D == 1)
        for (int64_t l = 0; l < n; ++l)
            if (oh[l] < 0) { oh[l] = 0; hd[oPi + 2 * (size_t)l] = 0; hd[oPi + 2 * (size_t)l + 1] = 0; }

    void *sp = nullptr;
    if ((st = vio_get_stream(cv->ctx, &sp)) != VIO_OK) return fail(cv->err, st, "vio_get_stream");
    cv->q.stream = (hipStream_t)sp;

    const size_t o_cov = 0, o_cc = PD * PD, o_out = o_cc + CD * CD, o_info = o_out + (size_t)n * D * D, nout = align8(o_info + (size_t)n * D * D);
    sg.o_cov = o_cov; sg.o_cc = o_cc; sg.o_out = o_out; sg.o_info = o_info; sg.nout = nout;
    if ((st = cv->out.ensure(cv->err, nout * sizeof(double) + 8 * sizeof(int))) != VIO_OK) return st;
    int *d_status = (int *)(cv->out.d + nout);

    if ((st = hip_ck(cv->err, hipMemcpyAsync(cv->in.d, cv->in.h, nd * sizeof(double) + ni * sizeof(int), hipMemcpyHostToDevice, cv->q.stream), "upload")) != VIO_OK) return st;
    // status[0]: failing pivot (-1: none); status[1]: smallest landmark without a positive definite information (NO_BAD_LM: none)
    if ((st = hip_ck(cv->err, hipMemsetAsync(d_status, 0xff, sizeof(int), cv->q.stream), "hipMemsetAsync")) != VIO_OK) return st;
    if ((st = hip_ck(cv->err, hipMemsetAsync(d_status + 1, 0x7f, sizeof(int), cv->q.stream), "hipMemsetAsync")) != VIO_OK) return st;
    return VIO_OK;
}

// k_cov_pose's and k_cov_landmarks' arguments for a staged window
static CovPoseItem pose_item(vio_cov *cv, const Staged &sg) {
    int *di = (int *)(cv->in.d + sg.nd), *d_status = (int *)(cv->out.d + sg.nout);
    CovPoseItem it;
    it.S = cv->in.d + sg.oS; it.keep = di + sg.iKeep; it.n = sg.nk; it.cov = cv->out.d + sg.o_cov; it.cc = cv->out.d + sg.o_cc;
    it.status = d_status; it.ratio = (double *)(d_status + 2);
    return it;
}

static CovLmArgs lm_args(vio_cov *cv, const Staged &sg) {
    int *di = (int *)(cv->in.d + sg.nd), *d_status = (int *)(cv->out.d + sg.nout);
    CovLmArgs a;
    a.cc = cv->out.d + sg.o_cc; a.poses = cv->in.d + sg.oP; a.ext = cv->in.d + sg.oE; a.val = cv->in.d + sg.oV; a.pts_i = cv->in.d + sg.oPi;
    a.pts_j = cv->in.d + sg.oPj; a.off = di + sg.iOff; a.ofr = di + sg.iOfr; a.ohost = di + sg.iHost; a.n = (int)sg.n;
    a.ext_free = !sg.ext_fixed; a.loss_type = cv->cfg.loss_type; a.loss_delta = cv->cfg.loss_delta; a.sqrt_info = cv->cfg.reproj_sqrt_info;
    a.out = cv->out.d + sg.o_out; a.info = cv->out.d + sg.o_info; a.bad = d_status + 1;
    return a;
}

static vio_status read_back(vio_cov *cv, const Staged &sg) {
    return hip_ck(cv->err, hipMemcpyAsync(cv->out.h, cv->out.d, sg.nout * sizeof(double) + 8 * sizeof(int), hipMemcpyDeviceToHost, cv->q.stream), "read-back");
}

// After the read-back has completed: the window's verdict, and on success its outputs and the handle's landmark information and
// pivot ratio.  On failure nothing is written.
static vio_status finish(vio_cov *cv, const Staged &sg, double *pose_cov, double *lm_out) {
    const int64_t n = sg.n;
    const int D = sg.D;
    const int *h_status = (const int *)(cv->out.h + sg.nout);
    const int *hi = (const int *)(cv->in.h + sg.nd);
    char nm[64];
    if (h_status[0] >= 0)
        return fail(cv->err, VIO_ERR_NOT_FINITE, "pose covariance: pivot %d (%s) of the reduced H_pp_schur is not positive and finite",
                    h_status[0], var_name(hi[sg.iKeep + h_status[0]], nm, sizeof(nm)));
    if (n > 0 && h_status[1] != NO_BAD_LM)
        return fail(cv->err, VIO_ERR_NOT_FINITE, "landmark %d: its information is not positive definite and finite", h_status[1]);
    if (pose_cov) memcpy(pose_cov, cv->out.h + sg.o_cov, sizeof(double) * PD * PD);
    if (lm_out && n > 0) memcpy(lm_out, cv->out.h + sg.o_out, sizeof(double) * (size_t)n * D * D);
    cv->info.assign(cv->out.h + sg.o_info, cv->out.h + sg.o_info + (size_t)n * D * D);
    cv->last_n = n;
    cv->last_dim = D;
    cv->pivot_ratio = *(const double *)(h_status + 2);
    return VIO_OK;
}

static vio_status compute(vio_cov *cv, int D, int32_t gauge, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                          const double *pts_i, const double *pts_j, int64_t n, double *pose_cov, double *lm_out) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    DeviceScope dev(cv->cfg.device);
    if (!dev.ok) return fail(cv->err, VIO_ERR_HIP, "hipSetDevice(%d)", cv->cfg.device);
    Staged sg;
    vio_status st = stage(cv, D, gauge, m, lm, host, target, pts_i, pts_j, n, sg);
    if (st != VIO_OK) return st;
    const double t_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();

    if ((st = hip_ck(cv->err, hipEventRecord(cv->q.ev[0], cv->q.stream), "hipEventRecord")) != VIO_OK) return st;
    const CovPoseItem it = pose_item(cv, sg);
    k_cov_pose<<<1, POSE_NT, 0, cv->q.stream>>>(it.S, it.keep, it.n, it.cov, it.cc, it.status, it.ratio);
    if ((st = hip_ck(cv->err, hipGetLastError(), "k_cov_pose launch")) != VIO_OK) return st;
    if ((st = hip_ck(cv->err, hipEventRecord(cv->q.ev[1], cv->q.stream), "hipEventRecord")) != VIO_OK) return st;
    if (n > 0) {
        const CovLmArgs a = lm_args(cv, sg);
        if (D == 1) k_cov_landmarks<1><<<(unsigned)((n + LmNT<1>::v - 1) / LmNT<1>::v), LmNT<1>::v, 0, cv->q.stream>>>(a);
        else k_cov_landmarks<3><<<(unsigned)((n + LmNT<3>::v - 1) / LmNT<3>::v), LmNT<3>::v, 0, cv->q.stream>>>(a);
        if ((st = hip_ck(cv->err, hipGetLastError(), "k_cov_landmarks launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(cv->err, hipEventRecord(cv->q.ev[2], cv->q.stream), "hipEventRecord")) != VIO_OK) return st;
    if ((st = read_back(cv, sg)) != VIO_OK) return st;
    if ((st = hip_ck(cv->err, hipStreamSynchronize(cv->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;

    if ((st = finish(cv, sg, pose_cov, lm_out)) != VIO_OK) return st;
    float ms1 = 0, ms2 = 0;
    if ((st = hip_ck(cv->err, hipEventElapsedTime(&ms1, cv->q.ev[0], cv->q.ev[1]), "hipEventElapsedTime")) != VIO_OK ||
        (st = hip_ck(cv->err, hipEventElapsedTime(&ms2, cv->q.ev[1], cv->q.ev[2]), "hipEventElapsedTime")) != VIO_OK) {
        for (double &t : cv->timing) t = NAN;   // (the outputs are written: only the timings are unknown)
        return VIO_OK;
    }
    cv->timing[0] = t_host;
    cv->timing[1] = ms1;
    cv->timing[2] = ms2;
    cv->timing[3] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    return VIO_OK;
}

// a window's error, reported on the batch's first handle as well
static vio_status batch_fail(vio_cov *c0, vio_status st, int i, const vio_cov *cv) {
    char msg[sizeof(cv->err)];
    memcpy(msg, cv->err, sizeof(msg));
    return fail(c0->err, st, "vio_cov_compute_batch: window %d: %s", i, msg);
}

// The batch: every window staged in its own handle's buffers (one upload each), one table upload, k_cov_pose_batch and
// k_cov_landmarks_batch once for all windows, one read-back per window, one synchronisation.
static vio_status compute_batch(vio_cov *const *cvs, int32_t count, int32_t gauge, int32_t xyz, const vio_cov_batch_item *items,
                                vio_status *window_status) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    vio_cov *c0 = cvs[0];
    const int D = xyz ? 3 : 1;
    if (gauge != VIO_COV_GAUGE_NONE && gauge != VIO_COV_GAUGE_FIX_OLDEST) return fail(c0->err, VIO_ERR_BAD_ARG, "unknown gauge %d", gauge);
    // one device, one stream, no handle twice (a handle's buffers hold one window), no shard
    void *s0 = nullptr;
    for (int32_t i = 0; i < count; ++i) {
        vio_cov *cv = cvs[i];
        if (!cv) return fail(c0->err, VIO_ERR_BAD_ARG, "vio_cov_compute_batch: window %d: null handle", i);
        cv->err[0] = 0;
        if (cv->cfg.shard_count > 1) return fail(c0->err, VIO_ERR_UNSUPPORTED, "vio_cov_compute_batch: window %d: sharded context", i);
        if (cv->cfg.device != c0->cfg.device)
            return fail(c0->err, VIO_ERR_BAD_ARG, "vio_cov_compute_batch: window %d is on device %d, window 0 on %d: the contexts must share one device and one stream", i, cv->cfg.device, c0->cfg.device);
        for (int32_t j = 0; j < i; ++j)
            if (cvs[j] == cv) return fail(c0->err, VIO_ERR_BAD_ARG, "vio_cov_compute_batch: windows %d and %d are the same handle", j, i);
    }
    DeviceScope dev(c0->cfg.device);
    if (!dev.ok) return fail(c0->err, VIO_ERR_HIP, "hipSetDevice(%d)", c0->cfg.device);
    for (int32_t i = 0; i < count; ++i) {
        void *sp = nullptr;
        if (vio_get_stream(cvs[i]->ctx, &sp) != VIO_OK) return fail(c0->err, VIO_ERR_BAD_ARG, "vio_cov_compute_batch: window %d: vio_get_stream", i);
        if (i == 0) s0 = sp;
        else if (sp != s0) return fail(c0->err, VIO_ERR_BAD_ARG, "vio_cov_compute_batch: window %d is on another stream than window 0: the contexts must share one device and one stream", i);
    }
    vio_status st = VIO_OK;
    std::vector<Staged> sg(count);
    for (int32_t i = 0; i < count; ++i) {
        const vio_cov_batch_item &it = items[i];
        st = stage(cvs[i], D, gauge, it.m, it.lm, D == 1 ? it.host : nullptr, it.target, D == 1 ? it.pts_i : nullptr, it.pts_j, it.n, sg[i]);
        if (st != VIO_OK) return batch_fail(c0, st, i, cvs[i]);
    }
    // the tables: CovPoseItem[count] | CovLmArgs[count] | blk0[count + 1]
    const int lnt = D == 1 ? LmNT<1>::v : LmNT<3>::v;
    const size_t bPose = 0, bLm = align8(bPose + sizeof(CovPoseItem) * count), bBlk = align8(bLm + sizeof(CovLmArgs) * count),
                 nbytes = bBlk + sizeof(int) * ((size_t)count + 1);
    if ((st = c0->tab.ensure(c0->err, nbytes)) != VIO_OK) return st;
    char *ht = c0->tab.h;
    CovPoseItem *tp = (CovPoseItem *)(ht + bPose);
    CovLmArgs *tl = (CovLmArgs *)(ht + bLm);
    int *blk0 = (int *)(ht + bBlk);
    int64_t nblk = 0;
    for (int32_t i = 0; i < count; ++i) {
        tp[i] = pose_item(cvs[i], sg[i]);
        tl[i] = lm_args(cvs[i], sg[i]);
        blk0[i] = (int)nblk;
        nblk += (sg[i].n + lnt - 1) / lnt;
        if (nblk > INT32_MAX) return fail(c0->err, VIO_ERR_BAD_ARG, "vio_cov_compute_batch: too many landmarks in the batch");
    }
    blk0[count] = (int)nblk;
    hipStream_t stream = (hipStream_t)s0;
    const char *dt = c0->tab.d;
    if ((st = hip_ck(c0->err, hipMemcpyAsync(c0->tab.d, c0->tab.h, nbytes, hipMemcpyHostToDevice, stream), "table upload")) != VIO_OK) return st;
    const double t_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();

    if ((st = hip_ck(c0->err, hipEventRecord(c0->q.ev[0], stream), "hipEventRecord")) != VIO_OK) return st;
    k_cov_pose_batch<<<(unsigned)count, POSE_NT, 0, stream>>>((const CovPoseItem *)(dt + bPose));
    if ((st = hip_ck(c0->err, hipGetLastError(), "k_cov_pose_batch launch")) != VIO_OK) return st;
    if ((st = hip_ck(c0->err, hipEventRecord(c0->q.ev[1], stream), "hipEventRecord")) != VIO_OK) return st;
    if (nblk > 0) {
        const CovLmArgs *dl = (const CovLmArgs *)(dt + bLm);
        const int *db = (const int *)(dt + bBlk);
        if (D == 1) k_cov_landmarks_batch<1><<<(unsigned)nblk, LmNT<1>::v, 0, stream>>>(dl, db, count);
        else k_cov_landmarks_batch<3><<<(unsigned)nblk, LmNT<3>::v, 0, stream>>>(dl, db, count);
        if ((st = hip_ck(c0->err, hipGetLastError(), "k_cov_landmarks_batch launch")) != VIO_OK) return st;
    }
    if ((st = hip_ck(c0->err, hipEventRecord(c0->q.ev[2], stream), "hipEventRecord")) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i)
        if ((st = read_back(cvs[i], sg[i])) != VIO_OK) return batch_fail(c0, st, i, cvs[i]);
    if ((st = hip_ck(c0->err, hipStreamSynchronize(stream), "hipStreamSynchronize")) != VIO_OK) return st;

    vio_status ret = VIO_OK;
    for (int32_t i = 0; i < count; ++i) {
        const vio_status wst = finish(cvs[i], sg[i], items[i].pose_cov, items[i].lm_out);
        if (window_status) window_status[i] = wst;
        if (wst != VIO_OK) ret = wst;
    }
    const float ms1 = elapsed_ms(c0->q.ev[0], c0->q.ev[1]), ms2 = elapsed_ms(c0->q.ev[1], c0->q.ev[2]);
    double tm[4] = {NAN, NAN, NAN, NAN};
    if (!std::isnan(ms1) && !std::isnan(ms2)) {
        tm[0] = t_host;
        tm[1] = ms1;
        tm[2] = ms2;
        tm[3] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    }
    for (int32_t i = 0; i < count; ++i) memcpy(cvs[i]->timing, tm, sizeof(tm));
    return ret;
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
    if (cv->q.create_events() != hipSuccess) { vio_cov_destroy(cv); return VIO_ERR_HIP; }
    *out = cv;
    return VIO_OK;
}

void vio_cov_destroy(vio_cov *cv) {
    if (!cv) return;
    DeviceScope dev(cv->cfg.device);
    cv->q.release();
    delete cv;                              // (the buffers free themselves)
}

vio_status vio_cov_set_config(vio_cov *cv, const vio_config *cfg) {
    if (!cv || !cfg) return VIO_ERR_BAD_ARG;
    if (cfg->device != cv->cfg.device) return fail(cv->err, VIO_ERR_BAD_ARG, "device %d: the handle was made for device %d", cfg->device, cv->cfg.device);
    if (cfg->shard_count > 1) return fail(cv->err, VIO_ERR_UNSUPPORTED, "sharded context");
    const vio_config &o = cv->cfg;
    if (cfg->ext_fixed != o.ext_fixed || cfg->loss_type != o.loss_type || cfg->loss_delta != o.loss_delta ||
        cfg->reproj_sqrt_info != o.reproj_sqrt_info || memcmp(cfg->gravity, o.gravity, sizeof(o.gravity)) != 0 || cfg->item_policy != o.item_policy)
        cv->relinearize = true;
    cv->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_cov_pivot_ratio(vio_cov *cv, double *ratio) {
    if (!cv || !ratio) return VIO_ERR_BAD_ARG;
    if (cv->last_n < 0) return fail(cv->err, VIO_ERR_BAD_ARG, "no successful compute yet");
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

vio_status vio_cov_compute_batch(vio_cov *const *cvs, int32_t count, int32_t gauge, int32_t xyz, const vio_cov_batch_item *items,
                                 vio_status *window_status) {
    if (count < 0 || (count > 0 && (!cvs || !items))) return VIO_ERR_BAD_ARG;
    if (count == 0) return VIO_OK;
    if (!cvs[0]) return VIO_ERR_BAD_ARG;
    cvs[0]->err[0] = 0;
    return compute_batch(cvs, count, gauge, xyz, items, window_status);
}

vio_status vio_cov_landmark_information(vio_cov *cv, int64_t n, double *info) {
    if (!cv) return VIO_ERR_BAD_ARG;
    if (cv->last_n < 0 || n != cv->last_n) return fail(cv->err, VIO_ERR_BAD_ARG, "no compute with n=%lld to read back", (long long)n);
    if (info && n > 0) memcpy(info, cv->info.data(), sizeof(double) * cv->info.size());
    return VIO_OK;
}

vio_status vio_cov_timing(vio_cov *cv, double *out4) {
    if (!cv || !out4) return VIO_ERR_BAD_ARG;
    memcpy(out4, cv->timing, sizeof(cv->timing));
    return VIO_OK;
}

}   // extern "C"

