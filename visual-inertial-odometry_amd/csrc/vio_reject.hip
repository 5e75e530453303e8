// vio_reject.hip — libvio_reject_hip.so: rejectWithF and undistortedPoints for many streams in one call (include/vio_reject.h,
// DESIGN.md section 21).
//
//   k_reject_lift     a thread per point, every item of the call in the grid (blockIdx.y).  Undistort: the lift, the normalised point
//                     as float, then the id lookup: prev_ids goes through LDS in chunks of VIO_REJECT_ID_CHUNK, every thread scans the
//                     chunk for its id and keeps the first match; the velocity from the matched previous point.  Bare lift: the two
//                     doubles.
//   k_reject_ransac   one 256-thread workgroup per pair.  Prologue: both point sets lifted (the same rej_lift: the bits are
//                     k_reject_lift's), mapped to virtual pixels and rounded to float, into the pair's scratch slice as doubles.
//                     Then rounds of VIO_REJECT_ROUND hypotheses: lane h of the first wavefront samples and fits hypothesis base + h
//                     with its 9 x 9 normal matrix and eigenvectors in LDS (entry-major, lane-minor: no per-lane arrays, no bank
//                     conflicts); all threads score (hypothesis, correspondence) pairs into integer LDS counters; thread 0 folds the
//                     round into the running winner (count, lowest h).  The refit: the inlier flags thread per correspondence, the
//                     centroids, the scales and the 45 entries of the normal matrix's upper triangle each summed by one thread in
//                     correspondence order, the eigenproblem by thread 0 in the same LDS; the final mask thread per correspondence.
// The two kernels are in vio_reject_body.inc, which libvio_frame_hip compiles too; what the host side shares
// with it is in vio_reject_host.h.
// Contraction is off: products and sums round as the restatement's (tests/reject_reference.py) do.  No floating-point atomics; every
// sum has a fixed order, so repeated calls are bitwise identical and a pair's result does not depend on its batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_reject.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_reject_math.h"
#include "vio_sfm_math.h"

constexpr int MAX_ITEMS = VIO_REJECT_MAX_ITEMS;

#include "vio_reject_host.h"
#include "vio_reject_body.inc"

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_reject {
    int device = 0;
    ErrText err = {0};
    vio_reject_config cfg = REJ_DEFAULTS;
    vio_reject_camera camera = {};
    RejCam cam = {};
    bool have_camera = false;
    Twin<char> tab;                                          // descriptors | staged floats | staged ids
    Twin<char> out;                                          // results | masks, or un_pts | velocity, or the lifted doubles
    DevBuf<char> scratch;                                    // corr | flags
    StreamEvents<3> q;                                       // events: upload start, kernel start, kernel end
    double timing[3] = {NAN, NAN, NAN};
};

namespace {

bool finite_pts(const float *p, int n) {
    for (int k = 0; k < 2 * n; ++k)
        if (!std::isfinite(p[k])) return false;
    return true;
}

// the lift kernel over `count` items whose descriptors, floats and ids are staged in h->tab; the outputs come back in h->out
vio_status run_lift(vio_reject *h, int count, int max_n, size_t b_tab, size_t o_flt, size_t o_ids, size_t n_pts, bool bare,
                    std::chrono::steady_clock::time_point t0) {
    const size_t b_out = bare ? sizeof(double) * 2 * n_pts : sizeof(float) * 4 * n_pts;
    LiftArgs a;
    std::memset(&a, 0, sizeof(a));
    a.items = (const LiftItem *)h->tab.d;
    a.pts = (const float *)(h->tab.d + o_flt);
    a.ids = (const long long *)(h->tab.d + o_ids);
    a.un = (float *)h->out.d; a.vel = a.un + 2 * n_pts;
    a.lifted = (double *)h->out.d;
    a.cam = h->cam; a.bare = bare; a.count = count;
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess) return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    rej_launch_lift(q, a, max_n);
    (void)hipEventRecord(h->q.ev[2], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, b_out, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    return VIO_OK;
}

}  // namespace

extern "C" {

int32_t vio_reject_version(void) { return VIO_REJECT_VERSION; }

const char *vio_reject_last_error(const vio_reject *h) { return h ? h->err : "NULL handle"; }

vio_status vio_reject_create(int32_t device, void *stream, vio_reject **out) { return create_handle(device, stream, out, vio_reject_destroy); }

void vio_reject_destroy(vio_reject *h) { destroy_handle(h); }

vio_status vio_reject_set_camera(vio_reject *h, const vio_reject_camera *cam) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = rej_check_camera(h->err, "vio_reject_set_camera", cam);
    if (st != VIO_OK) return st;
    rej_set_camera(*cam, h->camera, h->cam);
    h->have_camera = true;
    return VIO_OK;
}

vio_status vio_reject_set_config(vio_reject *h, const vio_reject_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = rej_check_config(h->err, "vio_reject_set_config", cfg);
    if (st != VIO_OK) return st;
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_reject_timing(const vio_reject *h, double *out3) {
    if (!h || !out3) return VIO_ERR_BAD_ARG;
    std::memcpy(out3, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_reject_batch(vio_reject *h, int32_t count, const vio_reject_item *items, vio_reject_result *results, uint8_t *mask) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_reject_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    if (!h->have_camera) return fail(h->err, VIO_ERR_BAD_ARG, "vio_reject_batch: no camera set");
    const auto t0 = std::chrono::steady_clock::now();
    // every argument of every item first: nothing is written or launched on an error
    std::vector<RejPair> ps((size_t)count);
    int64_t n_pts = 0, n_flt = 0, n_corr = 0;
    bool any = false;
    for (int i = 0; i < count; ++i) {
        const vio_reject_item &it = items[i];
        if (it.n < 0 || it.n > VIO_REJECT_MAX_POINTS) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: n must be in [0, %d]", i, VIO_REJECT_MAX_POINTS);
        if (it.n > 0 && (!it.cur_pts || !it.forw_pts)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: cur_pts and forw_pts are required", i);
        n_pts += it.n;
    }
    if (n_pts > 0 && !mask) return fail(h->err, VIO_ERR_BAD_ARG, "vio_reject_batch: NULL mask");
    n_pts = 0;
    for (int i = 0; i < count; ++i) {
        const vio_reject_item &it = items[i];
        RejPair &p = ps[(size_t)i];
        std::memset(&p, 0, sizeof(p));
        p.n = it.n; p.pair = it.pair;
        p.finite = finite_pts(it.cur_pts, it.n) && finite_pts(it.forw_pts, it.n);
        p.active = p.finite && it.n >= MINP;
        p.o_pt = n_pts; n_pts += it.n;
        if (!p.active) continue;                             // (nothing of it is staged)
        p.o_pts = n_flt; n_flt += 4 * (int64_t)it.n;
        p.o_corr = n_corr; n_corr += 4 * (int64_t)it.n;
        any = true;
    }
    if (any) {
        DeviceScope dev(h->device);
        if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
        const size_t b_it = align256(sizeof(RejPair) * (size_t)count), b_tab = b_it + sizeof(float) * (size_t)n_flt;
        const size_t b_res = align256(sizeof(RejRes) * (size_t)count), b_out = b_res + (size_t)n_pts;
        const size_t b_corr = align256(sizeof(double) * (size_t)n_corr);
        vio_status st;
        if ((st = h->tab.ensure(h->err, b_tab)) != VIO_OK || (st = h->out.ensure(h->err, b_out)) != VIO_OK ||
            (st = h->scratch.ensure(h->err, b_corr + sizeof(int32_t) * (size_t)n_pts)) != VIO_OK)
            return st;
        std::memcpy(h->tab.h, ps.data(), sizeof(RejPair) * (size_t)count);
        float *hf = (float *)(h->tab.h + b_it);
        for (int i = 0; i < count; ++i) {
            const RejPair &p = ps[(size_t)i];
            if (!p.active) continue;
            std::memcpy(hf + p.o_pts, items[i].cur_pts, sizeof(float) * 2 * (size_t)p.n);
            std::memcpy(hf + p.o_pts + 2 * (size_t)p.n, items[i].forw_pts, sizeof(float) * 2 * (size_t)p.n);
        }
        RansacArgs a = rej_ransac_args(h->cam, h->camera, h->cfg);
        a.pairs = (const RejPair *)h->tab.d;
        a.pts = (const float *)(h->tab.d + b_it);
        a.corr = (double *)h->scratch.d;
        a.flag = (int32_t *)(h->scratch.d + b_corr);
        a.res = (RejRes *)h->out.d;
        a.mask = (uint8_t *)(h->out.d + b_res);
        const auto t1 = std::chrono::steady_clock::now();
        hipStream_t q = h->q.stream;
        (void)hipEventRecord(h->q.ev[0], q);
        if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess) return fail_synced(h, "upload failed");
        (void)hipEventRecord(h->q.ev[1], q);
        hipLaunchKernelGGL(k_reject_ransac, dim3((unsigned)count), dim3(NT), 0, q, a);
        (void)hipEventRecord(h->q.ev[2], q);
        if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
        if (hipMemcpyAsync(h->out.h, h->out.d, b_out, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
            return fail_synced(h, "kernel or read-back failed");
        h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
        h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    }
    vio_status ret = VIO_OK;
    const RejRes *res = (const RejRes *)h->out.h;
    const uint8_t *hm = any ? (const uint8_t *)(h->out.h + align256(sizeof(RejRes) * (size_t)count)) : nullptr;
    for (int i = 0; i < count; ++i) {
        const RejPair &p = ps[(size_t)i];
        vio_reject_result &o = results[i];
        o.reserved = 0;
        for (int k = 0; k < 9; ++k) o.F[k] = NAN;
        if (p.active) {
            o.status = res[i].status; o.hyp = res[i].hyp;
            o.n_inliers = std::min(std::max(res[i].n_inliers, 0), p.n);
            std::memcpy(o.F, res[i].F, sizeof(o.F));
            std::memcpy(mask + p.o_pt, hm + p.o_pt, (size_t)p.n);
        } else if (p.finite) {                                  // the size gate
            o.status = VIO_OK; o.hyp = -1; o.n_inliers = p.n;
            if (p.n > 0) std::memset(mask + p.o_pt, 1, (size_t)p.n);
        } else {
            o.status = VIO_ERR_NOT_FINITE; o.hyp = -1; o.n_inliers = 0;
            std::memset(mask + p.o_pt, 0, (size_t)p.n);
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: a point is not finite", i);
            ret = VIO_ERR_NOT_FINITE;
        }
    }
    if (any) h->timing[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

vio_status vio_reject_undistort_batch(vio_reject *h, int32_t count, const vio_reject_undistort_item *items, int32_t *status) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !status)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_reject_undistort_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    if (!h->have_camera) return fail(h->err, VIO_ERR_BAD_ARG, "vio_reject_undistort_batch: no camera set");
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<LiftItem> its((size_t)count);
    int64_t n_pts = 0, n_flt = 0, n_ids = 0;
    int max_n = 0;
    for (int i = 0; i < count; ++i) {
        const vio_reject_undistort_item &it = items[i];
        if (it.n < 0 || it.n > VIO_REJECT_MAX_POINTS || it.m < 0 || it.m > VIO_REJECT_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: n and m must be in [0, %d]", i, VIO_REJECT_MAX_POINTS);
        if ((it.n > 0 && (!it.pts || !it.ids || !it.un_pts || !it.velocity)) || (it.m > 0 && (!it.prev_ids || !it.prev_un_pts)))
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: pts, ids, un_pts, velocity, prev_ids, prev_un_pts are required where they have rows", i);
        if (it.m > 0 && !(std::isfinite(it.dt) && it.dt > 0.0)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: dt must be finite and > 0", i);
        LiftItem &d = its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        d.n = it.n; d.m = it.m; d.dt = it.m > 0 ? it.dt : 1.0;
        d.active = finite_pts(it.pts, it.n);
        d.o_pts = n_flt; n_flt += 2 * (int64_t)it.n;
        d.o_prev = n_flt; n_flt += 2 * (int64_t)it.m;
        d.o_ids = n_ids; n_ids += (int64_t)it.n + it.m;
        d.o_out = n_pts; n_pts += it.n;
        max_n = std::max(max_n, it.n);
    }
    vio_status ret = VIO_OK;
    if (max_n > 0) {
        DeviceScope dev(h->device);
        if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
        const size_t b_it = align256(sizeof(LiftItem) * (size_t)count), b_flt = align256(sizeof(float) * (size_t)n_flt);
        const size_t b_tab = b_it + b_flt + sizeof(int64_t) * (size_t)n_ids;
        vio_status st;
        if ((st = h->tab.ensure(h->err, b_tab)) != VIO_OK || (st = h->out.ensure(h->err, sizeof(float) * 4 * (size_t)n_pts)) != VIO_OK) return st;
        std::memcpy(h->tab.h, its.data(), sizeof(LiftItem) * (size_t)count);
        float *hf = (float *)(h->tab.h + b_it);
        int64_t *hi = (int64_t *)(h->tab.h + b_it + b_flt);
        for (int i = 0; i < count; ++i) {
            const vio_reject_undistort_item &it = items[i];
            const LiftItem &d = its[(size_t)i];
            if (d.n > 0) { std::memcpy(hf + d.o_pts, it.pts, sizeof(float) * 2 * (size_t)d.n); std::memcpy(hi + d.o_ids, it.ids, sizeof(int64_t) * (size_t)d.n); }
            if (d.m > 0) {
                std::memcpy(hf + d.o_prev, it.prev_un_pts, sizeof(float) * 2 * (size_t)d.m);
                std::memcpy(hi + d.o_ids + d.n, it.prev_ids, sizeof(int64_t) * (size_t)d.m);
            }
        }
        st = run_lift(h, count, max_n, b_tab, b_it, b_it + b_flt, (size_t)n_pts, false, t0);
        if (st != VIO_OK) return st;
        const float *un = (const float *)h->out.h, *vel = un + 2 * (size_t)n_pts;
        for (int i = 0; i < count; ++i) {
            const LiftItem &d = its[(size_t)i];
            if (d.n == 0) continue;
            std::memcpy(items[i].un_pts, un + 2 * (size_t)d.o_out, sizeof(float) * 2 * (size_t)d.n);
            std::memcpy(items[i].velocity, vel + 2 * (size_t)d.o_out, sizeof(float) * 2 * (size_t)d.n);
        }
    }
    for (int i = 0; i < count; ++i) {
        status[i] = its[(size_t)i].active ? VIO_OK : VIO_ERR_NOT_FINITE;
        if (!its[(size_t)i].active) {
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: a point is not finite", i);
            ret = VIO_ERR_NOT_FINITE;
        }
    }
    if (max_n > 0) h->timing[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

vio_status vio_reject_lift(vio_reject *h, int32_t n, const float *pts, double *out) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (n < 0 || n > VIO_REJECT_MAX_POINTS || (n > 0 && (!pts || !out)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_reject_lift: n outside [0, %d] or a NULL array", VIO_REJECT_MAX_POINTS);
    if (!h->have_camera) return fail(h->err, VIO_ERR_BAD_ARG, "vio_reject_lift: no camera set");
    if (n == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    LiftItem d;
    std::memset(&d, 0, sizeof(d));
    d.n = n; d.active = 1; d.dt = 1.0;
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_it = align256(sizeof(LiftItem)), b_tab = b_it + sizeof(float) * 2 * (size_t)n;
    vio_status st;
    if ((st = h->tab.ensure(h->err, b_tab)) != VIO_OK || (st = h->out.ensure(h->err, sizeof(double) * 2 * (size_t)n)) != VIO_OK) return st;
    std::memcpy(h->tab.h, &d, sizeof(d));
    std::memcpy(h->tab.h + b_it, pts, sizeof(float) * 2 * (size_t)n);
    st = run_lift(h, 1, n, b_tab, b_it, b_it, (size_t)n, true, t0);
    if (st != VIO_OK) return st;
    std::memcpy(out, h->out.h, sizeof(double) * 2 * (size_t)n);
    h->timing[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VIO_OK;
}

}  // extern "C"
