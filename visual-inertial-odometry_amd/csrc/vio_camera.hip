// vio_camera.hip — libvio_camera_hip.so: the lift, undistortedPoints and rejectWithF through the reference's four camera models, for
// many streams with a camera each in one call (include/vio_camera.h).
//
// The kernels are k_reject_lift and k_reject_ransac of vio_reject_body.inc, the text libvio_reject_hip and libvio_frame_hip compile,
// here against vio_camera_host.h: the tables carry a camera slot, the lift is cam_lift of vio_camera_math.h, the virtual pixel and the
// normalised point divide by the ray's z.  The RANSAC behind the prologue is untouched.  The camera table (VIO_CAMERA_MAX_SLOTS CamDev)
// lives in device memory; a workgroup of k_reject_ransac reads its pair's camera once, uniformly, k_reject_lift per point.
// Contraction is off; no floating-point atomics; every sum has a fixed order.
// spaceToPlane (include/vio_camera_project.h) is k_camera_project of vio_camera_project_body.inc over
// vio_camera_project_math.h, with a device table of its own (VIO_CAMERA_MAX_SLOTS CamProj): CamDev is shared with libvio_frame_hip
// and stays as it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_camera.h"
#include "../../include/vio_camera_project.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_camera_math.h"
#include "vio_camera_project_math.h"
#include "vio_sfm_math.h"

constexpr int MAX_ITEMS = VIO_CAMERA_MAX_ITEMS;
static_assert(VIO_CAMERA_MAX_POINTS == VIO_REJECT_MAX_POINTS && VIO_CAMERA_MAX_ITEMS == VIO_REJECT_MAX_ITEMS, "the limits are vio_reject.h's");

#include "vio_camera_host.h"
#include "vio_reject_body.inc"
#include "vio_camera_project_body.inc"

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_camera {
    int device = 0;
    ErrText err = {0};
    vio_reject_config cfg = REJ_DEFAULTS;
    Twin<CamDev> cams;                                       // the camera table
    bool cams_dirty = true;
    Twin<CamProj> proj;                                      // the projection table (include/vio_camera_project.h)
    bool proj_dirty = true;
    Twin<char> tab;                                          // descriptors | staged floats | staged ids
    Twin<char> out;                                          // results | masks, or un_pts | velocity | flags, or rays | angles | flags
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

bool slot_set(const vio_camera *h, int slot) { return slot >= 0 && slot < VIO_CAMERA_MAX_SLOTS && h->cams.h[slot].set; }

// the table and the camera table go up on q; false: the upload failed
bool upload(vio_camera *h, size_t b_tab) {
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (h->cams_dirty) {
        if (hipMemcpyAsync(h->cams.d, h->cams.h, sizeof(CamDev) * VIO_CAMERA_MAX_SLOTS, hipMemcpyHostToDevice, q) != hipSuccess) return false;
        h->cams_dirty = false;
    }
    if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess) return false;
    (void)hipEventRecord(h->q.ev[1], q);
    return true;
}

// One per-point item of a lift or an undistort call, as the two entry points hand it to run_lift.
struct PointItem {
    int32_t n, m, slot;
    const float *pts;
    const int64_t *ids, *prev_ids;
    const float *prev_un_pts;
    double dt;
};

// k_reject_lift over `count` items; the outputs come back in h->out: bare: rays [P][3] | angles [P][2] | flags [P]; otherwise
// un_pts [P][2] | velocity [P][2] | flags [P].  its: the descriptors as they went up.
vio_status run_lift(vio_camera *h, int count, const std::vector<PointItem> &in, bool bare, std::vector<LiftItem> &its, size_t &n_total,
                    std::chrono::steady_clock::time_point t0) {
    its.assign((size_t)count, LiftItem());
    int64_t n_pts = 0, n_flt = 0, n_ids = 0;
    int max_n = 0;
    for (int i = 0; i < count; ++i) {
        const PointItem &it = in[(size_t)i];
        LiftItem &d = its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        d.n = it.n; d.m = it.m; d.dt = it.m > 0 ? it.dt : 1.0; d.slot = it.slot;
        d.active = finite_pts(it.pts, it.n);
        d.o_pts = n_flt; n_flt += 2 * (int64_t)it.n;
        d.o_prev = n_flt; n_flt += 2 * (int64_t)it.m;
        d.o_ids = n_ids; n_ids += bare ? 0 : (int64_t)it.n + it.m;
        d.o_out = n_pts; n_pts += it.n;
        max_n = std::max(max_n, it.n);
    }
    n_total = (size_t)n_pts;
    if (max_n == 0) return VIO_OK;
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_it = align256(sizeof(LiftItem) * (size_t)count), b_flt = align256(sizeof(float) * (size_t)n_flt);
    const size_t b_tab = b_it + b_flt + sizeof(int64_t) * (size_t)n_ids;
    const size_t b_val = bare ? sizeof(double) * 5 * n_total : sizeof(float) * 4 * n_total, b_out = b_val + n_total;
    vio_status st;
    if ((st = h->tab.ensure(h->err, b_tab)) != VIO_OK || (st = h->out.ensure(h->err, b_out)) != VIO_OK) return st;
    std::memcpy(h->tab.h, its.data(), sizeof(LiftItem) * (size_t)count);
    float *hf = (float *)(h->tab.h + b_it);
    int64_t *hi = (int64_t *)(h->tab.h + b_it + b_flt);
    for (int i = 0; i < count; ++i) {
        const PointItem &it = in[(size_t)i];
        const LiftItem &d = its[(size_t)i];
        if (d.n > 0) {
            std::memcpy(hf + d.o_pts, it.pts, sizeof(float) * 2 * (size_t)d.n);
            if (!bare) std::memcpy(hi + d.o_ids, it.ids, sizeof(int64_t) * (size_t)d.n);
        }
        if (d.m > 0) {
            std::memcpy(hf + d.o_prev, it.prev_un_pts, sizeof(float) * 2 * (size_t)d.m);
            std::memcpy(hi + d.o_ids + d.n, it.prev_ids, sizeof(int64_t) * (size_t)d.m);
        }
    }
    LiftArgs a;
    std::memset(&a, 0, sizeof(a));
    a.items = (const LiftItem *)h->tab.d;
    a.pts = (const float *)(h->tab.d + b_it);
    a.ids = (const long long *)(h->tab.d + b_it + b_flt);
    a.un = (float *)h->out.d; a.vel = a.un + 2 * n_total;
    a.lifted = (double *)h->out.d; a.angles = a.lifted + 3 * n_total;
    a.flags = (uint8_t *)(h->out.d + b_val);
    a.cams = h->cams.d; a.bare = bare; a.count = count;
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    if (!upload(h, b_tab)) return fail_synced(h, "upload failed");
    rej_launch_lift(q, a, max_n);
    (void)hipEventRecord(h->q.ev[2], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, b_out, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    return VIO_OK;
}

// the flags of item d: any bad lift, the clamped points
void fold_flags(const uint8_t *flags, const LiftItem &d, bool &bad, int &clamped) {
    bad = false; clamped = 0;
    for (int k = 0; k < d.n; ++k) {
        const uint8_t f = flags[d.o_out + k];
        bad |= (f & CAM_FLAG_BAD) != 0;
        clamped += (f & CAM_FLAG_CLAMPED) != 0;
    }
}

}  // namespace

extern "C" {

int32_t vio_camera_version(void) { return VIO_CAMERA_VERSION; }

const char *vio_camera_last_error(const vio_camera *h) { return h ? h->err : "NULL handle"; }

vio_status vio_camera_create(int32_t device, void *stream, vio_camera **out) {
    return create_handle(device, stream, out, vio_camera_destroy, [](vio_camera *h) {
        if (h->cams.ensure(h->err, sizeof(CamDev) * VIO_CAMERA_MAX_SLOTS) != VIO_OK) return false;
        std::memset(h->cams.h, 0, sizeof(CamDev) * VIO_CAMERA_MAX_SLOTS);
        if (h->proj.ensure(h->err, sizeof(CamProj) * VIO_CAMERA_MAX_SLOTS) != VIO_OK) return false;
        std::memset(h->proj.h, 0, sizeof(CamProj) * VIO_CAMERA_MAX_SLOTS);
        return true;
    });
}

void vio_camera_destroy(vio_camera *h) { destroy_handle(h); }

vio_status vio_camera_set(vio_camera *h, int32_t slot, const vio_camera_model *cam) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_CAMERA_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_set: slot must be in [0, %d)", VIO_CAMERA_MAX_SLOTS);
    const vio_status st = cam_check_model(h->err, cam);
    if (st != VIO_OK) return st;
    h->cams.h[slot] = cam_device_form(*cam);
    h->cams_dirty = true;
    h->proj.h[slot] = cam_project_form(*cam);               // (inv_poly of the slot is cleared)
    h->proj_dirty = true;
    return VIO_OK;
}

vio_status vio_camera_set_config(vio_camera *h, const vio_reject_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = rej_check_config(h->err, "vio_camera_set_config", cfg);
    if (st != VIO_OK) return st;
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_camera_timing(const vio_camera *h, double *out3) {
    if (!h || !out3) return VIO_ERR_BAD_ARG;
    std::memcpy(out3, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_camera_lift_batch(vio_camera *h, int32_t count, const vio_camera_lift_item *items, vio_camera_lift_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_lift_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<PointItem> in((size_t)count);
    for (int i = 0; i < count; ++i) {
        const vio_camera_lift_item &it = items[i];
        if (it.n < 0 || it.n > VIO_CAMERA_MAX_POINTS) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: n must be in [0, %d]", i, VIO_CAMERA_MAX_POINTS);
        if (it.n > 0 && (!it.pts || !it.rays)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: pts and rays are required", i);
        if (!slot_set(h, it.slot)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: camera slot %d is outside [0, %d) or not set", i, it.slot, VIO_CAMERA_MAX_SLOTS);
        in[(size_t)i] = PointItem{it.n, 0, it.slot, it.pts, nullptr, nullptr, nullptr, 1.0};
    }
    std::vector<LiftItem> its;
    size_t n_total = 0;
    const vio_status st = run_lift(h, count, in, true, its, n_total, t0);
    if (st != VIO_OK) return st;
    const double *rays = (const double *)h->out.h, *angles = rays + 3 * n_total;
    const uint8_t *flags = (const uint8_t *)(h->out.h + sizeof(double) * 5 * n_total);
    vio_status ret = VIO_OK;
    for (int i = 0; i < count; ++i) {
        const LiftItem &d = its[(size_t)i];
        bool bad = false;
        int clamped = 0;
        if (d.n > 0) {
            std::memcpy(items[i].rays, rays + 3 * (size_t)d.o_out, sizeof(double) * 3 * (size_t)d.n);
            if (items[i].angles) std::memcpy(items[i].angles, angles + 2 * (size_t)d.o_out, sizeof(double) * 2 * (size_t)d.n);
            fold_flags(flags, d, bad, clamped);
        }
        results[i].status = d.active ? VIO_OK : VIO_ERR_NOT_FINITE;
        results[i].n_clamped = clamped;
        if (!d.active) {
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: a point is not finite", i);
            ret = VIO_ERR_NOT_FINITE;
        }
    }
    if (n_total > 0) h->timing[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

vio_status vio_camera_undistort_batch(vio_camera *h, int32_t count, const vio_camera_undistort_item *items, vio_camera_lift_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_undistort_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<PointItem> in((size_t)count);
    for (int i = 0; i < count; ++i) {
        const vio_camera_undistort_item &it = items[i];
        if (it.n < 0 || it.n > VIO_CAMERA_MAX_POINTS || it.m < 0 || it.m > VIO_CAMERA_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: n and m must be in [0, %d]", i, VIO_CAMERA_MAX_POINTS);
        if ((it.n > 0 && (!it.pts || !it.ids || !it.un_pts || !it.velocity)) || (it.m > 0 && (!it.prev_ids || !it.prev_un_pts)))
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: pts, ids, un_pts, velocity, prev_ids, prev_un_pts are required where they have rows", i);
        if (it.m > 0 && !(std::isfinite(it.dt) && it.dt > 0.0)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: dt must be finite and > 0", i);
        if (!slot_set(h, it.slot)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: camera slot %d is outside [0, %d) or not set", i, it.slot, VIO_CAMERA_MAX_SLOTS);
        in[(size_t)i] = PointItem{it.n, it.m, it.slot, it.pts, it.ids, it.prev_ids, it.prev_un_pts, it.dt};
    }
    std::vector<LiftItem> its;
    size_t n_total = 0;
    const vio_status st = run_lift(h, count, in, false, its, n_total, t0);
    if (st != VIO_OK) return st;
    const float *un = (const float *)h->out.h, *vel = un + 2 * n_total;
    const uint8_t *flags = (const uint8_t *)(h->out.h + sizeof(float) * 4 * n_total);
    vio_status ret = VIO_OK;
    for (int i = 0; i < count; ++i) {
        const LiftItem &d = its[(size_t)i];
        bool bad = false;
        int clamped = 0;
        if (d.n > 0) fold_flags(flags, d, bad, clamped);
        bad = bad || !d.active;
        if (bad) {                                              // (the kernel wrote NaN itself where the host saw the pixel)
            for (int k = 0; k < 2 * d.n; ++k) { items[i].un_pts[k] = NAN; items[i].velocity[k] = NAN; }
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: a point is not finite, or its lift is not", i);
            ret = VIO_ERR_NOT_FINITE;
        } else if (d.n > 0) {
            std::memcpy(items[i].un_pts, un + 2 * (size_t)d.o_out, sizeof(float) * 2 * (size_t)d.n);
            std::memcpy(items[i].velocity, vel + 2 * (size_t)d.o_out, sizeof(float) * 2 * (size_t)d.n);
        }
        results[i].status = bad ? VIO_ERR_NOT_FINITE : VIO_OK;
        results[i].n_clamped = bad ? 0 : clamped;
    }
    if (n_total > 0) h->timing[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

vio_status vio_camera_reject_batch(vio_camera *h, int32_t count, const vio_camera_reject_item *items, vio_reject_result *results, uint8_t *mask) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_reject_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    // every argument of every item first: nothing is written or launched on an error
    std::vector<RejPair> ps((size_t)count);
    int64_t n_pts = 0, n_flt = 0, n_corr = 0;
    bool any = false;
    for (int i = 0; i < count; ++i) {
        const vio_camera_reject_item &it = items[i];
        if (it.n < 0 || it.n > VIO_CAMERA_MAX_POINTS) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: n must be in [0, %d]", i, VIO_CAMERA_MAX_POINTS);
        if (it.n > 0 && (!it.cur_pts || !it.forw_pts)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: cur_pts and forw_pts are required", i);
        if (!slot_set(h, it.slot)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: camera slot %d is outside [0, %d) or not set", i, it.slot, VIO_CAMERA_MAX_SLOTS);
        n_pts += it.n;
    }
    if (n_pts > 0 && !mask) return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_reject_batch: NULL mask");
    n_pts = 0;
    for (int i = 0; i < count; ++i) {
        const vio_camera_reject_item &it = items[i];
        RejPair &p = ps[(size_t)i];
        std::memset(&p, 0, sizeof(p));
        p.n = it.n; p.pair = it.pair; p.slot = it.slot;
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
        RansacArgs a;
        std::memset(&a, 0, sizeof(a));
        a.cams = h->cams.d;
        a.focal = h->cfg.focal_length; a.thr = h->cfg.f_threshold * h->cfg.f_threshold;
        a.seed = h->cfg.seed; a.hyps = h->cfg.ransac_hypotheses;
        a.pairs = (const RejPair *)h->tab.d;
        a.pts = (const float *)(h->tab.d + b_it);
        a.corr = (double *)h->scratch.d;
        a.flag = (int32_t *)(h->scratch.d + b_corr);
        a.res = (RejRes *)h->out.d;
        a.mask = (uint8_t *)(h->out.d + b_res);
        const auto t1 = std::chrono::steady_clock::now();
        hipStream_t q = h->q.stream;
        if (!upload(h, b_tab)) return fail_synced(h, "upload failed");
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
        if (p.active && res[i].status != VIO_ERR_NOT_FINITE) {
            o.status = res[i].status; o.hyp = res[i].hyp;
            o.n_inliers = std::min(std::max(res[i].n_inliers, 0), p.n);
            std::memcpy(o.F, res[i].F, sizeof(o.F));
            std::memcpy(mask + p.o_pt, hm + p.o_pt, (size_t)p.n);
        } else if (p.finite && !p.active) {                     // the size gate
            o.status = VIO_OK; o.hyp = -1; o.n_inliers = p.n;
            if (p.n > 0) std::memset(mask + p.o_pt, 1, (size_t)p.n);
        } else {                                                // a pixel that is not finite, or (on the device) a lift that is not
            o.status = VIO_ERR_NOT_FINITE; o.hyp = -1; o.n_inliers = 0;
            std::memset(mask + p.o_pt, 0, (size_t)p.n);
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: a point is not finite, or its lift is not", i);
            ret = VIO_ERR_NOT_FINITE;
        }
    }
    if (any) h->timing[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

// ---- include/vio_camera_project.h ----------------------------------------------------------------------------

vio_status vio_camera_set_inv_poly(vio_camera *h, int32_t slot, int32_t n, const double *inv_poly) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!slot_set(h, slot)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_set_inv_poly: camera slot %d is outside [0, %d) or not set", slot, VIO_CAMERA_MAX_SLOTS);
    if (h->proj.h[slot].model != VIO_CAMERA_MODEL_SCARAMUZZA) return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_set_inv_poly: slot %d does not hold a SCARAMUZZA camera", slot);
    if (n < 1 || n > VIO_CAMERA_INV_POLY_MAX || !inv_poly) return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_set_inv_poly: n must be in [1, %d] and inv_poly given", VIO_CAMERA_INV_POLY_MAX);
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(inv_poly[i])) return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_set_inv_poly: coefficient %d is not finite", i);
    CamProj &C = h->proj.h[slot];
    for (int i = 0; i < VIO_CAMERA_INV_POLY_MAX; ++i) C.inv[i] = i < n ? inv_poly[i] : 0.0;
    C.n_inv = n;
    h->proj_dirty = true;
    return VIO_OK;
}

vio_status vio_camera_project_batch(vio_camera *h, int32_t count, const vio_camera_project_item *items, vio_camera_project_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_camera_project_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<ProjItem> its((size_t)count);
    int64_t n_pts = 0;
    int max_n = 0;
    for (int i = 0; i < count; ++i) {
        const vio_camera_project_item &it = items[i];
        if (it.n < 0 || it.n > VIO_CAMERA_MAX_POINTS) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: n must be in [0, %d]", i, VIO_CAMERA_MAX_POINTS);
        if (it.n > 0 && (!it.points || !it.pixels)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: points and pixels are required", i);
        if (!slot_set(h, it.slot)) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: camera slot %d is outside [0, %d) or not set", i, it.slot, VIO_CAMERA_MAX_SLOTS);
        const CamProj &C = h->proj.h[it.slot];
        if (C.model == VIO_CAMERA_MODEL_SCARAMUZZA && C.n_inv < 1)
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: SCARAMUZZA slot %d has no inv_poly (vio_camera_set_inv_poly)", i, it.slot);
        ProjItem &d = its[(size_t)i];
        d.n = it.n; d.slot = it.slot; d.o_pt = n_pts;
        n_pts += it.n;
        max_n = std::max(max_n, it.n);
    }
    const size_t n_total = (size_t)n_pts;
    if (max_n > 0) {
        DeviceScope dev(h->device);
        if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
        const size_t b_it = align256(sizeof(ProjItem) * (size_t)count), b_tab = b_it + sizeof(double) * 3 * n_total;
        const size_t b_pix = sizeof(double) * 2 * n_total, b_out = b_pix + n_total;
        vio_status st;
        if ((st = h->tab.ensure(h->err, b_tab)) != VIO_OK || (st = h->out.ensure(h->err, b_out)) != VIO_OK) return st;
        std::memcpy(h->tab.h, its.data(), sizeof(ProjItem) * (size_t)count);
        double *hp = (double *)(h->tab.h + b_it);
        for (int i = 0; i < count; ++i)
            if (items[i].n > 0) std::memcpy(hp + 3 * its[(size_t)i].o_pt, items[i].points, sizeof(double) * 3 * (size_t)items[i].n);
        ProjArgs a;
        std::memset(&a, 0, sizeof(a));
        a.items = (const ProjItem *)h->tab.d;
        a.pts = (const double *)(h->tab.d + b_it);
        a.pix = (double *)h->out.d;
        a.flags = (uint8_t *)(h->out.d + b_pix);
        a.cams = h->proj.d; a.count = count;
        const auto t1 = std::chrono::steady_clock::now();
        hipStream_t q = h->q.stream;
        (void)hipEventRecord(h->q.ev[0], q);
        if (h->proj_dirty) {
            if (hipMemcpyAsync(h->proj.d, h->proj.h, sizeof(CamProj) * VIO_CAMERA_MAX_SLOTS, hipMemcpyHostToDevice, q) != hipSuccess) return fail_synced(h, "upload failed");
            h->proj_dirty = false;
        }
        if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess) return fail_synced(h, "upload failed");
        (void)hipEventRecord(h->q.ev[1], q);
        hipLaunchKernelGGL(k_camera_project, dim3((unsigned)((max_n + NT - 1) / NT), (unsigned)count), dim3(NT), 0, q, a);
        (void)hipEventRecord(h->q.ev[2], q);
        if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
        if (hipMemcpyAsync(h->out.h, h->out.d, b_out, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
            return fail_synced(h, "kernel or read-back failed");
        h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
        h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    }
    const double *pix = (const double *)h->out.h;
    const uint8_t *flags = max_n > 0 ? (const uint8_t *)(h->out.h + sizeof(double) * 2 * n_total) : nullptr;
    vio_status ret = VIO_OK;
    for (int i = 0; i < count; ++i) {
        const ProjItem &d = its[(size_t)i];
        int flagged = 0;
        bool bad = false;
        if (d.n > 0) {
            std::memcpy(items[i].pixels, pix + 2 * (size_t)d.o_pt, sizeof(double) * 2 * (size_t)d.n);
            if (items[i].flags) std::memcpy(items[i].flags, flags + d.o_pt, (size_t)d.n);
            for (int k = 0; k < d.n; ++k) {
                const uint8_t f = flags[d.o_pt + k];
                flagged += f != 0;
                bad |= (f & VIO_CAMERA_PROJECT_NOT_FINITE) != 0;
            }
        }
        results[i].status = bad ? VIO_ERR_NOT_FINITE : VIO_OK;
        results[i].n_flagged = flagged;
        if (bad) {
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: a point or its pixel is not finite", i);
            ret = VIO_ERR_NOT_FINITE;
        }
    }
    if (max_n > 0) h->timing[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

}  // extern "C"
