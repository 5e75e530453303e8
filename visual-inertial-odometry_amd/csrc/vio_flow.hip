// vio_flow.hip — libvio_flow_hip.so: pyramidal Lucas-Kanade tracking of the keypoints of many image pairs in one call
// (include/vio_flow.h).
// Contraction is off: products and sums round as the host restatement's (tests/flow_reference.py) do.  No floating-point atomics.
// The kernels, described where they are, are in vio_flow_body.inc, which libvio_frame_hip compiles too; what the
// host side shares with that library is in vio_flow_host.h.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_flow.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_flow_math.h"

#include "vio_flow_host.h"
#include "vio_flow_body.inc"

constexpr int MAX_ITEMS = 16384;

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_flow {
    int device = 0;
    ErrText err = {0};
    vio_flow_config cfg = FLOW_DEFAULTS;
    Twin<char> tab;                                      // item descriptors | keypoint descriptors
    Twin<uint8_t> pyr;                                   // level 0 of every image (the part uploaded) | the levels above
    Twin<FlowOut> out;
    vio_flow_back_config bcfg = FLOW_BACK_DEFAULTS;      // the forward-backward check (include/vio_flow_back.h), off
    Twin<FlowBackOut> bout;
    StreamEvents<4> q;                                   // events: upload start, pyramid start, tracking start, end
    double timing[4] = {NAN, NAN, NAN, NAN};
};

namespace {

vio_status check_image(vio_flow *h, int i, int width, int height, int stride) {
    if (width < 1 || height < 1 || width > VIO_FLOW_MAX_DIM || height > VIO_FLOW_MAX_DIM || stride < width)
        return fail(h->err, VIO_ERR_BAD_ARG, "item %d: width and height must be in [1, %d] and stride >= width", i, VIO_FLOW_MAX_DIM);
    int32_t w[MAXL], hh[MAXL];
    if (!flow_level_dims(width, height, h->cfg.levels, w, hh))
        return fail(h->err, VIO_ERR_BAD_ARG, "item %d: a %d x %d image has a level below 2 x 2 among its %d", i, width, height, h->cfg.levels);
    return VIO_OK;
}

// vio_flow_track_batch, and with the check enabled vio_flow_track_back_batch (back may be NULL): fn names the call in errors
vio_status track_run(vio_flow *h, const char *fn, int32_t count, const vio_flow_item *items, float *next_pts, vio_flow_pt_info *info,
                     vio_flow_back_info *back) {
    const bool check = h->bcfg.enabled != 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !next_pts)))
        return fail(h->err, VIO_ERR_BAD_ARG, "%s: count outside [0, %d] or a NULL array", fn, MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const int L = h->cfg.levels;
    size_t total = 0;
    for (int i = 0; i < count; ++i) {
        const vio_flow_item &it = items[i];
        if (it.n_pts < 0 || it.n_pts > VIO_FLOW_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: n_pts must be in [0, %d]", i, VIO_FLOW_MAX_POINTS);
        const vio_status st = check_image(h, i, it.width, it.height, it.stride);
        if (st != VIO_OK) return st;
        if (it.n_pts > 0 && (!it.img_prev || !it.img_next || !it.prev_pts))
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: img_prev, img_next and prev_pts are required", i);
        total += (size_t)it.n_pts;
    }
    if (total == 0) return VIO_OK;
    // the pyramid buffer: level 0 of every image of an item with keypoints, then the levels above; the descriptor tables
    std::vector<FlowItemD> its((size_t)count);
    std::vector<int64_t> at((size_t)count * 2 * MAXL, 0);       // the levels' offsets in the pyramid buffer: [item][prev, next][level]
    int64_t off = 0, max_px[MAXL] = {0};
    for (int i = 0; i < count; ++i) {
        FlowItemD &d = its[(size_t)i];
        int64_t *prev = &at[(size_t)i * 2 * MAXL], *next = prev + MAXL;
        std::memset(&d, 0, sizeof(d));
        if (items[i].n_pts == 0) continue;
        flow_level_dims(items[i].width, items[i].height, L, d.w, d.h);
        flow_item(d, L, d.w, d.h, d.w);                         // (rows tightly packed)
        prev[0] = off; off += (int64_t)d.w[0] * d.h[0];
        next[0] = off; off += (int64_t)d.w[0] * d.h[0];
        for (int l = 0; l < L; ++l) max_px[l] = std::max(max_px[l], (int64_t)d.w[l] * d.h[l]);
    }
    const size_t b_l0 = (size_t)off;
    off = (int64_t)align256(b_l0);
    for (int i = 0; i < count; ++i) {
        const FlowItemD &d = its[(size_t)i];
        int64_t *prev = &at[(size_t)i * 2 * MAXL], *next = prev + MAXL;
        if (!d.active) continue;
        for (int l = 1; l < L; ++l) {
            prev[l] = off; off += (int64_t)d.w[l] * d.h[l];
            next[l] = off; off += (int64_t)d.w[l] * d.h[l];
        }
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_it = align256(sizeof(FlowItemD) * (size_t)count), b_tab = b_it + sizeof(FlowPt) * total;
    vio_status st;
    if ((st = h->tab.ensure(h->err, b_tab)) != VIO_OK || (st = h->pyr.ensure(h->err, (size_t)off)) != VIO_OK ||
        (st = h->out.ensure(h->err, sizeof(FlowOut) * total)) != VIO_OK ||
        (check && back && (st = h->bout.ensure(h->err, sizeof(FlowBackOut) * total)) != VIO_OK))
        return st;
    for (int i = 0; i < count; ++i) {                    // (the pyramid buffer is where it stays now)
        FlowItemD &d = its[(size_t)i];
        const int64_t *prev = &at[(size_t)i * 2 * MAXL], *next = prev + MAXL;
        for (int l = 0; d.active && l < L; ++l) { d.prev[l] = h->pyr.d + prev[l]; d.next[l] = h->pyr.d + next[l]; }
    }
    std::memcpy(h->tab.h, its.data(), sizeof(FlowItemD) * (size_t)count);
    FlowPt *hp = (FlowPt *)(h->tab.h + b_it);
    size_t row = 0;
    for (int i = 0; i < count; ++i) {
        const vio_flow_item &it = items[i];
        const FlowItemD &d = its[(size_t)i];
        if (!d.active) continue;
        copy_rows(h->pyr.h + at[(size_t)i * 2 * MAXL], it.width, it.img_prev, it.stride, it.width, it.height);
        copy_rows(h->pyr.h + at[(size_t)i * 2 * MAXL + MAXL], it.width, it.img_next, it.stride, it.width, it.height);
        flow_fill_pts(hp + row, i, it);
        row += (size_t)it.n_pts;
    }
    const FlowArgs a = flow_args((const FlowItemD *)h->tab.d, (const FlowPt *)(h->tab.d + b_it), h->out.d, total, L, h->cfg);
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess ||
        hipMemcpyAsync(h->pyr.d, h->pyr.h, b_l0, hipMemcpyHostToDevice, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    flow_launch_pyramids(q, a.items, 2 * count, 1, L, max_px);
    (void)hipEventRecord(h->q.ev[2], q);
    if (check) flow_launch_track_back(q, flow_back_args(a.items, a.pts, a.out, back ? h->bout.d : nullptr, total, L, h->cfg, h->bcfg), h->cfg.inverse != 0);
    else flow_launch_track(q, a, h->cfg.inverse != 0);
    (void)hipEventRecord(h->q.ev[3], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    const size_t outb = sizeof(FlowOut) * total;
    if (hipMemcpyAsync(h->out.h, h->out.d, outb, hipMemcpyDeviceToHost, q) != hipSuccess ||
        (check && back && hipMemcpyAsync(h->bout.h, h->bout.d, sizeof(FlowBackOut) * total, hipMemcpyDeviceToHost, q) != hipSuccess) ||
        hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    const vio_status ret = flow_unpack(h->err, h->out.h, count, items, next_pts, info);
    if (check && back) flow_unpack_back(h->bout.h, count, items, back);
    const auto t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    h->timing[2] = elapsed_ms(h->q.ev[2], h->q.ev[3]);
    h->timing[3] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return ret;
}

}  // namespace

extern "C" {

int32_t vio_flow_version(void) { return VIO_FLOW_VERSION; }

const char *vio_flow_last_error(const vio_flow *h) { return h ? h->err : "NULL handle"; }

vio_status vio_flow_create(int32_t device, void *stream, vio_flow **out) { return create_handle(device, stream, out, vio_flow_destroy); }

void vio_flow_destroy(vio_flow *h) { destroy_handle(h); }

vio_status vio_flow_set_config(vio_flow *h, const vio_flow_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = flow_check_config(h->err, "vio_flow_set_config", cfg);
    if (st != VIO_OK) return st;
    if (h->bcfg.enabled && h->bcfg.levels > cfg->levels)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_flow_set_config: %d levels are fewer than the %d of the forward-backward check", cfg->levels, h->bcfg.levels);
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_flow_set_back(vio_flow *h, const vio_flow_back_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = flow_check_back(h->err, "vio_flow_set_back", cfg, h->cfg.levels);
    if (st != VIO_OK) return st;
    h->bcfg = cfg ? *cfg : FLOW_BACK_DEFAULTS;
    return VIO_OK;
}

vio_status vio_flow_timing(const vio_flow *h, double *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_flow_track_batch(vio_flow *h, int32_t count, const vio_flow_item *items, float *next_pts, vio_flow_pt_info *info) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    return track_run(h, "vio_flow_track_batch", count, items, next_pts, info, nullptr);
}

vio_status vio_flow_track_back_batch(vio_flow *h, int32_t count, const vio_flow_item *items, float *next_pts, vio_flow_pt_info *info,
                                     vio_flow_back_info *back) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!h->bcfg.enabled) return fail(h->err, VIO_ERR_BAD_ARG, "vio_flow_track_back_batch: the check is off (vio_flow_set_back)");
    return track_run(h, "vio_flow_track_back_batch", count, items, next_pts, info, back);
}

vio_status vio_flow_pyramid(vio_flow *h, const uint8_t *img, int32_t width, int32_t height, int32_t stride, uint8_t *out) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!img || !out) return fail(h->err, VIO_ERR_BAD_ARG, "vio_flow_pyramid: a NULL array");
    vio_status st = check_image(h, 0, width, height, stride);
    if (st != VIO_OK) return st;
    const int L = h->cfg.levels;
    FlowItemD d;
    std::memset(&d, 0, sizeof(d));
    flow_level_dims(width, height, L, d.w, d.h);
    flow_item(d, L, d.w, d.h, d.w);
    int64_t off = 0, max_px[MAXL] = {0};
    int64_t at[MAXL] = {0};
    for (int l = 0; l < L; ++l) {
        at[l] = off;
        max_px[l] = (int64_t)d.w[l] * d.h[l];
        off += max_px[l];
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    if ((st = h->tab.ensure(h->err, sizeof(FlowItemD))) != VIO_OK || (st = h->pyr.ensure(h->err, (size_t)off)) != VIO_OK) return st;
    for (int l = 0; l < L; ++l) d.prev[l] = d.next[l] = h->pyr.d + at[l];
    std::memcpy(h->tab.h, &d, sizeof(d));
    copy_rows(h->pyr.h, width, img, stride, width, height);
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->tab.d, h->tab.h, sizeof(FlowItemD), hipMemcpyHostToDevice, q) != hipSuccess ||
        hipMemcpyAsync(h->pyr.d, h->pyr.h, (size_t)max_px[0], hipMemcpyHostToDevice, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    flow_launch_pyramids(q, (const FlowItemD *)h->tab.d, 1, 1, L, max_px);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    const size_t rest = (size_t)(off - max_px[0]);
    if ((rest && hipMemcpyAsync(h->pyr.h + max_px[0], h->pyr.d + max_px[0], rest, hipMemcpyDeviceToHost, q) != hipSuccess) ||
        hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    std::memcpy(out, h->pyr.h, (size_t)off);
    return VIO_OK;
}

}  // extern "C"
