// vio_detect.hip — libvio_detect_hip.so: Shi-Tomasi corner detection with setMask for many images in one call
// (include/vio_detect.h).
// Contraction is off as in vio_flow.hip; with this arithmetic it cannot change a bit (vio_detect_math.h).  No floating-point atomics.
// The kernels, described where they are, are in vio_detect_body.inc, which libvio_frame_hip compiles too; what the
// host side shares with that library is in vio_detect_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_detect.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_detect_math.h"

#include "vio_detect_host.h"
#include "vio_detect_body.inc"

constexpr int MAX_ITEMS = 4096;

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_detect {
    int device = 0;
    ErrText err = {0};
    vio_detect_config cfg = DET_DEFAULTS;
    Twin<char> tab;                                      // item descriptors | tracked points
    Twin<uint8_t> img;                                   // the images and the masks
    Twin<char> out;                                      // DetRes per item | keep_order | new_pts
    DevBuf<double> r;
    DevBuf<uint32_t> cand;
    DevBuf<char> scratch;                                // tkey | kept_xy
    StreamEvents<6> q;                                   // events: upload, setmask, response, candidates, select start; end
    double timing[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
};

namespace {

vio_status check_image(vio_detect *h, int i, int width, int height, int stride) {
    if (width < 1 || height < 1 || width > VIO_DETECT_MAX_DIM || height > VIO_DETECT_MAX_DIM || stride < width)
        return fail(h->err, VIO_ERR_BAD_ARG, "item %d: width and height must be in [1, %d] and stride >= width", i, VIO_DETECT_MAX_DIM);
    return VIO_OK;
}

}  // namespace

extern "C" {

int32_t vio_detect_version(void) { return VIO_DETECT_VERSION; }

const char *vio_detect_last_error(const vio_detect *h) { return h ? h->err : "NULL handle"; }

vio_status vio_detect_create(int32_t device, void *stream, vio_detect **out) { return create_handle(device, stream, out, vio_detect_destroy); }

void vio_detect_destroy(vio_detect *h) { destroy_handle(h); }

vio_status vio_detect_set_config(vio_detect *h, const vio_detect_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = det_check_config(h->err, "vio_detect_set_config", cfg);
    if (st != VIO_OK) return st;
    h->cfg = *cfg;
    h->cfg.reserved = 0;
    return VIO_OK;
}

vio_status vio_detect_timing(const vio_detect *h, double *out6) {
    if (!h || !out6) return VIO_ERR_BAD_ARG;
    std::memcpy(out6, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_detect_batch(vio_detect *h, int32_t count, const vio_detect_item *items, vio_detect_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_detect_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    // every argument of every item first: nothing is written or launched on an error
    std::vector<DetItemD> its((size_t)count);
    std::vector<int64_t> at((size_t)count * 2, 0);       // the byte offsets of an item's image and mask in the image buffer
    int64_t b_img = 0;
    DetTotals T;
    vio_status st;
    for (int i = 0; i < count; ++i) {
        const vio_detect_item &it = items[i];
        if ((st = det_check_counts(h->err, "", i, it.n_tracked, it.max_total)) != VIO_OK || (st = check_image(h, i, it.width, it.height, it.stride)) != VIO_OK)
            return st;
        if (!it.img || (it.n_tracked > 0 && (!it.tracked || !it.track_cnt || !it.keep_order)) || (it.max_total > 0 && !it.new_pts))
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: img, and tracked, track_cnt, keep_order, new_pts where they have rows, are required", i);
        DetItemD &d = its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        if ((st = det_check_tracked(h->err, "", i, it.tracked, it.n_tracked, it.width, it.height, &d.active)) != VIO_OK) return st;
        det_item(d, T, it.width, it.height, it.width, it.n_tracked, it.max_total, it.mask != nullptr);      // (rows tightly packed)
        if (!d.active) continue;                         // (nothing of it is staged)
        const int64_t px = (int64_t)it.width * it.height;
        at[2 * (size_t)i] = b_img; b_img += px;
        if (d.has_mask) { at[2 * (size_t)i + 1] = b_img; b_img += px; }
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const DetSizes S = det_sizes(count, T.n_trk, T.n_new);
    if ((st = h->tab.ensure(h->err, S.b_tab)) != VIO_OK || (st = h->img.ensure(h->err, (size_t)b_img)) != VIO_OK ||
        (st = h->out.ensure(h->err, S.b_out)) != VIO_OK || (st = h->r.ensure(h->err, sizeof(double) * (size_t)T.n_r)) != VIO_OK ||
        (st = h->cand.ensure(h->err, sizeof(uint32_t) * (size_t)T.n_cand)) != VIO_OK || (st = h->scratch.ensure(h->err, S.b_scratch)) != VIO_OK)
        return st;
    for (int i = 0; i < count; ++i) {                    // (the image buffer is where it stays now)
        const vio_detect_item &it = items[i];
        DetItemD &d = its[(size_t)i];
        if (!d.active) continue;
        d.img = h->img.d + at[2 * (size_t)i];
        copy_rows(h->img.h + at[2 * (size_t)i], it.width, it.img, it.stride, it.width, it.height);
        if (!d.has_mask) continue;
        d.mask = h->img.d + at[2 * (size_t)i + 1];
        copy_rows(h->img.h + at[2 * (size_t)i + 1], it.width, it.mask, it.stride, it.width, it.height);
    }
    det_fill_table(h->tab.h, S, count, items, its.data());
    const DetArgs a = det_args(h->cfg, count, S, h->tab.d, h->out.d, h->scratch.d, h->r.d, h->cand.d);
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->tab.d, h->tab.h, S.b_tab, hipMemcpyHostToDevice, q) != hipSuccess ||
        (b_img && hipMemcpyAsync(h->img.d, h->img.h, (size_t)b_img, hipMemcpyHostToDevice, q) != hipSuccess) ||
        hipMemsetAsync(h->out.d, 0, S.b_res, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    det_launch(a, q, T.n_trk > 0, T.max_tiles > 0, T.max_tiles, &h->q.ev[2]);
    (void)hipEventRecord(h->q.ev[5], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, S.b_out, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    const vio_status ret = det_unpack(h->err, h->out.h, S, count, items, its.data(), results);
    const auto t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    for (int k = 1; k < 5; ++k) h->timing[k] = elapsed_ms(h->q.ev[k], h->q.ev[k + 1]);
    h->timing[5] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return ret;
}

vio_status vio_detect_response(vio_detect *h, const uint8_t *img, int32_t width, int32_t height, int32_t stride, double *out) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!img || !out) return fail(h->err, VIO_ERR_BAD_ARG, "vio_detect_response: a NULL array");
    vio_status st = check_image(h, 0, width, height, stride);
    if (st != VIO_OK) return st;
    DetItemD d;
    DetTotals T;
    std::memset(&d, 0, sizeof(d));
    d.active = 1;
    det_item(d, T, width, height, width, 0, 0, false);
    const size_t px = (size_t)width * (size_t)height;
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_res = align256(sizeof(DetRes));
    if ((st = h->tab.ensure(h->err, sizeof(DetItemD))) != VIO_OK || (st = h->img.ensure(h->err, px)) != VIO_OK ||
        (st = h->out.ensure(h->err, b_res + sizeof(double) * px)) != VIO_OK || (st = h->r.ensure(h->err, sizeof(double) * px)) != VIO_OK)
        return st;
    d.img = h->img.d;
    std::memcpy(h->tab.h, &d, sizeof(d));
    copy_rows(h->img.h, width, img, stride, width, height);
    DetArgs a = det_args(h->cfg, 1);
    a.items = (const DetItemD *)h->tab.d;
    a.r = h->r.d;
    a.res = (DetRes *)h->out.d;                          // (n_kept = 0 and no mask: every pixel is allowed, nothing else is read)
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->tab.d, h->tab.h, sizeof(DetItemD), hipMemcpyHostToDevice, q) != hipSuccess ||
        hipMemcpyAsync(h->img.d, h->img.h, px, hipMemcpyHostToDevice, q) != hipSuccess || hipMemsetAsync(h->out.d, 0, b_res, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    hipLaunchKernelGGL(k_detect_response, dim3((unsigned)d.tiles, 1, 1), dim3(NT), 0, q, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    double *stage = (double *)(h->out.h + b_res);
    if (hipMemcpyAsync(stage, h->r.d, sizeof(double) * px, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    std::memcpy(out, stage, sizeof(double) * px);
    return VIO_OK;
}

}  // extern "C"
