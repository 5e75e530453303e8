// vio_detect.hip — libvio_detect_hip.so: Shi-Tomasi corner detection with setMask for many images in one call
// (include/vio_detect.h).
//
//   k_detect_setmask     one workgroup per image: the greedy loop below over the tracked points, key (track_cnt, -index), disc <=.
//                        Leaves the kept centres and their indices in output order.
//   k_detect_response    a TX x TY tile per workgroup, every image of the call in the grid (blockIdx.z): the tile with a halo of 2 in
//                        LDS, the Sobel products at a halo of 1, the 3 x 3 box sums, R.  Integers up to the one sqrt.  Each wavefront
//                        then folds the R bits of its allowed pixels into the image's maximum with one integer atomicMax (the bit
//                        patterns of non-negative doubles order as the doubles do, and a maximum does not depend on the order).
//   k_detect_candidates  the same grid, one thread per pixel: the threshold, the 8 neighbours, allowed; a candidate's pixel index goes
//                        to the image's list through an integer counter.  The order of arrival is arbitrary.
//   k_detect_select      one workgroup per image: the greedy loop over the candidates, key (R bits, pixel index), disc <.
// The greedy loop: "take the sorted list in order and accept what no earlier accepted one is close to" is "repeatedly take the best
// remaining entry and strike those close to it".  A round is one pass over the list (strike against the last winner, else fold into
// the maximum), one reduction and one barrier; the rounds are bounded by a count known at launch.  No sort, no spin-waits, no
// synchronisation between workgroups; a thread only ever strikes the entries it reads itself.
// Contraction is off as in vio_flow.hip; with this arithmetic it cannot change a bit (vio_detect_math.h).  No floating-point atomics.
// The kernels themselves are in vio_detect_body.inc, which libvio_frame_hip compiles too; the host side is here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vio_detect.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_detect_math.h"

#include "vio_detect_body.inc"

constexpr int MAX_ITEMS = 4096;

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_detect {
    int device = 0;
    ErrText err = {0};
    vio_detect_config cfg = {VIO_DETECT_DEFAULT_QUALITY, VIO_DETECT_DEFAULT_MIN_DISTANCE, 0};
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

vio_status fail_synced(vio_detect *h, const char *msg) { (void)hipStreamSynchronize(h->q.stream); return fail(h->err, VIO_ERR_HIP, "%s", msg); }

vio_status check_image(vio_detect *h, int i, int width, int height, int stride) {
    if (width < 1 || height < 1 || width > VIO_DETECT_MAX_DIM || height > VIO_DETECT_MAX_DIM || stride < width)
        return fail(h->err, VIO_ERR_BAD_ARG, "item %d: width and height must be in [1, %d] and stride >= width", i, VIO_DETECT_MAX_DIM);
    return VIO_OK;
}

void copy_rows(uint8_t *dst, const uint8_t *src, int width, int height, int stride) {
    for (int y = 0; y < height; ++y) std::memcpy(dst + (size_t)y * (size_t)width, src + (size_t)y * (size_t)stride, (size_t)width);
}

void set_geometry(DetItemD &d, int width, int height) {
    d.w = width; d.h = height; d.pitch = width;          // (rows tightly packed)
    d.tiles_x = (width + TX - 1) / TX;
    d.tiles = d.tiles_x * ((height + TY - 1) / TY);
}

}  // namespace

extern "C" {

int32_t vio_detect_version(void) { return VIO_DETECT_VERSION; }

const char *vio_detect_last_error(const vio_detect *h) { return h ? h->err : "NULL handle"; }

vio_status vio_detect_create(int32_t device, void *stream, vio_detect **out) {
    if (!out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VIO_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return VIO_ERR_BAD_ARG;
    DeviceScope dev(device);
    if (!dev.ok) return VIO_ERR_HIP;
    vio_detect *h = new (std::nothrow) vio_detect();
    if (!h) return VIO_ERR_BAD_ARG;
    h->device = device;
    if (h->q.open_stream(stream) != hipSuccess) { delete h; return VIO_ERR_HIP; }
    if (h->q.create_events() != hipSuccess) { vio_detect_destroy(h); return VIO_ERR_HIP; }
    *out = h;
    return VIO_OK;
}

void vio_detect_destroy(vio_detect *h) {
    if (!h) return;
    DeviceScope dev(h->device);
    h->q.release();
    delete h;                                            // (the buffers free themselves)
}

vio_status vio_detect_set_config(vio_detect *h, const vio_detect_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg || !(cfg->quality > 0.0 && cfg->quality <= 1.0) || cfg->min_distance < 0)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_detect_set_config: quality in (0, 1], min_distance >= 0");
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
    int64_t b_img = 0, n_r = 0, n_cand = 0, n_trk = 0, n_new = 0;
    int max_tiles = 0;
    for (int i = 0; i < count; ++i) {
        const vio_detect_item &it = items[i];
        if (it.n_tracked < 0 || it.n_tracked > VIO_DETECT_MAX_POINTS || it.max_total < 0 || it.max_total > VIO_DETECT_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: n_tracked and max_total must be in [0, %d]", i, VIO_DETECT_MAX_POINTS);
        const vio_status st = check_image(h, i, it.width, it.height, it.stride);
        if (st != VIO_OK) return st;
        if (!it.img || (it.n_tracked > 0 && (!it.tracked || !it.track_cnt || !it.keep_order)) || (it.max_total > 0 && !it.new_pts))
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: img, and tracked, track_cnt, keep_order, new_pts where they have rows, are required", i);
        DetItemD &d = its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        d.active = 1;
        for (int k = 0; k < it.n_tracked; ++k) {
            const double x = it.tracked[2 * k], y = it.tracked[2 * k + 1];
            if (!std::isfinite(x) || !std::isfinite(y)) { d.active = 0; continue; }
            const double rx = std::nearbyint(x), ry = std::nearbyint(y);
            if (rx < 0.0 || rx >= (double)it.width || ry < 0.0 || ry >= (double)it.height)
                return fail(h->err, VIO_ERR_BAD_ARG, "item %d: tracked point %d (%g, %g) rounds to a pixel outside the %d x %d image", i, k, x, y,
                            it.width, it.height);
        }
        set_geometry(d, it.width, it.height);
        d.n_tracked = it.n_tracked; d.max_total = it.max_total;
        d.has_mask = it.mask != nullptr;
        d.trk = (int32_t)n_trk; d.newp = (int32_t)n_new;
        n_trk += it.n_tracked; n_new += it.max_total;
        if (!d.active) continue;                         // (nothing of it is staged)
        const int64_t px = (int64_t)it.width * it.height;
        at[2 * (size_t)i] = b_img; b_img += px;
        if (d.has_mask) { at[2 * (size_t)i + 1] = b_img; b_img += px; }
        d.r = n_r; n_r += px;
        d.cand = n_cand; n_cand += (int64_t)std::max(it.width - 2, 0) * std::max(it.height - 2, 0);
        max_tiles = std::max(max_tiles, d.tiles);
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_it = align256(sizeof(DetItemD) * (size_t)count), b_tab = b_it + sizeof(DetTrk) * (size_t)n_trk;
    const size_t b_res = align256(sizeof(DetRes) * (size_t)count), b_keep = align256(sizeof(int32_t) * (size_t)n_trk);
    const size_t b_out = b_res + b_keep + sizeof(float) * 2 * (size_t)n_new;
    const size_t b_key = align256(sizeof(unsigned long long) * (size_t)n_trk);
    vio_status st;
    if ((st = h->tab.ensure(h->err, b_tab)) != VIO_OK || (st = h->img.ensure(h->err, (size_t)b_img)) != VIO_OK ||
        (st = h->out.ensure(h->err, b_out)) != VIO_OK || (st = h->r.ensure(h->err, sizeof(double) * (size_t)n_r)) != VIO_OK ||
        (st = h->cand.ensure(h->err, sizeof(uint32_t) * (size_t)n_cand)) != VIO_OK ||
        (st = h->scratch.ensure(h->err, b_key + sizeof(int32_t) * 2 * (size_t)n_trk)) != VIO_OK)
        return st;
    for (int i = 0; i < count; ++i) {                    // (the image buffer is where it stays now)
        DetItemD &d = its[(size_t)i];
        if (!d.active) continue;
        d.img = h->img.d + at[2 * (size_t)i];
        if (d.has_mask) d.mask = h->img.d + at[2 * (size_t)i + 1];
    }
    std::memcpy(h->tab.h, its.data(), sizeof(DetItemD) * (size_t)count);
    DetTrk *ht = (DetTrk *)(h->tab.h + b_it);
    for (int i = 0; i < count; ++i) {
        const vio_detect_item &it = items[i];
        const DetItemD &d = its[(size_t)i];
        for (int k = 0; k < it.n_tracked; ++k) {
            DetTrk &t = ht[d.trk + k];
            t.cx = 0; t.cy = 0; t.cnt = 0; t.pad = 0;
            if (!d.active) continue;
            t.cx = (int32_t)std::nearbyint((double)it.tracked[2 * k]); t.cy = (int32_t)std::nearbyint((double)it.tracked[2 * k + 1]);
            t.cnt = it.track_cnt[k];
        }
        if (!d.active) continue;
        copy_rows(h->img.h + at[2 * (size_t)i], it.img, it.width, it.height, it.stride);
        if (d.has_mask) copy_rows(h->img.h + at[2 * (size_t)i + 1], it.mask, it.width, it.height, it.stride);
    }
    DetArgs a;
    a.items = (const DetItemD *)h->tab.d;
    a.trk = (const DetTrk *)(h->tab.d + b_it);
    a.r = h->r.d; a.cand = h->cand.d;
    a.tkey = (unsigned long long *)h->scratch.d;
    a.kept_xy = (int32_t *)(h->scratch.d + b_key);
    a.res = (DetRes *)h->out.d;
    a.keep_order = (int32_t *)(h->out.d + b_res);
    a.new_pts = (float *)(h->out.d + b_res + b_keep);
    a.quality = h->cfg.quality; a.d2 = det_d2(h->cfg.min_distance); a.count = count;
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess ||
        (b_img && hipMemcpyAsync(h->img.d, h->img.h, (size_t)b_img, hipMemcpyHostToDevice, q) != hipSuccess) ||
        hipMemsetAsync(h->out.d, 0, b_res, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    if (n_trk > 0) hipLaunchKernelGGL(k_detect_setmask, dim3((unsigned)count), dim3(NT_MASK), 0, q, a);
    (void)hipEventRecord(h->q.ev[2], q);
    if (max_tiles > 0) hipLaunchKernelGGL(k_detect_response, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(NT), 0, q, a);
    (void)hipEventRecord(h->q.ev[3], q);
    if (max_tiles > 0) hipLaunchKernelGGL(k_detect_candidates, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(NT), 0, q, a);
    (void)hipEventRecord(h->q.ev[4], q);
    if (max_tiles > 0) hipLaunchKernelGGL(k_detect_select, dim3((unsigned)count), dim3(NT_SEL), 0, q, a);
    (void)hipEventRecord(h->q.ev[5], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, b_out, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    vio_status ret = VIO_OK;
    const DetRes *res = (const DetRes *)h->out.h;
    const int32_t *keep = (const int32_t *)(h->out.h + b_res);
    const float *newp = (const float *)(h->out.h + b_res + b_keep);
    for (int i = 0; i < count; ++i) {
        const vio_detect_item &it = items[i];
        const DetItemD &d = its[(size_t)i];
        vio_detect_result &o = results[i];
        o.status = VIO_OK; o.n_kept = 0; o.n_new = 0; o.n_candidates = 0; o.max_response = 0.0;
        if (d.active) {
            // (the counts are the device's; they are bounded here so that no copy can leave the caller's arrays whatever they hold)
            o.n_kept = std::min(std::max(res[i].n_kept, 0), it.n_tracked);
            o.n_new = std::min(std::max(res[i].n_new, 0), it.max_total);
            o.n_candidates = res[i].n_cand;
            std::memcpy(&o.max_response, &res[i].maxbits, sizeof(double));
        } else {
            o.status = VIO_ERR_NOT_FINITE;
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: a tracked point is not finite", i);
            ret = VIO_ERR_NOT_FINITE;
        }
        for (int k = 0; k < it.n_tracked; ++k) it.keep_order[k] = k < o.n_kept ? keep[d.trk + k] : -1;
        if (o.n_new > 0) std::memcpy(it.new_pts, newp + 2 * (size_t)d.newp, sizeof(float) * 2 * (size_t)o.n_new);
    }
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
    std::memset(&d, 0, sizeof(d));
    d.active = 1;
    set_geometry(d, width, height);
    const size_t px = (size_t)width * (size_t)height;
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_res = align256(sizeof(DetRes));
    if ((st = h->tab.ensure(h->err, sizeof(DetItemD))) != VIO_OK || (st = h->img.ensure(h->err, px)) != VIO_OK ||
        (st = h->out.ensure(h->err, b_res + sizeof(double) * px)) != VIO_OK || (st = h->r.ensure(h->err, sizeof(double) * px)) != VIO_OK)
        return st;
    d.img = h->img.d;
    std::memcpy(h->tab.h, &d, sizeof(d));
    copy_rows(h->img.h, img, width, height, stride);
    DetArgs a;
    std::memset(&a, 0, sizeof(a));
    a.items = (const DetItemD *)h->tab.d;
    a.r = h->r.d;
    a.res = (DetRes *)h->out.d;                          // (n_kept = 0 and no mask: every pixel is allowed, nothing else is read)
    a.quality = h->cfg.quality; a.d2 = det_d2(h->cfg.min_distance); a.count = 1;
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
