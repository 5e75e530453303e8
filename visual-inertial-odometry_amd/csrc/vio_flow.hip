// vio_flow.hip — libvio_flow_hip.so: pyramidal Lucas-Kanade tracking of the keypoints of many image pairs in one call
// (include/vio_flow.h).
//
//   k_flow_pyr_down   one launch per level, every image of the call in the grid (blockIdx.y), one thread per output pixel: the 5 x 5
//                     [1 4 6 4 1] x [1 4 6 4 1] sum of the level below with BORDER_REFLECT_101, (sum + 128) >> 8.  Integers only.
//   k_flow_track      one wavefront per keypoint, WAVES wavefronts per workgroup; the keypoints of every item of the call are one
//                     flat grid through the host-made descriptor table.  The levels L - 1 .. 0 run inside the kernel with the state
//                     in registers.  Patch pixel m belongs to lane m mod 64 (at most PPL pixels per lane); the template's values
//                     (inverse mode: its gradients and H too) are formed once per level and stay in registers.  Each iteration every
//                     lane adds its pixels' terms in ascending order into six accumulators, the butterfly v[i] += v[i ^ s],
//                     s = 1 .. 32, leaves the same six sums in every lane, and every lane runs the 2 x 2 solve and the decision.
//                     The Scharr gradients are formed on the fly from the 4 x 4 pixels around a sample.
// Keypoints of one workgroup end after different iteration counts, so k_flow_track has no workgroup barrier: shuffles only.  Every
// lane of a wavefront holds the same loop state, so the trip counts are uniform within the wavefront.
// Contraction is off: products and sums round as the host restatement's (tests/flow_reference.py) do.  No floating-point atomics.
// The kernels themselves are in vio_flow_body.inc, which libvio_frame_hip compiles too; the host side is here.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vio_flow.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_flow_math.h"

#include "vio_flow_body.inc"

constexpr int MAX_ITEMS = 16384;

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_flow {
    int device = 0;
    ErrText err = {0};
    vio_flow_config cfg = {VIO_FLOW_DEFAULT_LEVELS, VIO_FLOW_DEFAULT_HALF_PATCH, VIO_FLOW_DEFAULT_MAX_ITER, 0, VIO_FLOW_DEFAULT_BORDER, 0};
    Twin<char> tab;                                      // item descriptors | keypoint descriptors
    Twin<uint8_t> pyr;                                   // level 0 of every image (the part uploaded) | the levels above
    Twin<FlowOut> out;
    StreamEvents<4> q;                                   // events: upload start, pyramid start, tracking start, end
    double timing[4] = {NAN, NAN, NAN, NAN};
};

namespace {

vio_status fail_synced(vio_flow *h, const char *msg) { (void)hipStreamSynchronize(h->q.stream); return fail(h->err, VIO_ERR_HIP, "%s", msg); }

// the sizes of the levels of a width x height image; false if one is smaller than 2 x 2
bool level_dims(int width, int height, int levels, int32_t *w, int32_t *hh) {
    for (int l = 0; l < levels; ++l) {
        w[l] = l ? w[l - 1] / 2 : width;
        hh[l] = l ? hh[l - 1] / 2 : height;
        if (w[l] < 2 || hh[l] < 2) return false;
    }
    return true;
}

vio_status check_image(vio_flow *h, int i, int width, int height, int stride) {
    if (width < 1 || height < 1 || width > VIO_FLOW_MAX_DIM || height > VIO_FLOW_MAX_DIM || stride < width)
        return fail(h->err, VIO_ERR_BAD_ARG, "item %d: width and height must be in [1, %d] and stride >= width", i, VIO_FLOW_MAX_DIM);
    int32_t w[MAXL], hh[MAXL];
    if (!level_dims(width, height, h->cfg.levels, w, hh))
        return fail(h->err, VIO_ERR_BAD_ARG, "item %d: a %d x %d image has a level below 2 x 2 among its %d", i, width, height, h->cfg.levels);
    return VIO_OK;
}

void copy_rows(uint8_t *dst, const uint8_t *src, int width, int height, int stride) {
    for (int y = 0; y < height; ++y) std::memcpy(dst + (size_t)y * (size_t)width, src + (size_t)y * (size_t)stride, (size_t)width);
}

// one k_flow_pyr_down launch per level above 0; max_px[l]: the largest level-l image of the call
void launch_pyramids(vio_flow *h, const FlowItemD *items_d, int nimg, const int64_t *max_px) {
    for (int l = 0; l + 1 < h->cfg.levels; ++l) {
        PyrArgs pa;
        pa.items = items_d; pa.level = l; pa.nimg = nimg; pa.both = 1; pa.pad = 0;
        hipLaunchKernelGGL(k_flow_pyr_down, dim3((unsigned)((max_px[l + 1] + NT - 1) / NT), (unsigned)nimg), dim3(NT), 0, h->q.stream, pa);
    }
}

}  // namespace

extern "C" {

int32_t vio_flow_version(void) { return VIO_FLOW_VERSION; }

const char *vio_flow_last_error(const vio_flow *h) { return h ? h->err : "NULL handle"; }

vio_status vio_flow_create(int32_t device, void *stream, vio_flow **out) {
    if (!out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VIO_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return VIO_ERR_BAD_ARG;
    DeviceScope dev(device);
    if (!dev.ok) return VIO_ERR_HIP;
    vio_flow *h = new (std::nothrow) vio_flow();
    if (!h) return VIO_ERR_BAD_ARG;
    h->device = device;
    if (h->q.open_stream(stream) != hipSuccess) { delete h; return VIO_ERR_HIP; }
    if (h->q.create_events() != hipSuccess) { vio_flow_destroy(h); return VIO_ERR_HIP; }
    *out = h;
    return VIO_OK;
}

void vio_flow_destroy(vio_flow *h) {
    if (!h) return;
    DeviceScope dev(h->device);
    h->q.release();
    delete h;                                            // (the buffers free themselves)
}

vio_status vio_flow_set_config(vio_flow *h, const vio_flow_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg || cfg->levels < 1 || cfg->levels > VIO_FLOW_MAX_LEVELS || cfg->half_patch < 1 || cfg->half_patch > VIO_FLOW_MAX_HALF_PATCH ||
        cfg->max_iter < 1 || cfg->max_iter > 1000 || (cfg->inverse != 0 && cfg->inverse != 1) || cfg->border < 0 ||
        (cfg->early_stop != 0 && cfg->early_stop != 1))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_flow_set_config: levels in [1, %d], half_patch in [1, %d], max_iter in [1, 1000], "
                    "inverse and early_stop 0 or 1, border >= 0", VIO_FLOW_MAX_LEVELS, VIO_FLOW_MAX_HALF_PATCH);
    h->cfg = *cfg;
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
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !next_pts)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_flow_track_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
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
        d.active = 1;
        level_dims(items[i].width, items[i].height, L, d.w, d.h);
        for (int l = 0; l < L; ++l) d.pitch[l] = d.w[l];        // (rows tightly packed)
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
        (st = h->out.ensure(h->err, sizeof(FlowOut) * total)) != VIO_OK)
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
        copy_rows(h->pyr.h + at[(size_t)i * 2 * MAXL], it.img_prev, it.width, it.height, it.stride);
        copy_rows(h->pyr.h + at[(size_t)i * 2 * MAXL + MAXL], it.img_next, it.width, it.height, it.stride);
        for (int k = 0; k < it.n_pts; ++k) {
            FlowPt &p = hp[row + (size_t)k];
            p.item = i; p.has_guess = it.guess != nullptr;
            p.px = it.prev_pts[2 * k]; p.py = it.prev_pts[2 * k + 1];
            p.gx = it.guess ? it.guess[2 * k] : 0.f; p.gy = it.guess ? it.guess[2 * k + 1] : 0.f;
        }
        row += (size_t)it.n_pts;
    }
    FlowArgs a;
    a.items = (const FlowItemD *)h->tab.d;
    a.pts = (const FlowPt *)(h->tab.d + b_it);
    a.out = h->out.d;
    a.npts = (int32_t)total; a.levels = L; a.half_patch = h->cfg.half_patch; a.max_iter = h->cfg.max_iter;
    a.border = h->cfg.border; a.early_stop = h->cfg.early_stop;
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess ||
        hipMemcpyAsync(h->pyr.d, h->pyr.h, b_l0, hipMemcpyHostToDevice, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    launch_pyramids(h, a.items, 2 * count, max_px);
    (void)hipEventRecord(h->q.ev[2], q);
    const dim3 grid((unsigned)((total + WAVES - 1) / WAVES));
    if (h->cfg.inverse) hipLaunchKernelGGL(k_flow_track<true>, grid, dim3(NT), 0, q, a);
    else hipLaunchKernelGGL(k_flow_track<false>, grid, dim3(NT), 0, q, a);
    (void)hipEventRecord(h->q.ev[3], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    const size_t outb = sizeof(FlowOut) * total;
    if (hipMemcpyAsync(h->out.h, h->out.d, outb, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    vio_status ret = VIO_OK;
    row = 0;
    for (int i = 0; i < count; ++i) {
        for (int k = 0; k < items[i].n_pts; ++k) {
            const FlowOut &o = h->out.h[row + (size_t)k];
            next_pts[2 * (row + k)] = o.x; next_pts[2 * (row + k) + 1] = o.y;
            if (info) {
                vio_flow_pt_info &fi = info[row + k];
                fi.status = o.status; fi.iterations = o.iterations; fi.cost = o.cost;
            }
            if (o.status == VIO_ERR_NOT_FINITE) {
                if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: keypoint %d or its guess is not finite", i, k);
                ret = VIO_ERR_NOT_FINITE;
            }
        }
        row += (size_t)items[i].n_pts;
    }
    const auto t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    h->timing[2] = elapsed_ms(h->q.ev[2], h->q.ev[3]);
    h->timing[3] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return ret;
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
    d.active = 1;
    level_dims(width, height, L, d.w, d.h);
    int64_t off = 0, max_px[MAXL] = {0};
    int64_t at[MAXL] = {0};
    for (int l = 0; l < L; ++l) {
        at[l] = off; d.pitch[l] = d.w[l];
        max_px[l] = (int64_t)d.w[l] * d.h[l];
        off += max_px[l];
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    if ((st = h->tab.ensure(h->err, sizeof(FlowItemD))) != VIO_OK || (st = h->pyr.ensure(h->err, (size_t)off)) != VIO_OK) return st;
    for (int l = 0; l < L; ++l) d.prev[l] = d.next[l] = h->pyr.d + at[l];
    std::memcpy(h->tab.h, &d, sizeof(d));
    copy_rows(h->pyr.h, img, width, height, stride);
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->tab.d, h->tab.h, sizeof(FlowItemD), hipMemcpyHostToDevice, q) != hipSuccess ||
        hipMemcpyAsync(h->pyr.d, h->pyr.h, (size_t)max_px[0], hipMemcpyHostToDevice, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    launch_pyramids(h, (const FlowItemD *)h->tab.d, 1, max_px);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    const size_t rest = (size_t)(off - max_px[0]);
    if ((rest && hipMemcpyAsync(h->pyr.h + max_px[0], h->pyr.d + max_px[0], rest, hipMemcpyDeviceToHost, q) != hipSuccess) ||
        hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    std::memcpy(out, h->pyr.h, (size_t)off);
    return VIO_OK;
}

}  // extern "C"
