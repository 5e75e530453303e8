// vio_clahe.hip — libvio_clahe_hip.so: CLAHE equalisation of many 8-bit images in one call (include/vio_clahe.h).
//
//   k_clahe_lut      one 256-thread workgroup per (tile, image).  The tile's histogram in LDS with integer atomicAdd, one private copy
//                    per wavefront (a flat tile puts every pixel in one bin), the source read through the reflection where the image
//                    was extended.  Then thread b owns bin b: the merged count, the clip, the tile's excess by a butterfly across the
//                    wave and one LDS slot per wave, the closed form of the redistribution, an inclusive scan (wave scan plus the
//                    waves' offsets), and the LUT byte to global memory.
//   k_clahe_apply    a TX x TY block of pixels per workgroup, every image of the call in the grid (blockIdx.z).  Four pixels per
//                    thread and pass, one 4-byte load and one 4-byte store (the device copies have a pitch that is a multiple of 4, so
//                    every row is aligned); the four look-ups per pixel are byte gathers indexed by the pixel's value, out of
//                    LDS: the LUTs of the tiles the block of pixels can touch (a contiguous range in x and in y, known from the
//                    block's corners since the tile index is monotone in the position) are copied there first.  Gathering from
//                    global memory instead was measured and is slower.
// No floating-point atomics, no spin-waits, nothing between workgroups.  Contraction is off as in vio_flow.hip and vio_detect.hip: here
// it matters, a fused multiply-add in the blend changes output bytes (vio_clahe_math.h).
// The kernels themselves are in vio_clahe_body.inc, which libvio_frame_hip compiles too; the host side is here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vio_clahe.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_clahe_math.h"

#include "vio_clahe_body.inc"

constexpr int MAX_ITEMS = 4096;

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_clahe {
    int device = 0;
    ErrText err = {0};
    vio_clahe_config cfg = {VIO_CLAHE_DEFAULT_CLIP_LIMIT, VIO_CLAHE_DEFAULT_TILES, VIO_CLAHE_DEFAULT_TILES};
    Twin<char> tab;                                      // item descriptors
    Twin<uint8_t> img;                                   // the sources, rows at the device pitch
    Twin<uint8_t> out;                                   // the LUTs of every item | the results, laid out as the sources
    StreamEvents<4> q;                                   // events: upload, k_clahe_lut, k_clahe_apply start; end
    double timing[4] = {NAN, NAN, NAN, NAN};
};

namespace {

vio_status fail_synced(vio_clahe *h, const char *msg) { (void)hipStreamSynchronize(h->q.stream); return fail(h->err, VIO_ERR_HIP, "%s", msg); }

size_t last_byte(const vio_clahe_item &it, int stride) { return (size_t)(it.height - 1) * (size_t)stride + (size_t)it.width; }

}  // namespace

extern "C" {

int32_t vio_clahe_version(void) { return VIO_CLAHE_VERSION; }

const char *vio_clahe_last_error(const vio_clahe *h) { return h ? h->err : "NULL handle"; }

vio_status vio_clahe_create(int32_t device, void *stream, vio_clahe **out) {
    if (!out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VIO_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return VIO_ERR_BAD_ARG;
    DeviceScope dev(device);
    if (!dev.ok) return VIO_ERR_HIP;
    vio_clahe *h = new (std::nothrow) vio_clahe();
    if (!h) return VIO_ERR_BAD_ARG;
    h->device = device;
    if (h->q.open_stream(stream) != hipSuccess) { delete h; return VIO_ERR_HIP; }
    if (h->q.create_events() != hipSuccess) { vio_clahe_destroy(h); return VIO_ERR_HIP; }
    // (16 x 16 tiles stage 64 KB; a launch that asks for more than the kernel may have fails and is reported)
    (void)hipFuncSetAttribute((const void *)k_clahe_apply, hipFuncAttributeMaxDynamicSharedMemorySize,
                              VIO_CLAHE_MAX_TILES * VIO_CLAHE_MAX_TILES * BINS);
    (void)hipGetLastError();
    *out = h;
    return VIO_OK;
}

void vio_clahe_destroy(vio_clahe *h) {
    if (!h) return;
    DeviceScope dev(h->device);
    h->q.release();
    delete h;                                            // (the buffers free themselves)
}

vio_status vio_clahe_set_config(vio_clahe *h, const vio_clahe_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg || !std::isfinite(cfg->clip_limit) || cfg->clip_limit < 0.0 || cfg->tiles_x < 1 || cfg->tiles_x > VIO_CLAHE_MAX_TILES ||
        cfg->tiles_y < 1 || cfg->tiles_y > VIO_CLAHE_MAX_TILES)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_clahe_set_config: clip_limit finite and >= 0, tiles_x and tiles_y in [1, %d]", VIO_CLAHE_MAX_TILES);
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_clahe_timing(const vio_clahe *h, double *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_clahe_apply_batch(vio_clahe *h, int32_t count, const vio_clahe_item *items, vio_clahe_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_clahe_apply_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    // every argument of every item first: nothing is written or launched on an error
    const int tiles_x = h->cfg.tiles_x, tiles_y = h->cfg.tiles_y, tiles = tiles_x * tiles_y;
    std::vector<ClaheItemD> its((size_t)count);
    std::vector<int64_t> at((size_t)count, 0);           // an item's byte offset in the input buffer and, past the LUTs, in the output buffer
    int64_t b_img = 0;
    int max_ptiles = 0;
    bool want_luts = false;
    for (int i = 0; i < count; ++i) {
        const vio_clahe_item &it = items[i];
        if (it.width < 1 || it.height < 1 || it.width > VIO_CLAHE_MAX_DIM || it.height > VIO_CLAHE_MAX_DIM || it.src_stride < it.width ||
            it.dst_stride < it.width)
            return fail(h->err, VIO_ERR_BAD_ARG, "item %d: width and height must be in [1, %d] and both strides >= width", i, VIO_CLAHE_MAX_DIM);
        if (!it.src || !it.dst) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: src and dst are required", i);
        const uintptr_t s0 = (uintptr_t)it.src, s1 = s0 + last_byte(it, it.src_stride), d0 = (uintptr_t)it.dst, d1 = d0 + last_byte(it, it.dst_stride);
        if (s0 < d1 && d0 < s1) return fail(h->err, VIO_ERR_BAD_ARG, "item %d: dst overlaps src", i);
        const ClaheGeom g = clahe_geometry(it.width, it.height, tiles_x, tiles_y, h->cfg.clip_limit);
        ClaheItemD &d = its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        d.w = it.width; d.h = it.height;
        d.pitch = (it.width + PX - 1) / PX * PX;
        d.ext = g.ext; d.tile_w = g.tile_w; d.tile_h = g.tile_h; d.area = g.area; d.clip = g.clip;
        d.ptiles_x = (it.width + TX - 1) / TX;
        d.ptiles = d.ptiles_x * ((it.height + TY - 1) / TY);
        d.lut_scale = g.lut_scale; d.inv_tile_w = g.inv_tile_w; d.inv_tile_h = g.inv_tile_h;
        at[(size_t)i] = b_img;
        b_img += (int64_t)align256((size_t)d.pitch * (size_t)d.h);
        max_ptiles = std::max(max_ptiles, d.ptiles);
        want_luts = want_luts || it.luts != nullptr;
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_tab = sizeof(ClaheItemD) * (size_t)count, b_lut = align256((size_t)count * (size_t)tiles * BINS);
    vio_status st;
    if ((st = h->tab.ensure(h->err, b_tab)) != VIO_OK || (st = h->img.ensure(h->err, (size_t)b_img)) != VIO_OK ||
        (st = h->out.ensure(h->err, b_lut + (size_t)b_img)) != VIO_OK)
        return st;
    for (int i = 0; i < count; ++i) {                    // (the buffers are where they stay now)
        its[(size_t)i].src = h->img.d + at[(size_t)i];
        its[(size_t)i].dst = h->out.d + b_lut + at[(size_t)i];
    }
    std::memcpy(h->tab.h, its.data(), b_tab);
    for (int i = 0; i < count; ++i) {
        const vio_clahe_item &it = items[i];
        const ClaheItemD &d = its[(size_t)i];
        for (int y = 0; y < d.h; ++y) {
            uint8_t *row = h->img.h + at[(size_t)i] + (size_t)y * (size_t)d.pitch;
            std::memcpy(row, it.src + (size_t)y * (size_t)it.src_stride, (size_t)d.w);
            std::memset(row + d.w, 0, (size_t)(d.pitch - d.w));
        }
    }
    ClaheArgs a;
    a.items = (const ClaheItemD *)h->tab.d;
    a.luts = h->out.d;
    a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.count = count;
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess ||
        hipMemcpyAsync(h->img.d, h->img.h, (size_t)b_img, hipMemcpyHostToDevice, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    hipLaunchKernelGGL(k_clahe_lut, dim3((unsigned)tiles, 1, (unsigned)count), dim3(NT), 0, q, a);
    (void)hipEventRecord(h->q.ev[2], q);
    hipLaunchKernelGGL(k_clahe_apply, dim3((unsigned)max_ptiles, 1, (unsigned)count), dim3(NT), (size_t)tiles * BINS, q, a);
    (void)hipEventRecord(h->q.ev[3], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    const size_t from = want_luts ? 0 : b_lut;
    if (hipMemcpyAsync(h->out.h + from, h->out.d + from, b_lut + (size_t)b_img - from, hipMemcpyDeviceToHost, q) != hipSuccess ||
        hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    for (int i = 0; i < count; ++i) {
        const vio_clahe_item &it = items[i];
        const ClaheItemD &d = its[(size_t)i];
        vio_clahe_result &o = results[i];
        o.status = VIO_OK; o.clip = d.clip; o.tile_w = d.tile_w; o.tile_h = d.tile_h;
        for (int y = 0; y < d.h; ++y)
            std::memcpy(it.dst + (size_t)y * (size_t)it.dst_stride, h->out.h + b_lut + at[(size_t)i] + (size_t)y * (size_t)d.pitch, (size_t)d.w);
        if (it.luts) std::memcpy(it.luts, h->out.h + (size_t)i * (size_t)tiles * BINS, (size_t)tiles * BINS);
    }
    const auto t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    h->timing[2] = elapsed_ms(h->q.ev[2], h->q.ev[3]);
    h->timing[3] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return VIO_OK;
}

}  // extern "C"
