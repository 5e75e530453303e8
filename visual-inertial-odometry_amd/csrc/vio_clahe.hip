// vio_clahe.hip — libvio_clahe_hip.so: CLAHE equalisation of many 8-bit images in one call (include/vio_clahe.h).
// No floating-point atomics, no spin-waits, nothing between workgroups.  Contraction is off as in vio_flow.hip and vio_detect.hip: here
// it matters, a fused multiply-add in the blend changes output bytes (vio_clahe_math.h).
// The kernels, described where they are, are in vio_clahe_body.inc, which libvio_frame_hip compiles too; what the
// host side shares with that library is in vio_clahe_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_clahe.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_clahe_math.h"

#include "vio_clahe_host.h"
#include "vio_clahe_body.inc"

constexpr int MAX_ITEMS = 4096;

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_clahe {
    int device = 0;
    ErrText err = {0};
    vio_clahe_config cfg = CLAHE_DEFAULTS;
    Twin<char> tab;                                      // item descriptors
    Twin<uint8_t> img;                                   // the sources, rows at the device pitch
    Twin<uint8_t> out;                                   // the LUTs of every item | the results, laid out as the sources
    StreamEvents<4> q;                                   // events: upload, k_clahe_lut, k_clahe_apply start; end
    double timing[4] = {NAN, NAN, NAN, NAN};
};

namespace {

size_t last_byte(const vio_clahe_item &it, int stride) { return (size_t)(it.height - 1) * (size_t)stride + (size_t)it.width; }

}  // namespace

extern "C" {

int32_t vio_clahe_version(void) { return VIO_CLAHE_VERSION; }

const char *vio_clahe_last_error(const vio_clahe *h) { return h ? h->err : "NULL handle"; }

vio_status vio_clahe_create(int32_t device, void *stream, vio_clahe **out) {
    return create_handle(device, stream, out, vio_clahe_destroy, [](vio_clahe *) { clahe_allow_lds(); return true; });
}

void vio_clahe_destroy(vio_clahe *h) { destroy_handle(h); }

vio_status vio_clahe_set_config(vio_clahe *h, const vio_clahe_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = clahe_check_config(h->err, "vio_clahe_set_config", cfg);
    if (st != VIO_OK) return st;
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
    const int tiles = h->cfg.tiles_x * h->cfg.tiles_y;
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
        ClaheItemD &d = its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        clahe_item(d, it.width, it.height, clahe_pitch(it.width), h->cfg);
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
    for (int i = 0; i < count; ++i)
        pack_rows(h->img.h + at[(size_t)i], its[(size_t)i].pitch, items[i].src, items[i].width, items[i].height, items[i].src_stride);
    const ClaheArgs a = clahe_args((const ClaheItemD *)h->tab.d, h->out.d, h->cfg, count);
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->tab.d, h->tab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess ||
        hipMemcpyAsync(h->img.d, h->img.h, (size_t)b_img, hipMemcpyHostToDevice, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    clahe_launch(q, a, max_ptiles, h->q.ev[2]);
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
        copy_rows(it.dst, it.dst_stride, h->out.h + b_lut + at[(size_t)i], d.pitch, d.w, d.h);
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
