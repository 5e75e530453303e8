// vio_frame.hip — libvio_frame_hip.so: frames that stay on the device across CLAHE, tracking and detection (include/vio_frame.h,
// DESIGN.md section 23).
//
// The numeric kernels are those of libvio_clahe_hip, libvio_flow_hip, libvio_detect_hip and libvio_reject_hip, compiled from the same
// four files (vio_clahe_body.inc, vio_flow_body.inc, vio_detect_body.inc, vio_reject_body.inc), each inside a namespace since their
// constants share names.  The five kernels that join them in vio_frame_read_batch are in vio_front_body.inc.
// What is here is the host side: the slot table and the block pool (vio_frame_slots.h, plain C++), the descriptor
// tables that point the kernels at resident frames, and the copies.  A frame is written by one upload (or by k_clahe_apply out of the
// upload buffer) and the pyramid kernel, and read in place ever after: there is no repacking pass.
// Contraction is off for all of it, as in the three libraries; in CLAHE it decides bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vio_frame.h"
#include "vio_companion.h"
#include "vio_frame_slots.h"

#pragma clang fp contract(off)

#include "vio_clahe_math.h"
#include "vio_detect_math.h"
#include "vio_flow_math.h"
#include "vio_front_math.h"
#include "vio_reject_math.h"
#include "vio_sfm_math.h"

namespace kc {
#include "vio_clahe_body.inc"
}
namespace kf {
#include "vio_flow_body.inc"
}
namespace kd {
#include "vio_detect_body.inc"
}
namespace kr {
#include "vio_reject_body.inc"
}
#include "vio_front_body.inc"

static_assert(FRAME_MAX_SLOTS == VIO_FRAME_MAX_SLOTS && FRAME_MAX_LEVELS == VIO_FLOW_MAX_LEVELS && FRAME_MAX_DIM == VIO_FRAME_MAX_DIM,
              "vio_frame_slots.h restates the header's limits");
static_assert(FRAME_MAX_TRACK_POINTS == VIO_FRAME_MAX_TRACK_POINTS && FRONT_CAP == VIO_FRAME_MAX_TRACK_POINTS, "one capacity");
static_assert(VIO_FRAME_MAX_TRACK_POINTS <= VIO_DETECT_MAX_POINTS && VIO_FRAME_MAX_TRACK_POINTS <= VIO_REJECT_MAX_POINTS &&
              VIO_FRAME_MAX_TRACK_POINTS <= VIO_FLOW_MAX_POINTS, "a slot's table fits every library's limits");
static_assert(VIO_FRAME_MAX_DIM == VIO_FLOW_MAX_DIM && VIO_FRAME_MAX_DIM == VIO_DETECT_MAX_DIM && VIO_FRAME_MAX_DIM == VIO_CLAHE_MAX_DIM,
              "one size limit");

struct vio_frame {
    int device = 0;
    ErrText err = {0};
    int32_t equalize = 0;
    vio_clahe_config ccfg = {VIO_CLAHE_DEFAULT_CLIP_LIMIT, VIO_CLAHE_DEFAULT_TILES, VIO_CLAHE_DEFAULT_TILES};
    vio_flow_config fcfg = {VIO_FLOW_DEFAULT_LEVELS, VIO_FLOW_DEFAULT_HALF_PATCH, VIO_FLOW_DEFAULT_MAX_ITER, 0, VIO_FLOW_DEFAULT_BORDER, 0};
    vio_detect_config dcfg = {VIO_DETECT_DEFAULT_QUALITY, VIO_DETECT_DEFAULT_MIN_DISTANCE, 0};
    FrameTable tab;
    // uploads: the pinned staging of the raw images (and of a mask) with its device twin, the upload buffer the CLAHE kernels read; the
    // descriptor tables of a push.  `staged` is recorded behind the copies that read the pinned halves, and waited for before they are
    // written again.
    Twin<uint8_t> raw;
    Twin<char> ptab;                                     // push: ClaheItemD per item | FlowItemD per item
    DevBuf<uint8_t> luts;
    hipEvent_t staged = nullptr;
    bool staged_pending = false;
    // track and detect wait for their results, so their buffers are free again when they return
    Twin<char> ttab;                                     // track: FlowItemD per item | FlowPt per keypoint
    Twin<kf::FlowOut> tout;
    Twin<char> dtab;                                     // detect: DetItemD per item | DetTrk per tracked point
    Twin<char> dout;                                     // DetRes per item | keep_order | new_pts
    DevBuf<double> r;
    DevBuf<uint32_t> cand;
    DevBuf<char> scratch;                                // tkey | kept_xy
    StreamEvents<8> q;                                   // push: 0 .. 3; track: 4, 5; detect: 6, 7
    uint64_t counters[4] = {0, 0, 0, 0};
    double timing[8] = {NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN};
    bool push_timed = true;                              // false: the last push's events have not been read yet
    // vio_frame_read_batch: the camera and the settings of the join; the point tables of every slot (allocated and zeroed at the first
    // use, SLOT_BYTES each); its descriptor tables, its device work space and its results.  It waits, so they are free when it returns.
    vio_reject_config rcfg = {0u, VIO_REJECT_DEFAULT_HYPOTHESES, VIO_REJECT_DEFAULT_F_THRESHOLD, VIO_REJECT_DEFAULT_FOCAL_LENGTH};
    vio_reject_camera camera = {};
    RejCam cam = {};
    bool have_camera = false;
    int32_t max_cnt = VIO_FRAME_DEFAULT_MAX_CNT, border = VIO_FRAME_DEFAULT_BORDER;
    DevBuf<char> ptsd;
    Twin<char> rtab;                                     // FrontItem | FlowItemD | DetItemD | RejPair | LiftItem, per item each
    DevBuf<char> rwork;
    Twin<char> rout;                                     // FrontRes per item | the result rows
    hipEvent_t rev[5] = {};                              // behind the filter, the reject, the detection, the finish, the read-back
    double rtiming[8] = {NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN};
};

namespace {

constexpr int MAX_ITEMS = VIO_FRAME_MAX_SLOTS;

vio_status fail_synced(vio_frame *h, const char *msg) { (void)hipStreamSynchronize(h->q.stream); return fail(h->err, VIO_ERR_HIP, "%s", msg); }

void *device_block(int64_t bytes) {
    void *p = nullptr;
    return hipMalloc(&p, (size_t)bytes) == hipSuccess ? p : nullptr;
}

vio_status fail_check(vio_frame *h, const char *fn, FrameCheck c, int item, int slot) {
    switch (c) {
    case FRAME_BAD_SLOT: return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d is outside [0, %d)", fn, item, slot, VIO_FRAME_MAX_SLOTS);
    case FRAME_TWICE: return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d is listed twice", fn, item, slot);
    case FRAME_BAD_DIMS: return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: width and height must be in [1, %d], which 0 or 1, level in [0, %d)",
                                     fn, item, VIO_FRAME_MAX_DIM, h->tab.levels);
    case FRAME_SMALL_LEVEL: return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: the image has a level below 2 x 2 among its %d", fn, item, h->tab.levels);
    case FRAME_GEOMETRY: return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d holds %d x %d frames; vio_frame_reset it first", fn, item,
                                     slot, h->tab.slots[slot].width, h->tab.slots[slot].height);
    case FRAME_TOO_FEW: return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d holds %d frame(s), too few", fn, item, slot,
                                    h->tab.slots[slot].n_frames);
    case FRAME_BAD_TIME: return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: the time must be finite and, while slot %d holds the frame before's normalised points, after its %.17g",
                                     fn, item, slot, h->tab.slots[slot].time);
    case FRAME_BAD_POINTS: return fail(h->err, VIO_ERR_BAD_ARG, "%s: slot %d: n must be in [0, %d]", fn, slot, VIO_FRAME_MAX_TRACK_POINTS);
    case FRAME_MASK_GEOMETRY: return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d's mask is %d x %d, its frames are %d x %d", fn, item, slot,
                                          h->tab.slots[slot].mask_w, h->tab.slots[slot].mask_h, h->tab.slots[slot].width, h->tab.slots[slot].height);
    default: return VIO_OK;
    }
}

// the pinned staging may be written again once the copies that read it have finished
void wait_staged(vio_frame *h) {
    if (h->staged_pending) (void)hipEventSynchronize(h->staged);
    h->staged_pending = false;
}

void mark_staged(vio_frame *h) {
    h->staged_pending = hipEventRecord(h->staged, h->q.stream) == hipSuccess;
    if (!h->staged_pending) (void)hipStreamSynchronize(h->q.stream);
}

// rows at `pitch`, the padding zero
void pack_rows(uint8_t *dst, int pitch, const uint8_t *src, int width, int height, int stride) {
    for (int y = 0; y < height; ++y) {
        uint8_t *row = dst + (size_t)y * (size_t)pitch;
        std::memcpy(row, src + (size_t)y * (size_t)stride, (size_t)width);
        std::memset(row + width, 0, (size_t)(pitch - width));
    }
}

void read_push_timing(vio_frame *h) {
    if (h->push_timed) return;
    (void)hipEventSynchronize(h->q.ev[3]);
    for (int k = 0; k < 3; ++k) h->timing[1 + k] = elapsed_ms(h->q.ev[k], h->q.ev[k + 1]);
    h->push_timed = true;
}

// what a push and a read ask of an item's image besides the slot table's checks
vio_status check_images(vio_frame *h, const char *fn, int32_t count, const vio_frame_push_item *items) {
    for (int i = 0; i < count; ++i) {
        if (items[i].stride < items[i].width) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: stride < width", fn, i);
        if (!items[i].img) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: img is required", fn, i);
    }
    return VIO_OK;
}

// The push of `count` checked items, which vio_frame_push_batch and vio_frame_read_batch share: the roll, the uploads, the CLAHE and
// the pyramid kernels, enqueued; it does not wait for them.
vio_status push_run(vio_frame *h, int32_t count, const vio_frame_push_item *items, std::chrono::steady_clock::time_point t0) {
    const int L = h->tab.levels, tiles_x = h->ccfg.tiles_x, tiles_y = h->ccfg.tiles_y, tiles = tiles_x * tiles_y;
    std::vector<FrameLayout> lay((size_t)count);
    std::vector<int64_t> at((size_t)count);              // an item's offset in the staging and in the upload buffer
    int64_t b_raw = 0, max_px[FRAME_MAX_LEVELS] = {0};
    for (int i = 0; i < count; ++i) {
        frame_layout(items[i].width, items[i].height, L, lay[(size_t)i]);
        at[(size_t)i] = b_raw;
        b_raw += frame_align((int64_t)lay[(size_t)i].pitch[0] * items[i].height);
        for (int l = 0; l < L; ++l) max_px[l] = std::max(max_px[l], (int64_t)lay[(size_t)i].w[l] * lay[(size_t)i].h[l]);
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    read_push_timing(h);                                 // (the events are about to be recorded again)
    wait_staged(h);
    const size_t b_ci = align256(sizeof(kc::ClaheItemD) * (size_t)count), b_tab = b_ci + sizeof(kf::FlowItemD) * (size_t)count;
    vio_status st;
    if ((st = h->ptab.ensure(h->err, b_tab)) != VIO_OK || (st = h->raw.ensure(h->err, (size_t)b_raw)) != VIO_OK ||
        (h->equalize && (st = h->luts.ensure(h->err, (size_t)count * (size_t)tiles * kc::BINS)) != VIO_OK))
        return st;
    // the roll: from here on the slots name the new frames
    kc::ClaheItemD *ci = (kc::ClaheItemD *)h->ptab.h;
    kf::FlowItemD *fi = (kf::FlowItemD *)(h->ptab.h + b_ci);
    std::memset(h->ptab.h, 0, b_tab);
    int max_ptiles = 0;
    for (int i = 0; i < count; ++i) {
        const vio_frame_push_item &it = items[i];
        const FrameLayout &Y = lay[(size_t)i];
        const int blk = h->tab.push(it.slot, it.width, it.height, device_block);
        if (blk < 0) return fail(h->err, VIO_ERR_HIP, "item %d: no device memory for a frame of %lld bytes", i, (long long)Y.bytes);
        kf::FlowItemD &f = fi[i];
        f.active = 1;
        for (int l = 0; l < L; ++l) {
            f.w[l] = Y.w[l]; f.h[l] = Y.h[l]; f.pitch[l] = Y.pitch[l];
            f.next[l] = h->tab.level_ptr(blk, Y, l);
        }
        pack_rows(h->raw.h + at[(size_t)i], Y.pitch[0], it.img, it.width, it.height, it.stride);
        if (!h->equalize) continue;
        const ClaheGeom g = clahe_geometry(it.width, it.height, tiles_x, tiles_y, h->ccfg.clip_limit);
        kc::ClaheItemD &d = ci[i];
        d.w = it.width; d.h = it.height; d.pitch = Y.pitch[0];
        d.ext = g.ext; d.tile_w = g.tile_w; d.tile_h = g.tile_h; d.area = g.area; d.clip = g.clip;
        d.ptiles_x = (it.width + kc::TX - 1) / kc::TX;
        d.ptiles = d.ptiles_x * ((it.height + kc::TY - 1) / kc::TY);
        d.lut_scale = g.lut_scale; d.inv_tile_w = g.inv_tile_w; d.inv_tile_h = g.inv_tile_h;
        d.src = h->raw.d + at[(size_t)i];
        d.dst = f.next[0];
        max_ptiles = std::max(max_ptiles, d.ptiles);
    }
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    bool ok = hipMemcpyAsync(h->ptab.d, h->ptab.h, b_tab, hipMemcpyHostToDevice, q) == hipSuccess;
    if (h->equalize) {                                   // one copy into the upload buffer; k_clahe_apply writes the frames
        ok = ok && hipMemcpyAsync(h->raw.d, h->raw.h, (size_t)b_raw, hipMemcpyHostToDevice, q) == hipSuccess;
    } else {                                             // the image is level 0: one copy each, to where the frame lies
        for (int i = 0; ok && i < count; ++i)
            ok = hipMemcpyAsync(fi[i].next[0], h->raw.h + at[(size_t)i], (size_t)lay[(size_t)i].pitch[0] * (size_t)items[i].height,
                                hipMemcpyHostToDevice, q) == hipSuccess;
    }
    mark_staged(h);
    if (!ok) return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    if (h->equalize) {
        kc::ClaheArgs a;
        a.items = (const kc::ClaheItemD *)h->ptab.d;
        a.luts = h->luts.d;
        a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.count = count;
        hipLaunchKernelGGL(kc::k_clahe_lut, dim3((unsigned)tiles, 1, (unsigned)count), dim3(kc::NT), 0, q, a);
        hipLaunchKernelGGL(kc::k_clahe_apply, dim3((unsigned)max_ptiles, 1, (unsigned)count), dim3(kc::NT), (size_t)tiles * kc::BINS, q, a);
    }
    (void)hipEventRecord(h->q.ev[2], q);
    for (int l = 0; l + 1 < L; ++l) {
        kf::PyrArgs pa;
        pa.items = (const kf::FlowItemD *)(h->ptab.d + b_ci); pa.level = l; pa.nimg = count; pa.both = 0; pa.pad = 0;
        hipLaunchKernelGGL(kf::k_flow_pyr_down, dim3((unsigned)((max_px[l + 1] + kf::NT - 1) / kf::NT), (unsigned)count), dim3(kf::NT), 0, q, pa);
    }
    (void)hipEventRecord(h->q.ev[3], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    for (int i = 0; i < count; ++i) h->counters[0] += (uint64_t)items[i].width * (uint64_t)items[i].height;
    h->counters[2] += b_tab;
    h->push_timed = false;
    h->timing[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VIO_OK;
}


// A slot's point table on the device: cur_pts | ids | prev_un_ids | prev_un_pts | track_cnt | the next free id.
constexpr size_t CAP = VIO_FRAME_MAX_TRACK_POINTS;
constexpr size_t SLOT_BYTES = 36 * CAP + 256;

struct SlotPts {
    float *cur;
    long long *ids, *prev_ids;
    float *prev_pts;
    int32_t *cnt;
    long long *next_id;
};

SlotPts slot_pts(const vio_frame *h, int slot) {
    char *b = h->ptsd.d + (size_t)slot * SLOT_BYTES;
    SlotPts p;
    p.cur = (float *)b; p.ids = (long long *)(b + 8 * CAP); p.prev_ids = (long long *)(b + 16 * CAP);
    p.prev_pts = (float *)(b + 24 * CAP); p.cnt = (int32_t *)(b + 32 * CAP); p.next_id = (long long *)(b + 36 * CAP);
    return p;
}

// the tables of every slot, zeroed once (every id counter starts at 0)
vio_status ensure_points(vio_frame *h) {
    if (h->ptsd.d) return VIO_OK;
    const vio_status st = h->ptsd.ensure(h->err, SLOT_BYTES * (size_t)VIO_FRAME_MAX_SLOTS);
    if (st != VIO_OK) return st;
    if (hipMemsetAsync(h->ptsd.d, 0, SLOT_BYTES * (size_t)VIO_FRAME_MAX_SLOTS, h->q.stream) != hipSuccess) {
        h->ptsd.release();
        return fail(h->err, VIO_ERR_HIP, "hipMemsetAsync of the point tables");
    }
    return VIO_OK;
}

}  // namespace

extern "C" {

int32_t vio_frame_version(void) { return VIO_FRAME_VERSION; }

const char *vio_frame_last_error(const vio_frame *h) { return h ? h->err : "NULL handle"; }

vio_status vio_frame_create(int32_t device, void *stream, vio_frame **out) {
    if (!out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VIO_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return VIO_ERR_BAD_ARG;
    DeviceScope dev(device);
    if (!dev.ok) return VIO_ERR_HIP;
    vio_frame *h = new (std::nothrow) vio_frame();
    if (!h) return VIO_ERR_BAD_ARG;
    h->device = device;
    if (h->q.open_stream(stream) != hipSuccess) { delete h; return VIO_ERR_HIP; }
    if (h->q.create_events() != hipSuccess || hipEventCreate(&h->staged) != hipSuccess) { vio_frame_destroy(h); return VIO_ERR_HIP; }
    for (hipEvent_t &e : h->rev)
        if (hipEventCreate(&e) != hipSuccess) { e = nullptr; vio_frame_destroy(h); return VIO_ERR_HIP; }
    // (16 x 16 tiles stage 64 KB; a launch that asks for more than the kernel may have fails and is reported)
    (void)hipFuncSetAttribute((const void *)kc::k_clahe_apply, hipFuncAttributeMaxDynamicSharedMemorySize,
                              VIO_CLAHE_MAX_TILES * VIO_CLAHE_MAX_TILES * kc::BINS);
    (void)hipGetLastError();
    *out = h;
    return VIO_OK;
}

void vio_frame_destroy(vio_frame *h) {
    if (!h) return;
    DeviceScope dev(h->device);
    h->q.release();                                      // (waits for the stream: nothing reads a block any more)
    if (h->staged) (void)hipEventDestroy(h->staged);
    for (hipEvent_t e : h->rev)
        if (e) (void)hipEventDestroy(e);
    h->tab.pool.destroy([](void *p) { (void)hipFree(p); });
    delete h;                                            // (the other buffers free themselves)
}

vio_status vio_frame_set_config(vio_frame *h, int32_t equalize, const vio_clahe_config *clahe, const vio_flow_config *flow,
                                const vio_detect_config *detect) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_clahe_config c0 = {VIO_CLAHE_DEFAULT_CLIP_LIMIT, VIO_CLAHE_DEFAULT_TILES, VIO_CLAHE_DEFAULT_TILES};
    const vio_flow_config f0 = {VIO_FLOW_DEFAULT_LEVELS, VIO_FLOW_DEFAULT_HALF_PATCH, VIO_FLOW_DEFAULT_MAX_ITER, 0, VIO_FLOW_DEFAULT_BORDER, 0};
    const vio_detect_config d0 = {VIO_DETECT_DEFAULT_QUALITY, VIO_DETECT_DEFAULT_MIN_DISTANCE, 0};
    const vio_clahe_config c = clahe ? *clahe : c0;
    const vio_flow_config f = flow ? *flow : f0;
    vio_detect_config d = detect ? *detect : d0;
    if (equalize != 0 && equalize != 1) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_config: equalize 0 or 1");
    if (!std::isfinite(c.clip_limit) || c.clip_limit < 0.0 || c.tiles_x < 1 || c.tiles_x > VIO_CLAHE_MAX_TILES || c.tiles_y < 1 ||
        c.tiles_y > VIO_CLAHE_MAX_TILES)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_config: clip_limit finite and >= 0, tiles_x and tiles_y in [1, %d]", VIO_CLAHE_MAX_TILES);
    if (f.levels < 1 || f.levels > VIO_FLOW_MAX_LEVELS || f.half_patch < 1 || f.half_patch > VIO_FLOW_MAX_HALF_PATCH || f.max_iter < 1 ||
        f.max_iter > 1000 || (f.inverse != 0 && f.inverse != 1) || f.border < 0 || (f.early_stop != 0 && f.early_stop != 1))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_config: levels in [1, %d], half_patch in [1, %d], max_iter in [1, 1000], "
                    "inverse and early_stop 0 or 1, border >= 0", VIO_FLOW_MAX_LEVELS, VIO_FLOW_MAX_HALF_PATCH);
    if (!(d.quality > 0.0 && d.quality <= 1.0) || d.min_distance < 0)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_config: quality in (0, 1], min_distance >= 0");
    d.reserved = 0;
    h->equalize = equalize; h->ccfg = c; h->fcfg = f; h->dcfg = d;
    h->tab.set_levels(f.levels);
    return VIO_OK;
}

vio_status vio_frame_counters(const vio_frame *h, uint64_t *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->counters, sizeof(h->counters));
    return VIO_OK;
}

vio_status vio_frame_timing(vio_frame *h, double *out8) {
    if (!h || !out8) return VIO_ERR_BAD_ARG;
    DeviceScope dev(h->device);
    read_push_timing(h);
    std::memcpy(out8, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_frame_reset(vio_frame *h, int32_t slot) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!FrameTable::slot_ok(slot)) return fail_check(h, "vio_frame_reset", FRAME_BAD_SLOT, 0, slot);
    h->tab.reset(slot);
    return VIO_OK;
}

vio_status vio_frame_push_batch(vio_frame *h, int32_t count, const vio_frame_push_item *items) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && !items))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_push_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    // every argument of every item first: nothing is written, launched or rolled on an error
    std::vector<int32_t> sl((size_t)count), ww((size_t)count), hh((size_t)count);
    for (int i = 0; i < count; ++i) { sl[(size_t)i] = items[i].slot; ww[(size_t)i] = items[i].width; hh[(size_t)i] = items[i].height; }
    int32_t bad = -1;
    const FrameCheck ck = h->tab.check_push(count, sl.data(), ww.data(), hh.data(), &bad);
    if (ck != FRAME_OK) return fail_check(h, "vio_frame_push_batch", ck, bad, sl[(size_t)bad]);
    const vio_status st = check_images(h, "vio_frame_push_batch", count, items);
    return st != VIO_OK ? st : push_run(h, count, items, t0);
}

vio_status vio_frame_set_mask(vio_frame *h, int32_t slot, const uint8_t *mask, int32_t width, int32_t height, int32_t stride) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!FrameTable::slot_ok(slot)) return fail_check(h, "vio_frame_set_mask", FRAME_BAD_SLOT, 0, slot);
    if (!mask) { h->tab.clear_mask(slot); return VIO_OK; }
    FrameLayout Y;
    if (!frame_mask_layout(width, height, Y) || stride < width)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_mask: width and height must be in [1, %d] and stride >= width", VIO_FRAME_MAX_DIM);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    wait_staged(h);
    vio_status st;
    if ((st = h->raw.ensure(h->err, (size_t)Y.bytes)) != VIO_OK) return st;
    const int blk = h->tab.set_mask(slot, width, height, device_block);
    if (blk < 0) return fail(h->err, VIO_ERR_HIP, "vio_frame_set_mask: no device memory for a mask of %lld bytes", (long long)Y.bytes);
    pack_rows(h->raw.h, Y.pitch[0], mask, width, height, stride);
    const bool ok = hipMemcpyAsync(h->tab.level_ptr(blk, Y, 0), h->raw.h, (size_t)Y.pitch[0] * (size_t)height, hipMemcpyHostToDevice,
                                   h->q.stream) == hipSuccess;
    mark_staged(h);
    if (!ok) return fail_synced(h, "upload failed");
    h->counters[0] += (uint64_t)width * (uint64_t)height;
    return VIO_OK;
}

vio_status vio_frame_download(vio_frame *h, int32_t slot, int32_t which, int32_t level, uint8_t *out) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!out) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_download: a NULL array");
    const FrameCheck ck = h->tab.check_frame(slot, which, level);
    if (ck != FRAME_OK) return fail_check(h, "vio_frame_download", ck, 0, slot);
    const FrameSlot &s = h->tab.slots[slot];
    FrameLayout Y;
    frame_layout(s.width, s.height, h->tab.levels, Y);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const uint8_t *src = h->tab.level_ptr(which == VIO_FRAME_PREV ? s.prev : s.next, Y, level);
    const size_t w = (size_t)Y.w[level], rows = (size_t)Y.h[level];
    if (hipMemcpy2DAsync(out, w, src, (size_t)Y.pitch[level], w, rows, hipMemcpyDeviceToHost, h->q.stream) != hipSuccess ||
        hipStreamSynchronize(h->q.stream) != hipSuccess)
        return fail_synced(h, "read-back failed");
    h->counters[level == 0 ? 1 : 3] += (uint64_t)(w * rows);
    return VIO_OK;
}

vio_status vio_frame_track_batch(vio_frame *h, int32_t count, const vio_frame_track_item *items, float *next_pts, vio_flow_pt_info *info) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !next_pts)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_track_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const int L = h->tab.levels;
    size_t total = 0;
    for (int i = 0; i < count; ++i) {
        const vio_frame_track_item &it = items[i];
        if (it.n_pts < 0 || it.n_pts > VIO_FLOW_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_track_batch: item %d: n_pts must be in [0, %d]", i, VIO_FLOW_MAX_POINTS);
        const FrameCheck ck = h->tab.check_track(it.slot);
        if (ck != FRAME_OK) return fail_check(h, "vio_frame_track_batch", ck, i, it.slot);
        if (it.n_pts > 0 && !it.prev_pts) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_track_batch: item %d: prev_pts is required", i);
        total += (size_t)it.n_pts;
    }
    if (total == 0) return VIO_OK;
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_it = align256(sizeof(kf::FlowItemD) * (size_t)count), b_tab = b_it + sizeof(kf::FlowPt) * total;
    vio_status st;
    if ((st = h->ttab.ensure(h->err, b_tab)) != VIO_OK || (st = h->tout.ensure(h->err, sizeof(kf::FlowOut) * total)) != VIO_OK) return st;
    std::memset(h->ttab.h, 0, b_it);
    kf::FlowItemD *fi = (kf::FlowItemD *)h->ttab.h;
    kf::FlowPt *hp = (kf::FlowPt *)(h->ttab.h + b_it);
    size_t row = 0;
    for (int i = 0; i < count; ++i) {
        const vio_frame_track_item &it = items[i];
        if (it.n_pts == 0) continue;
        const FrameSlot &s = h->tab.slots[it.slot];
        FrameLayout Y;
        frame_layout(s.width, s.height, L, Y);
        kf::FlowItemD &f = fi[i];
        f.active = 1;
        for (int l = 0; l < L; ++l) {
            f.w[l] = Y.w[l]; f.h[l] = Y.h[l]; f.pitch[l] = Y.pitch[l];
            f.prev[l] = h->tab.level_ptr(s.prev, Y, l); f.next[l] = h->tab.level_ptr(s.next, Y, l);
        }
        for (int k = 0; k < it.n_pts; ++k) {
            kf::FlowPt &p = hp[row + (size_t)k];
            p.item = i; p.has_guess = it.guess != nullptr;
            p.px = it.prev_pts[2 * k]; p.py = it.prev_pts[2 * k + 1];
            p.gx = it.guess ? it.guess[2 * k] : 0.f; p.gy = it.guess ? it.guess[2 * k + 1] : 0.f;
        }
        row += (size_t)it.n_pts;
    }
    kf::FlowArgs a;
    a.items = (const kf::FlowItemD *)h->ttab.d;
    a.pts = (const kf::FlowPt *)(h->ttab.d + b_it);
    a.out = h->tout.d;
    a.npts = (int32_t)total; a.levels = L; a.half_patch = h->fcfg.half_patch; a.max_iter = h->fcfg.max_iter;
    a.border = h->fcfg.border; a.early_stop = h->fcfg.early_stop;
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->ttab.d, h->ttab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess) return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[4], q);
    const dim3 grid((unsigned)((total + kf::WAVES - 1) / kf::WAVES));
    if (h->fcfg.inverse) hipLaunchKernelGGL(kf::k_flow_track<true>, grid, dim3(kf::NT), 0, q, a);
    else hipLaunchKernelGGL(kf::k_flow_track<false>, grid, dim3(kf::NT), 0, q, a);
    (void)hipEventRecord(h->q.ev[5], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    const size_t outb = sizeof(kf::FlowOut) * total;
    if (hipMemcpyAsync(h->tout.h, h->tout.d, outb, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    h->counters[2] += b_tab; h->counters[3] += outb;
    vio_status ret = VIO_OK;
    row = 0;
    for (int i = 0; i < count; ++i) {
        for (int k = 0; k < items[i].n_pts; ++k) {
            const kf::FlowOut &o = h->tout.h[row + (size_t)k];
            next_pts[2 * (row + k)] = o.x; next_pts[2 * (row + k) + 1] = o.y;
            if (info) {
                vio_flow_pt_info &pi = info[row + k];
                pi.status = o.status; pi.iterations = o.iterations; pi.cost = o.cost;
            }
            if (o.status == VIO_ERR_NOT_FINITE) {
                if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "item %d: keypoint %d or its guess is not finite", i, k);
                ret = VIO_ERR_NOT_FINITE;
            }
        }
        row += (size_t)items[i].n_pts;
    }
    h->timing[4] = elapsed_ms(h->q.ev[4], h->q.ev[5]);
    h->timing[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

vio_status vio_frame_detect_batch(vio_frame *h, int32_t count, const vio_frame_detect_item *items, vio_detect_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_detect_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    // every argument of every item first: nothing is written or launched on an error
    std::vector<kd::DetItemD> its((size_t)count);
    int64_t n_r = 0, n_cand = 0, n_trk = 0, n_new = 0;
    int max_tiles = 0;
    for (int i = 0; i < count; ++i) {
        const vio_frame_detect_item &it = items[i];
        if (it.n_tracked < 0 || it.n_tracked > VIO_DETECT_MAX_POINTS || it.max_total < 0 || it.max_total > VIO_DETECT_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_detect_batch: item %d: n_tracked and max_total must be in [0, %d]", i, VIO_DETECT_MAX_POINTS);
        const FrameCheck ck = h->tab.check_detect(it.slot);
        if (ck != FRAME_OK) return fail_check(h, "vio_frame_detect_batch", ck, i, it.slot);
        if ((it.n_tracked > 0 && (!it.tracked || !it.track_cnt || !it.keep_order)) || (it.max_total > 0 && !it.new_pts))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_detect_batch: item %d: tracked, track_cnt, keep_order, new_pts are required where they have rows", i);
        const FrameSlot &s = h->tab.slots[it.slot];
        kd::DetItemD &d = its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        d.active = 1;
        for (int k = 0; k < it.n_tracked; ++k) {
            const double x = it.tracked[2 * k], y = it.tracked[2 * k + 1];
            if (!std::isfinite(x) || !std::isfinite(y)) { d.active = 0; continue; }
            const double rx = std::nearbyint(x), ry = std::nearbyint(y);
            if (rx < 0.0 || rx >= (double)s.width || ry < 0.0 || ry >= (double)s.height)
                return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_detect_batch: item %d: tracked point %d (%g, %g) rounds to a pixel outside the %d x %d image",
                            i, k, x, y, s.width, s.height);
        }
        FrameLayout Y;
        frame_layout(s.width, s.height, h->tab.levels, Y);
        d.w = s.width; d.h = s.height; d.pitch = Y.pitch[0];
        d.tiles_x = (s.width + kd::TX - 1) / kd::TX;
        d.tiles = d.tiles_x * ((s.height + kd::TY - 1) / kd::TY);
        d.n_tracked = it.n_tracked; d.max_total = it.max_total;
        d.has_mask = s.mask >= 0;
        d.trk = (int32_t)n_trk; d.newp = (int32_t)n_new;
        n_trk += it.n_tracked; n_new += it.max_total;
        if (!d.active) continue;
        const int64_t px = (int64_t)s.width * s.height;
        d.img = h->tab.level_ptr(s.next, Y, 0);
        if (d.has_mask) d.mask = (const uint8_t *)h->tab.pool.blocks[(size_t)s.mask].base;
        d.r = n_r; n_r += px;
        d.cand = n_cand; n_cand += (int64_t)std::max(s.width - 2, 0) * std::max(s.height - 2, 0);
        max_tiles = std::max(max_tiles, d.tiles);
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_it = align256(sizeof(kd::DetItemD) * (size_t)count), b_tab = b_it + sizeof(kd::DetTrk) * (size_t)n_trk;
    const size_t b_res = align256(sizeof(kd::DetRes) * (size_t)count), b_keep = align256(sizeof(int32_t) * (size_t)n_trk);
    const size_t b_out = b_res + b_keep + sizeof(float) * 2 * (size_t)n_new;
    const size_t b_key = align256(sizeof(unsigned long long) * (size_t)n_trk);
    vio_status st;
    if ((st = h->dtab.ensure(h->err, b_tab)) != VIO_OK || (st = h->dout.ensure(h->err, b_out)) != VIO_OK ||
        (st = h->r.ensure(h->err, sizeof(double) * (size_t)n_r)) != VIO_OK ||
        (st = h->cand.ensure(h->err, sizeof(uint32_t) * (size_t)n_cand)) != VIO_OK ||
        (st = h->scratch.ensure(h->err, b_key + sizeof(int32_t) * 2 * (size_t)n_trk)) != VIO_OK)
        return st;
    std::memcpy(h->dtab.h, its.data(), sizeof(kd::DetItemD) * (size_t)count);
    kd::DetTrk *ht = (kd::DetTrk *)(h->dtab.h + b_it);
    for (int i = 0; i < count; ++i) {
        const vio_frame_detect_item &it = items[i];
        const kd::DetItemD &d = its[(size_t)i];
        for (int k = 0; k < it.n_tracked; ++k) {
            kd::DetTrk &t = ht[d.trk + k];
            t.cx = 0; t.cy = 0; t.cnt = 0; t.pad = 0;
            if (!d.active) continue;
            t.cx = (int32_t)std::nearbyint((double)it.tracked[2 * k]); t.cy = (int32_t)std::nearbyint((double)it.tracked[2 * k + 1]);
            t.cnt = it.track_cnt[k];
        }
    }
    kd::DetArgs a;
    a.items = (const kd::DetItemD *)h->dtab.d;
    a.trk = (const kd::DetTrk *)(h->dtab.d + b_it);
    a.r = h->r.d; a.cand = h->cand.d;
    a.tkey = (unsigned long long *)h->scratch.d;
    a.kept_xy = (int32_t *)(h->scratch.d + b_key);
    a.res = (kd::DetRes *)h->dout.d;
    a.keep_order = (int32_t *)(h->dout.d + b_res);
    a.new_pts = (float *)(h->dout.d + b_res + b_keep);
    a.quality = h->dcfg.quality; a.d2 = det_d2(h->dcfg.min_distance); a.count = count;
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->dtab.d, h->dtab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess || hipMemsetAsync(h->dout.d, 0, b_res, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[6], q);
    if (n_trk > 0) hipLaunchKernelGGL(kd::k_detect_setmask, dim3((unsigned)count), dim3(kd::NT_MASK), 0, q, a);
    if (max_tiles > 0) hipLaunchKernelGGL(kd::k_detect_response, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(kd::NT), 0, q, a);
    if (max_tiles > 0) hipLaunchKernelGGL(kd::k_detect_candidates, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(kd::NT), 0, q, a);
    if (max_tiles > 0) hipLaunchKernelGGL(kd::k_detect_select, dim3((unsigned)count), dim3(kd::NT_SEL), 0, q, a);
    (void)hipEventRecord(h->q.ev[7], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    if (hipMemcpyAsync(h->dout.h, h->dout.d, b_out, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    h->counters[2] += b_tab; h->counters[3] += b_out;
    vio_status ret = VIO_OK;
    const kd::DetRes *res = (const kd::DetRes *)h->dout.h;
    const int32_t *keep = (const int32_t *)(h->dout.h + b_res);
    const float *newp = (const float *)(h->dout.h + b_res + b_keep);
    for (int i = 0; i < count; ++i) {
        const vio_frame_detect_item &it = items[i];
        const kd::DetItemD &d = its[(size_t)i];
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
    h->timing[6] = elapsed_ms(h->q.ev[6], h->q.ev[7]);
    h->timing[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

vio_status vio_frame_set_camera(vio_frame *h, const vio_reject_camera *cam, const vio_reject_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    // (the rules of vio_reject_set_camera and vio_reject_set_config)
    if (!cam) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_camera: NULL camera");
    if (cam->model != VIO_REJECT_MODEL_PINHOLE) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_camera: model %d: only PINHOLE is built", cam->model);
    const double v[8] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->k1, cam->k2, cam->p1, cam->p2};
    for (double x : v)
        if (!std::isfinite(x)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_camera: a parameter is not finite");
    if (cam->fx == 0.0 || cam->fy == 0.0 || cam->width < 1 || cam->height < 1)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_camera: fx, fy must not be 0, width and height at least 1");
    const vio_reject_config c0 = {0u, VIO_REJECT_DEFAULT_HYPOTHESES, VIO_REJECT_DEFAULT_F_THRESHOLD, VIO_REJECT_DEFAULT_FOCAL_LENGTH};
    const vio_reject_config c = cfg ? *cfg : c0;
    if (c.ransac_hypotheses < 1 || c.ransac_hypotheses > VIO_REJECT_MAX_HYPOTHESES || !(c.f_threshold > 0.0) || !std::isfinite(c.f_threshold) ||
        !(c.focal_length > 0.0) || !std::isfinite(c.focal_length))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_camera: ransac_hypotheses in [1, %d], f_threshold and focal_length finite and > 0",
                    VIO_REJECT_MAX_HYPOTHESES);
    h->camera = *cam;
    h->camera.reserved = 0;
    h->cam = rej_camera(cam->fx, cam->fy, cam->cx, cam->cy, cam->k1, cam->k2, cam->p1, cam->p2);
    h->rcfg = c;
    h->have_camera = true;
    return VIO_OK;
}

vio_status vio_frame_set_tracker(vio_frame *h, int32_t max_cnt, int32_t border) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (max_cnt < 0 || max_cnt > VIO_FRAME_MAX_TRACK_POINTS || border < 0)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_tracker: max_cnt in [0, %d], border >= 0", VIO_FRAME_MAX_TRACK_POINTS);
    h->max_cnt = max_cnt; h->border = border;
    return VIO_OK;
}

vio_status vio_frame_read_timing(const vio_frame *h, double *out8) {
    if (!h || !out8) return VIO_ERR_BAD_ARG;
    std::memcpy(out8, h->rtiming, sizeof(h->rtiming));
    return VIO_OK;
}

vio_status vio_frame_points_set(vio_frame *h, int32_t slot, int32_t n, const float *pts, const int64_t *ids, const int32_t *track_cnt) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const FrameCheck ck = h->tab.check_points_set(slot, n);
    if (ck != FRAME_OK) return fail_check(h, "vio_frame_points_set", ck, 0, slot);
    if (n > 0 && (!pts || !ids || !track_cnt)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_points_set: pts, ids and track_cnt are required");
    const FrameSlot &s = h->tab.slots[slot];
    for (int k = 0; k < n; ++k) {
        const float x = pts[2 * k], y = pts[2 * k + 1];
        if (!std::isfinite(x) || !std::isfinite(y) || !front_in_border(x, y, s.width, s.height, 0))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_points_set: point %d (%g, %g) is not finite or rounds to a pixel outside the %d x %d frame",
                        k, (double)x, (double)y, s.width, s.height);
        if (ids[k] < -1) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_points_set: point %d: an id is -1 or not negative", k);
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const vio_status st = ensure_points(h);
    if (st != VIO_OK) return st;
    if (n > 0) {
        const SlotPts p = slot_pts(h, slot);
        hipStream_t q = h->q.stream;
        if (hipMemcpyAsync(p.cur, pts, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, q) != hipSuccess ||
            hipMemcpyAsync(p.ids, ids, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, q) != hipSuccess ||
            hipMemcpyAsync(p.cnt, track_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, q) != hipSuccess ||
            hipStreamSynchronize(q) != hipSuccess)
            return fail_synced(h, "upload failed");
        h->counters[2] += 20 * (uint64_t)n;
    }
    h->tab.points_set(slot, n);
    return VIO_OK;
}

vio_status vio_frame_points_get(vio_frame *h, int32_t slot, int32_t *n, float *pts, int64_t *ids, int32_t *track_cnt, int32_t *m,
                                int64_t *prev_un_ids, float *prev_un_pts, int64_t *next_id) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!FrameTable::slot_ok(slot)) return fail_check(h, "vio_frame_points_get", FRAME_BAD_SLOT, 0, slot);
    const FrameSlot &s = h->tab.slots[slot];
    const size_t np = h->ptsd.d ? (size_t)s.n_pts : 0, mp = h->ptsd.d ? (size_t)s.n_prev_un : 0;
    if (n) *n = (int32_t)np;
    if (m) *m = (int32_t)mp;
    if (next_id) *next_id = 0;
    if (!h->ptsd.d) return VIO_OK;
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const SlotPts p = slot_pts(h, slot);
    hipStream_t q = h->q.stream;
    bool ok = true;
    uint64_t bytes = 0;
    const auto get = [&](void *dst, const void *src, size_t b) {
        if (!dst || b == 0) return;
        ok = ok && hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, q) == hipSuccess;
        bytes += b;
    };
    get(pts, p.cur, sizeof(float) * 2 * np); get(ids, p.ids, sizeof(int64_t) * np); get(track_cnt, p.cnt, sizeof(int32_t) * np);
    get(prev_un_ids, p.prev_ids, sizeof(int64_t) * mp); get(prev_un_pts, p.prev_pts, sizeof(float) * 2 * mp);
    get(next_id, p.next_id, sizeof(int64_t));
    if (!ok || hipStreamSynchronize(q) != hipSuccess) return fail_synced(h, "read-back failed");
    h->counters[3] += bytes;
    return VIO_OK;
}

vio_status vio_frame_read_batch(vio_frame *h, int32_t count, const vio_frame_read_item *items, int32_t publish, vio_frame_read_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_read_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    if (publish != 0 && publish != 1) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_read_batch: publish 0 or 1");
    if (count == 0) return VIO_OK;
    if (!h->have_camera) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_read_batch: no camera set");
    const auto t0 = std::chrono::steady_clock::now();
    // every argument of every item first: nothing is written, launched or rolled on an error
    const size_t B = (size_t)count;
    std::vector<int32_t> sl(B), ww(B), hh(B);
    std::vector<double> tt(B);
    std::vector<vio_frame_push_item> push(B);
    for (size_t i = 0; i < B; ++i) {
        const vio_frame_read_item &it = items[i];
        sl[i] = it.slot; ww[i] = it.width; hh[i] = it.height; tt[i] = it.time;
        push[i].slot = it.slot; push[i].width = it.width; push[i].height = it.height; push[i].stride = it.stride; push[i].img = it.img;
    }
    int32_t bad = -1;
    const FrameCheck ck = h->tab.check_read(count, sl.data(), ww.data(), hh.data(), tt.data(), publish != 0, &bad);
    if (ck != FRAME_OK) return fail_check(h, "vio_frame_read_batch", ck, bad, sl[(size_t)bad]);
    vio_status st = check_images(h, "vio_frame_read_batch", count, push.data());
    if (st != VIO_OK) return st;
    for (int i = 0; i < count; ++i)
        if (!items[i].pts || !items[i].ids || !items[i].track_cnt || !items[i].un_pts || !items[i].velocity)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_read_batch: item %d: pts, ids, track_cnt, un_pts and velocity are required", i);
    // what the host knows of each slot before the roll
    std::vector<FrameSlot> was(B);
    int64_t total = 0, n_r = 0, n_cand = 0;
    int rows_cap = std::max(h->max_cnt, 1), max_tiles = 0;
    for (size_t i = 0; i < B; ++i) {
        was[i] = h->tab.slots[sl[i]];
        if (was[i].n_frames < 1) was[i].n_pts = 0;          // (points lie in a frame)
        total += was[i].n_pts;
        rows_cap = std::max(rows_cap, was[i].n_pts);
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    // the tables that travel: their size depends on the count of items alone
    const size_t o_flow = align256(sizeof(FrontItem) * B), o_det = o_flow + align256(sizeof(kf::FlowItemD) * B);
    const size_t o_pair = o_det + align256(sizeof(kd::DetItemD) * B), o_lift = o_pair + align256(sizeof(kr::RejPair) * B);
    const size_t b_tab = o_lift + align256(sizeof(kr::LiftItem) * B);
    // the device work space, every per-point array at FRONT_CAP rows per item
    size_t b_work = 0;
    const auto carve = [&](size_t bytes) { const size_t at = b_work; b_work += align256(bytes); return at; };
    const size_t rowsN = B * CAP;
    const size_t w_dres = carve(sizeof(kd::DetRes) * B), w_rres = carve(sizeof(kr::RejRes) * B), b_zero = b_work;
    const size_t w_fpts = carve(sizeof(kf::FlowPt) * rowsN), w_fout = carve(sizeof(kf::FlowOut) * rowsN);
    const size_t w_rstage = carve(sizeof(float) * 4 * rowsN), w_corr = carve(sizeof(double) * 4 * rowsN);
    const size_t w_flag = carve(sizeof(int32_t) * rowsN), w_rmask = carve(rowsN);
    const size_t w_fa = carve(sizeof(float) * 2 * rowsN), w_ida = carve(sizeof(long long) * rowsN), w_cnta = carve(sizeof(int32_t) * rowsN);
    const size_t w_fb = carve(sizeof(float) * 2 * rowsN), w_idb = carve(sizeof(long long) * rowsN), w_cntb = carve(sizeof(int32_t) * rowsN);
    const size_t w_trk = carve(sizeof(kd::DetTrk) * rowsN), w_tkey = carve(sizeof(unsigned long long) * rowsN);
    const size_t w_kxy = carve(sizeof(int32_t) * 2 * rowsN), w_keep = carve(sizeof(int32_t) * rowsN), w_new = carve(sizeof(float) * 2 * rowsN);
    const size_t w_lstage = carve(sizeof(float) * 4 * rowsN), w_lids = carve(sizeof(long long) * 2 * rowsN);
    const size_t w_un = carve(sizeof(float) * 2 * rowsN), w_vel = carve(sizeof(float) * 2 * rowsN), w_cntm = carve(sizeof(int32_t) * rowsN);
    const size_t row_bytes = (36 * (size_t)rows_cap + 7) & ~(size_t)7;
    const size_t b_res = align256(sizeof(FrontRes) * B), b_out = b_res + row_bytes * B;
    for (size_t i = 0; i < B; ++i) {
        n_r += (int64_t)ww[i] * hh[i];
        n_cand += (int64_t)std::max(ww[i] - 2, 0) * std::max(hh[i] - 2, 0);
    }
    if ((st = ensure_points(h)) != VIO_OK || (st = h->rtab.ensure(h->err, b_tab)) != VIO_OK || (st = h->rwork.ensure(h->err, b_work)) != VIO_OK ||
        (st = h->rout.ensure(h->err, b_out)) != VIO_OK ||
        (publish && ((st = h->r.ensure(h->err, sizeof(double) * (size_t)n_r)) != VIO_OK ||
                     (st = h->cand.ensure(h->err, sizeof(uint32_t) * (size_t)n_cand)) != VIO_OK)))
        return st;
    // 1. the push: from here on the slots name the new frames
    if ((st = push_run(h, count, push.data(), t0)) != VIO_OK) return st;
    const int L = h->tab.levels;
    std::memset(h->rtab.h, 0, b_tab);
    FrontItem *fr = (FrontItem *)h->rtab.h;
    kf::FlowItemD *fi = (kf::FlowItemD *)(h->rtab.h + o_flow);
    kd::DetItemD *di = (kd::DetItemD *)(h->rtab.h + o_det);
    kr::RejPair *rp = (kr::RejPair *)(h->rtab.h + o_pair);
    kr::LiftItem *li = (kr::LiftItem *)(h->rtab.h + o_lift);
    n_r = 0; n_cand = 0;
    int64_t flow_off = 0;
    for (size_t i = 0; i < B; ++i) {
        const FrameSlot &s = h->tab.slots[sl[i]];
        const SlotPts p = slot_pts(h, sl[i]);
        FrameLayout Y;
        frame_layout(s.width, s.height, L, Y);
        FrontItem &f = fr[i];
        f.cur_pts = p.cur; f.ids = p.ids; f.cnt = p.cnt; f.prev_un_ids = p.prev_ids; f.prev_un_pts = p.prev_pts; f.next_id = p.next_id;
        f.n = s.n_frames == 2 ? was[i].n_pts : 0; f.m = was[i].n_prev_un;
        f.w = s.width; f.h = s.height; f.flow_off = (int32_t)flow_off;
        flow_off += f.n;
        if (f.n > 0) {
            kf::FlowItemD &d = fi[i];
            d.active = 1;
            for (int l = 0; l < L; ++l) {
                d.w[l] = Y.w[l]; d.h[l] = Y.h[l]; d.pitch[l] = Y.pitch[l];
                d.prev[l] = h->tab.level_ptr(s.prev, Y, l); d.next[l] = h->tab.level_ptr(s.next, Y, l);
            }
        }
        kd::DetItemD &d = di[i];
        d.w = s.width; d.h = s.height; d.pitch = Y.pitch[0];
        d.tiles_x = (s.width + kd::TX - 1) / kd::TX;
        d.tiles = d.tiles_x * ((s.height + kd::TY - 1) / kd::TY);
        d.n_tracked = 0; d.max_total = h->max_cnt;          // (n_tracked is k_front_after_reject's to write)
        d.active = 1; d.has_mask = s.mask >= 0;
        d.trk = (int32_t)(i * CAP); d.newp = (int32_t)(i * CAP);
        d.img = h->tab.level_ptr(s.next, Y, 0);
        if (d.has_mask) d.mask = (const uint8_t *)h->tab.pool.blocks[(size_t)s.mask].base;
        d.r = n_r; n_r += (int64_t)s.width * s.height;
        d.cand = n_cand; n_cand += (int64_t)std::max(s.width - 2, 0) * std::max(s.height - 2, 0);
        max_tiles = std::max(max_tiles, d.tiles);
        kr::RejPair &r = rp[i];
        r.pair = was[i].n_read; r.finite = 1;               // (n and active are k_front_filter's to write)
        r.o_pts = (int64_t)(i * 4 * CAP); r.o_corr = (int64_t)(i * 4 * CAP); r.o_pt = (int64_t)(i * CAP);
        kr::LiftItem &u = li[i];
        u.active = 1;                                       // (n and m are k_front_merge's to write)
        u.o_pts = (int64_t)(i * 4 * CAP); u.o_prev = (int64_t)(i * 4 * CAP + 2 * CAP);
        u.o_ids = (int64_t)(i * 2 * CAP); u.o_out = (int64_t)(i * CAP);
        u.dt = was[i].n_prev_un > 0 ? tt[i] - was[i].time : 1.0;
    }
    total = flow_off;
    char *W = h->rwork.d;
    FrontArgs a;
    std::memset(&a, 0, sizeof(a));
    a.items = (const FrontItem *)h->rtab.d;
    a.fpts = (kf::FlowPt *)(W + w_fpts); a.fout = (const kf::FlowOut *)(W + w_fout);
    a.pairs = (kr::RejPair *)(h->rtab.d + o_pair);
    a.rstage = (float *)(W + w_rstage); a.rmask = (const uint8_t *)(W + w_rmask); a.rres = (const kr::RejRes *)(W + w_rres);
    a.fa = (float *)(W + w_fa); a.ida = (long long *)(W + w_ida); a.cnta = (int32_t *)(W + w_cnta);
    a.fb = (float *)(W + w_fb); a.idb = (long long *)(W + w_idb); a.cntb = (int32_t *)(W + w_cntb);
    a.ditems = (kd::DetItemD *)(h->rtab.d + o_det); a.dtrk = (kd::DetTrk *)(W + w_trk); a.dres = (const kd::DetRes *)(W + w_dres);
    a.keep_order = (const int32_t *)(W + w_keep); a.new_pts = (const float *)(W + w_new);
    a.litems = (kr::LiftItem *)(h->rtab.d + o_lift);
    a.lstage = (float *)(W + w_lstage); a.lids = (long long *)(W + w_lids);
    a.un = (const float *)(W + w_un); a.vel = (const float *)(W + w_vel); a.cntm = (int32_t *)(W + w_cntm);
    a.res = (FrontRes *)h->rout.d; a.rows = h->rout.d + b_res; a.row_bytes = (int64_t)row_bytes; a.rows_cap = rows_cap;
    a.count = count; a.publish = publish; a.border = h->border;
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->rtab.d, h->rtab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess || hipMemsetAsync(W, 0, b_zero, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    const auto t1 = std::chrono::steady_clock::now();
    const dim3 per_item((unsigned)count), fnt(FNT);
    // 2 - 4. the slot's points into the new frame, and those that stay
    if (total > 0) {
        hipLaunchKernelGGL(k_front_begin, per_item, fnt, 0, q, a);
        kf::FlowArgs fa;
        fa.items = (const kf::FlowItemD *)(h->rtab.d + o_flow);
        fa.pts = a.fpts; fa.out = (kf::FlowOut *)(W + w_fout);
        fa.npts = (int32_t)total; fa.levels = L; fa.half_patch = h->fcfg.half_patch; fa.max_iter = h->fcfg.max_iter;
        fa.border = h->fcfg.border; fa.early_stop = h->fcfg.early_stop;
        const dim3 grid((unsigned)((total + kf::WAVES - 1) / kf::WAVES));
        if (h->fcfg.inverse) hipLaunchKernelGGL(kf::k_flow_track<true>, grid, dim3(kf::NT), 0, q, fa);
        else hipLaunchKernelGGL(kf::k_flow_track<false>, grid, dim3(kf::NT), 0, q, fa);
    }
    hipLaunchKernelGGL(k_front_filter, per_item, fnt, 0, q, a);
    (void)hipEventRecord(h->rev[0], q);
    if (publish) {
        // 5, 6. rejectWithF and what it keeps
        kr::RansacArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.pairs = a.pairs; ra.pts = a.rstage;
        ra.corr = (double *)(W + w_corr); ra.flag = (int32_t *)(W + w_flag); ra.mask = (uint8_t *)(W + w_rmask); ra.res = (kr::RejRes *)(W + w_rres);
        ra.cam = h->cam;
        ra.focal = h->rcfg.focal_length; ra.half_w = h->camera.width / 2.0; ra.half_h = h->camera.height / 2.0;
        ra.thr = h->rcfg.f_threshold * h->rcfg.f_threshold;
        ra.seed = h->rcfg.seed; ra.hyps = h->rcfg.ransac_hypotheses;
        if (total > 0) hipLaunchKernelGGL(kr::k_reject_ransac, per_item, dim3(kr::NT), 0, q, ra);
        hipLaunchKernelGGL(k_front_after_reject, per_item, fnt, 0, q, a);
        (void)hipEventRecord(h->rev[1], q);
        // 7. setMask and the detection
        kd::DetArgs da;
        da.items = a.ditems; da.trk = a.dtrk;
        da.r = h->r.d; da.cand = h->cand.d;
        da.tkey = (unsigned long long *)(W + w_tkey); da.kept_xy = (int32_t *)(W + w_kxy);
        da.res = (kd::DetRes *)(W + w_dres);
        da.keep_order = (int32_t *)(W + w_keep); da.new_pts = (float *)(W + w_new);
        da.quality = h->dcfg.quality; da.d2 = det_d2(h->dcfg.min_distance); da.count = count;
        if (total > 0) hipLaunchKernelGGL(kd::k_detect_setmask, per_item, dim3(kd::NT_MASK), 0, q, da);
        hipLaunchKernelGGL(kd::k_detect_response, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(kd::NT), 0, q, da);
        hipLaunchKernelGGL(kd::k_detect_candidates, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(kd::NT), 0, q, da);
        hipLaunchKernelGGL(kd::k_detect_select, per_item, dim3(kd::NT_SEL), 0, q, da);
    } else {
        (void)hipEventRecord(h->rev[1], q);
    }
    (void)hipEventRecord(h->rev[2], q);
    // 8 - 10. the merged point set, undistortedPoints, updateID and the roll
    hipLaunchKernelGGL(k_front_merge, per_item, fnt, 0, q, a);
    kr::LiftArgs la;
    std::memset(&la, 0, sizeof(la));
    la.items = a.litems; la.pts = a.lstage; la.ids = a.lids;
    la.un = (float *)(W + w_un); la.vel = (float *)(W + w_vel); la.lifted = nullptr;
    la.cam = h->cam; la.bare = 0; la.count = count;
    hipLaunchKernelGGL(kr::k_reject_lift, dim3((unsigned)((rows_cap + kr::NT - 1) / kr::NT), (unsigned)count), dim3(kr::NT), 0, q, la);
    hipLaunchKernelGGL(k_front_finish, per_item, fnt, 0, q, a);
    (void)hipEventRecord(h->rev[3], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    // 11. what is published comes down, and the call waits
    if (hipMemcpyAsync(h->rout.h, h->rout.d, b_out, hipMemcpyDeviceToHost, q) != hipSuccess) return fail_synced(h, "read-back failed");
    (void)hipEventRecord(h->rev[4], q);
    if (hipStreamSynchronize(q) != hipSuccess) return fail_synced(h, "kernel or read-back failed");
    h->counters[2] += b_tab; h->counters[3] += b_out;
    const FrontRes *res = (const FrontRes *)h->rout.h;
    for (size_t i = 0; i < B; ++i) {
        const vio_frame_read_item &it = items[i];
        const FrontRes &r = res[i];
        const size_t R = (size_t)rows_cap, n = (size_t)front_clamp(r.n, 0, rows_cap);
        const char *base = h->rout.h + b_res + i * row_bytes;
        std::memcpy(it.ids, base, sizeof(int64_t) * n);
        std::memcpy(it.pts, base + 8 * R, sizeof(float) * 2 * n);
        std::memcpy(it.un_pts, base + 16 * R, sizeof(float) * 2 * n);
        std::memcpy(it.velocity, base + 24 * R, sizeof(float) * 2 * n);
        std::memcpy(it.track_cnt, base + 32 * R, sizeof(int32_t) * n);
        vio_frame_read_result &o = results[i];
        o.status = VIO_OK; o.n = (int32_t)n; o.n_new = front_clamp(r.n_new, 0, (int32_t)n);
        o.n_tracked_in = r.n_tracked_in; o.n_after_track = r.n_after_track; o.n_after_reject = r.n_after_reject;
        o.reject_status = r.reject_status; o.reject_hyp = r.reject_hyp; o.n_candidates = r.n_candidates; o.reserved = 0;
        h->tab.points_after_read(it.slot, (int32_t)n, r.next_id, it.time);
    }
    read_push_timing(h);
    h->rtiming[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->rtiming[1] = elapsed_ms(h->q.ev[0], h->q.ev[3]);
    h->rtiming[2] = elapsed_ms(h->q.ev[3], h->rev[0]);
    for (int k = 0; k < 4; ++k) h->rtiming[3 + k] = elapsed_ms(h->rev[k], h->rev[k + 1]);
    h->rtiming[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VIO_OK;
}

}  // extern "C"
