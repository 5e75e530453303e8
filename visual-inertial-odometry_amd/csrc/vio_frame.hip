// vio_frame.hip — libvio_frame_hip.so: frames that stay on the device across CLAHE, tracking and detection (include/vio_frame.h,
// DESIGN.md section 23).
//
// The numeric kernels are those of libvio_clahe_hip, libvio_flow_hip, libvio_detect_hip and libvio_reject_hip, compiled from the same
// four files (vio_clahe_body.inc, vio_flow_body.inc, vio_detect_body.inc, vio_reject_body.inc), each inside a namespace since their
// constants share names.  The five kernels that join them in vio_frame_read_batch are in vio_front_body.inc, the
// three that bring a slot's prediction into its tracking step in vio_front_guess_body.inc (include/vio_frame_predict.h, section 39).
// vio_frame_set_slot_camera (include/vio_frame_camera.h) gives a slot a camera of its own, of any of the four models:
// a read that lists such a slot runs a second instantiation of vio_reject_body.inc (namespace kq, against vio_camera_math.h through
// vio_camera_host.h, as libvio_camera_hip compiles it) and of vio_front_body.inc (namespace fq), every descriptor carrying its slot.
// What is here is the host side that is this library's own: the slot table and the block pool (vio_frame_slots.h, plain C++), the
// descriptor tables that point the kernels at resident frames, and the copies.  The checks, fills, launches and unpacking of a stage
// are those of its library, from vio_{clahe,flow,detect,reject}_host.h and the end of each body.  A frame is
// written by one upload (or by k_clahe_apply out of the upload buffer) and the pyramid kernel, and read in place ever after.
// Contraction is off for all of it, as in the three libraries; in CLAHE it decides bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_frame.h"
#include "vio_companion.h"
#include "vio_frame_slots.h"

#pragma clang fp contract(off)

#include "vio_camera_math.h"
#include "vio_clahe_math.h"
#include "vio_detect_math.h"
#include "vio_flow_math.h"
#include "vio_front_math.h"
#include "vio_front_guess_math.h"
#include "vio_reject_math.h"
#include "vio_sfm_math.h"

namespace kc {
#include "vio_clahe_host.h"
#include "vio_clahe_body.inc"
}
namespace kf {
#include "vio_flow_host.h"
#include "vio_flow_body.inc"
}
namespace kd {
#include "vio_detect_host.h"
#include "vio_detect_body.inc"
}
namespace kr {
#include "vio_reject_host.h"
#include "vio_reject_body.inc"
}
#define FRONT_REJ kr
#include "vio_front_body.inc"
#include "vio_front_guess_body.inc"
#undef FRONT_REJ

// the same two texts against the four camera models and a camera per slot: the lift's customisation points change hands
#undef REJ_RAY
#undef REJ_RAY_UNSET
#undef REJ_ITEM_LIFT
#undef REJ_STORE_BARE
#undef REJ_UN_X
#undef REJ_UN_Y
#undef REJ_PROLOGUE_BEGIN
#undef REJ_PAIR_LIFT
#undef REJ_VIRTUAL_X
#undef REJ_VIRTUAL_Y
#undef REJ_PROLOGUE_END
namespace kq {
#include "vio_camera_host.h"
#include "vio_reject_body.inc"
}
namespace fq {
#define FRONT_REJ kq
#define FRONT_CAMERAS
#include "vio_front_body.inc"
#include "vio_front_guess_body.inc"
#undef FRONT_CAMERAS
#undef FRONT_REJ
}
#include "vio_frame_cameras.h"

static_assert(FRAME_CAM_SLOTS == VIO_FRAME_MAX_SLOTS && FRAME_CAM_SLOTS == VIO_CAMERA_MAX_SLOTS, "a camera per slot");
static_assert(sizeof(fq::FrontItem) == sizeof(FrontItem), "one item table for both sets of joining kernels");
static_assert(sizeof(GuessItem) == 16 && sizeof(GuessRes) == 16 && sizeof(fq::GuessArgs) == sizeof(GuessArgs), "the prediction's tables are the same in both");
static_assert(FRAME_MAX_SLOTS == VIO_FRAME_MAX_SLOTS && FRAME_MAX_LEVELS == VIO_FLOW_MAX_LEVELS && FRAME_MAX_DIM == VIO_FRAME_MAX_DIM,
              "vio_frame_slots.h restates the header's limits");
static_assert(FRAME_MAX_TRACK_POINTS == VIO_FRAME_MAX_TRACK_POINTS && FRONT_CAP == VIO_FRAME_MAX_TRACK_POINTS, "one capacity");
static_assert(VIO_FRAME_MAX_TRACK_POINTS <= VIO_DETECT_MAX_POINTS && VIO_FRAME_MAX_TRACK_POINTS <= VIO_REJECT_MAX_POINTS &&
              VIO_FRAME_MAX_TRACK_POINTS <= VIO_FLOW_MAX_POINTS, "a slot's table fits every library's limits");
static_assert(VIO_FRAME_MAX_DIM == VIO_FLOW_MAX_DIM && VIO_FRAME_MAX_DIM == VIO_DETECT_MAX_DIM && VIO_FRAME_MAX_DIM == VIO_CLAHE_MAX_DIM,
              "one size limit");

// a slot's pending prediction (include/vio_frame_predict.h), as it goes up: front_guess_normalise's rows
struct FramePrediction {
    bool pending = false;
    int32_t n_listed = 0;
    std::vector<long long> ids;
    std::vector<float> px;
    void drop() { pending = false; n_listed = 0; ids.clear(); px.clear(); }
};

struct vio_frame {
    int device = 0;
    ErrText err = {0};
    int32_t equalize = 0;
    vio_clahe_config ccfg = kc::CLAHE_DEFAULTS;
    vio_flow_config fcfg = kf::FLOW_DEFAULTS;
    vio_detect_config dcfg = kd::DET_DEFAULTS;
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
    Twin<kf::FlowBackOut> tbout;                         // the backward rows of a track with the check (include/vio_frame_back.h)
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
    vio_reject_config rcfg = kr::REJ_DEFAULTS;
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
    // the slots' own cameras (vio_frame_cameras.h) and the table's twin, which goes up ahead of a read that needs it when it has changed
    FrameCameras cams;
    Twin<CamDev> camtab;
    // include/vio_frame_back.h: the forward-backward check of the tracker, whether a published read runs rejectWithF, and per slot the
    // check's counts of its last read (checked, lost on the way back, too far)
    vio_flow_back_config bcfg = kf::FLOW_BACK_DEFAULTS;
    int32_t reject_f = 1;
    int32_t back_info[VIO_FRAME_MAX_SLOTS][3] = {};
    // include/vio_frame_predict.h: the slots' pending predictions, the fallback's threshold, and per slot what its last read made of
    // its prediction (listed, guessed, status 0 after the guessed pass, fell back)
    std::vector<FramePrediction> pred = std::vector<FramePrediction>((size_t)VIO_FRAME_MAX_SLOTS);
    int32_t min_tracked = 0;
    int32_t pred_info[VIO_FRAME_MAX_SLOTS][4] = {};
};

namespace {

constexpr int MAX_ITEMS = VIO_FRAME_MAX_SLOTS;

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

// a slot's frames as a flow item: every level's size, pitch and address (prev < 0: the slot's next alone)
void flow_item_of(const vio_frame *h, kf::FlowItemD &f, const FrameLayout &Y, int prev, int next) {
    kf::flow_item(f, h->tab.levels, Y.w, Y.h, Y.pitch);
    for (int l = 0; l < h->tab.levels; ++l) {
        if (prev >= 0) f.prev[l] = h->tab.level_ptr(prev, Y, l);
        f.next[l] = h->tab.level_ptr(next, Y, l);
    }
}

// ... and its newest frame, with the slot's mask if it has one, as a detection item (d zeroed, then d.active decided)
void det_item_of(const vio_frame *h, kd::DetItemD &d, kd::DetTotals &T, const FrameSlot &s, int n_tracked, int max_total) {
    FrameLayout Y;
    frame_layout(s.width, s.height, h->tab.levels, Y);
    kd::det_item(d, T, s.width, s.height, Y.pitch[0], n_tracked, max_total, s.mask >= 0);
    if (!d.active) return;
    d.img = h->tab.level_ptr(s.next, Y, 0);
    if (d.has_mask) d.mask = (const uint8_t *)h->tab.pool.blocks[(size_t)s.mask].base;
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
    const int L = h->tab.levels, tiles = h->ccfg.tiles_x * h->ccfg.tiles_y;
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
        flow_item_of(h, fi[i], Y, -1, blk);
        pack_rows(h->raw.h + at[(size_t)i], Y.pitch[0], it.img, it.width, it.height, it.stride);
        if (!h->equalize) continue;
        kc::ClaheItemD &d = ci[i];
        kc::clahe_item(d, it.width, it.height, Y.pitch[0], h->ccfg);
        d.src = h->raw.d + at[(size_t)i];
        d.dst = fi[i].next[0];
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
    if (h->equalize) kc::clahe_launch(q, kc::clahe_args((const kc::ClaheItemD *)h->ptab.d, h->luts.d, h->ccfg, count), max_ptiles, nullptr);
    (void)hipEventRecord(h->q.ev[2], q);
    kf::flow_launch_pyramids(q, (const kf::FlowItemD *)(h->ptab.d + b_ci), count, 0, L, max_px);
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

// the camera table's twin, allocated at the first read that needs it
vio_status ensure_cameras(vio_frame *h) {
    if (h->camtab.d) return VIO_OK;
    h->cams.dirty = true;
    return h->camtab.ensure(h->err, sizeof(h->cams.table));
}

// The two sets of kernels a read runs (read_run, at the end of the file): the tables and the kernels of each.
template <bool CAMS> struct ReadPath;
template <> struct ReadPath<false> {
    using RejPair = kr::RejPair; using LiftItem = kr::LiftItem; using RejRes = kr::RejRes;
    using RansacArgs = kr::RansacArgs; using LiftArgs = kr::LiftArgs;
    using Item = ::FrontItem; using Res = ::FrontRes; using Args = ::FrontArgs;
    static constexpr auto begin = ::k_front_begin, filter = ::k_front_filter, after_reject = ::k_front_after_reject, merge = ::k_front_merge,
                          finish = ::k_front_finish;
    using GuessItem = ::GuessItem; using GuessRes = ::GuessRes; using GuessArgs = ::GuessArgs;
    static constexpr auto guess = ::k_front_guess, fallback = ::k_front_fallback, take = ::k_front_take;
    static constexpr auto ransac = kr::k_reject_ransac;
};
template <> struct ReadPath<true> {
    using RejPair = kq::RejPair; using LiftItem = kq::LiftItem; using RejRes = kq::RejRes;
    using RansacArgs = kq::RansacArgs; using LiftArgs = kq::LiftArgs;
    using Item = fq::FrontItem; using Res = fq::FrontRes; using Args = fq::FrontArgs;
    static constexpr auto begin = fq::k_front_begin, filter = fq::k_front_filter, after_reject = fq::k_front_after_reject, merge = fq::k_front_merge,
                          finish = fq::k_front_finish;
    using GuessItem = fq::GuessItem; using GuessRes = fq::GuessRes; using GuessArgs = fq::GuessArgs;
    static constexpr auto guess = fq::k_front_guess, fallback = fq::k_front_fallback, take = fq::k_front_take;
    static constexpr auto ransac = kq::k_reject_ransac;
};

template <bool CAMS> vio_status read_run(vio_frame *h, int32_t count, const vio_frame_read_item *items, int32_t publish, vio_frame_read_result *results,
                                         std::chrono::steady_clock::time_point t0, const std::vector<int32_t> &sl, const std::vector<int32_t> &ww,
                                         const std::vector<int32_t> &hh, const std::vector<double> &tt, const std::vector<vio_frame_push_item> &push);

// vio_frame_track_batch, and with the check enabled vio_frame_track_back_batch (back may be NULL): fn names the call in errors
vio_status track_run(vio_frame *h, const char *fn, int32_t count, const vio_frame_track_item *items, float *next_pts, vio_flow_pt_info *info,
                     vio_flow_back_info *back) {
    const bool check = h->bcfg.enabled != 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && (!items || !next_pts)))
        return fail(h->err, VIO_ERR_BAD_ARG, "%s: count outside [0, %d] or a NULL array", fn, MAX_ITEMS);
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const int L = h->tab.levels;
    size_t total = 0;
    for (int i = 0; i < count; ++i) {
        const vio_frame_track_item &it = items[i];
        if (it.n_pts < 0 || it.n_pts > VIO_FLOW_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: n_pts must be in [0, %d]", fn, i, VIO_FLOW_MAX_POINTS);
        const FrameCheck ck = h->tab.check_track(it.slot);
        if (ck != FRAME_OK) return fail_check(h, fn, ck, i, it.slot);
        if (it.n_pts > 0 && !it.prev_pts) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: prev_pts is required", fn, i);
        total += (size_t)it.n_pts;
    }
    if (total == 0) return VIO_OK;
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_it = align256(sizeof(kf::FlowItemD) * (size_t)count), b_tab = b_it + sizeof(kf::FlowPt) * total;
    vio_status st;
    if ((st = h->ttab.ensure(h->err, b_tab)) != VIO_OK || (st = h->tout.ensure(h->err, sizeof(kf::FlowOut) * total)) != VIO_OK ||
        (check && back && (st = h->tbout.ensure(h->err, sizeof(kf::FlowBackOut) * total)) != VIO_OK))
        return st;
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
        flow_item_of(h, fi[i], Y, s.prev, s.next);
        kf::flow_fill_pts(hp + row, i, it);
        row += (size_t)it.n_pts;
    }
    const kf::FlowArgs a = kf::flow_args((const kf::FlowItemD *)h->ttab.d, (const kf::FlowPt *)(h->ttab.d + b_it), h->tout.d, total, L, h->fcfg);
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->ttab.d, h->ttab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess) return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[4], q);
    if (check) kf::flow_launch_track_back(q, kf::flow_back_args(a.items, a.pts, a.out, back ? h->tbout.d : nullptr, total, L, h->fcfg, h->bcfg), h->fcfg.inverse != 0);
    else kf::flow_launch_track(q, a, h->fcfg.inverse != 0);
    (void)hipEventRecord(h->q.ev[5], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    const size_t outb = sizeof(kf::FlowOut) * total, backb = check && back ? sizeof(kf::FlowBackOut) * total : 0;
    if (hipMemcpyAsync(h->tout.h, h->tout.d, outb, hipMemcpyDeviceToHost, q) != hipSuccess ||
        (backb && hipMemcpyAsync(h->tbout.h, h->tbout.d, backb, hipMemcpyDeviceToHost, q) != hipSuccess) || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    h->counters[2] += b_tab; h->counters[3] += outb + backb;
    const vio_status ret = kf::flow_unpack(h->err, h->tout.h, count, items, next_pts, info);
    if (backb) kf::flow_unpack_back(h->tbout.h, count, items, back);
    h->timing[4] = elapsed_ms(h->q.ev[4], h->q.ev[5]);
    h->timing[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

}  // namespace

extern "C" {

int32_t vio_frame_version(void) { return VIO_FRAME_VERSION; }

const char *vio_frame_last_error(const vio_frame *h) { return h ? h->err : "NULL handle"; }

vio_status vio_frame_create(int32_t device, void *stream, vio_frame **out) {
    return create_handle(device, stream, out, vio_frame_destroy, [](vio_frame *h) {
        if (hipEventCreate(&h->staged) != hipSuccess) return false;
        for (hipEvent_t &e : h->rev)
            if (hipEventCreate(&e) != hipSuccess) { e = nullptr; return false; }
        kc::clahe_allow_lds();
        return true;
    });
}

void vio_frame_destroy(vio_frame *h) {
    destroy_handle(h, [](vio_frame *h) {                 // (the stream has been waited for: nothing reads a block any more)
        if (h->staged) (void)hipEventDestroy(h->staged);
        for (hipEvent_t e : h->rev)
            if (e) (void)hipEventDestroy(e);
        h->tab.pool.destroy([](void *p) { (void)hipFree(p); });
    });
}

vio_status vio_frame_set_config(vio_frame *h, int32_t equalize, const vio_clahe_config *clahe, const vio_flow_config *flow,
                                const vio_detect_config *detect) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_clahe_config c = clahe ? *clahe : kc::CLAHE_DEFAULTS;
    const vio_flow_config f = flow ? *flow : kf::FLOW_DEFAULTS;
    vio_detect_config d = detect ? *detect : kd::DET_DEFAULTS;
    if (equalize != 0 && equalize != 1) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_config: equalize 0 or 1");
    vio_status st;
    if ((st = kc::clahe_check_config(h->err, "vio_frame_set_config", &c)) != VIO_OK || (st = kf::flow_check_config(h->err, "vio_frame_set_config", &f)) != VIO_OK ||
        (st = kd::det_check_config(h->err, "vio_frame_set_config", &d)) != VIO_OK)
        return st;
    if (h->bcfg.enabled && h->bcfg.levels > f.levels)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_config: %d flow levels are fewer than the %d of the forward-backward check", f.levels, h->bcfg.levels);
    d.reserved = 0;
    h->equalize = equalize; h->ccfg = c; h->fcfg = f; h->dcfg = d;
    if (f.levels != h->tab.levels)                          // (the slots' points go with their frames, and the predictions with the points)
        for (FramePrediction &p : h->pred) p.drop();
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
    h->cams.lift_info_set(slot, 0, 0);
    for (int32_t &v : h->back_info[slot]) v = 0;
    h->pred[(size_t)slot].drop();
    for (int32_t &v : h->pred_info[slot]) v = 0;
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
    vio_status st = check_images(h, "vio_frame_push_batch", count, items);
    if (st != VIO_OK || (st = push_run(h, count, items, t0)) != VIO_OK) return st;
    for (int i = 0; i < count; ++i) h->pred[(size_t)items[i].slot].drop();     // (as the roll drops the slot's points)
    return VIO_OK;
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
    return track_run(h, "vio_frame_track_batch", count, items, next_pts, info, nullptr);
}

vio_status vio_frame_track_back_batch(vio_frame *h, int32_t count, const vio_frame_track_item *items, float *next_pts, vio_flow_pt_info *info,
                                      vio_flow_back_info *back) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!h->bcfg.enabled) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_track_back_batch: the check is off (vio_frame_set_flow_back)");
    return track_run(h, "vio_frame_track_back_batch", count, items, next_pts, info, back);
}

vio_status vio_frame_set_flow_back(vio_frame *h, const vio_flow_back_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = kf::flow_check_back(h->err, "vio_frame_set_flow_back", cfg, h->fcfg.levels);
    if (st != VIO_OK) return st;
    h->bcfg = cfg ? *cfg : kf::FLOW_BACK_DEFAULTS;
    return VIO_OK;
}

vio_status vio_frame_set_reject_with_f(vio_frame *h, int32_t enabled) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (enabled != 0 && enabled != 1) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_reject_with_f: enabled 0 or 1");
    h->reject_f = enabled;
    return VIO_OK;
}

vio_status vio_frame_read_back_info(const vio_frame *h, int32_t slot, int32_t *n_checked, int32_t *n_back_lost, int32_t *n_back_far) {
    if (!h || !FrameTable::slot_ok(slot)) return VIO_ERR_BAD_ARG;
    if (n_checked) *n_checked = h->back_info[slot][0];
    if (n_back_lost) *n_back_lost = h->back_info[slot][1];
    if (n_back_far) *n_back_far = h->back_info[slot][2];
    return VIO_OK;
}

vio_status vio_frame_set_prediction_batch(vio_frame *h, int32_t count, const vio_frame_prediction_item *items) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || count > MAX_ITEMS || (count > 0 && !items))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_prediction_batch: count outside [0, %d] or a NULL array", MAX_ITEMS);
    // every argument of every item first: nothing is stored on an error
    std::vector<uint8_t> seen((size_t)VIO_FRAME_MAX_SLOTS, 0);
    for (int i = 0; i < count; ++i) {
        const vio_frame_prediction_item &it = items[i];
        if (!FrameTable::slot_ok(it.slot)) return fail_check(h, "vio_frame_set_prediction_batch", FRAME_BAD_SLOT, i, it.slot);
        if (seen[(size_t)it.slot]) return fail_check(h, "vio_frame_set_prediction_batch", FRAME_TWICE, i, it.slot);
        seen[(size_t)it.slot] = 1;
        if (it.n < 0 || it.n > VIO_FRAME_MAX_TRACK_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_prediction_batch: item %d: n must be in [0, %d]", i, VIO_FRAME_MAX_TRACK_POINTS);
        if (it.n > 0 && (!it.ids || !it.pixels)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_prediction_batch: item %d: ids and pixels are required", i);
        for (int k = 0; k < 2 * it.n; ++k)
            if (!std::isfinite(it.pixels[k]))
                return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_prediction_batch: item %d: pixel %d is not finite", i, k / 2);
    }
    for (int i = 0; i < count; ++i) {
        const vio_frame_prediction_item &it = items[i];
        FramePrediction &p = h->pred[(size_t)it.slot];
        std::vector<long long> ids((size_t)it.n);
        for (int k = 0; k < it.n; ++k) ids[(size_t)k] = (long long)it.ids[k];
        p.ids.resize((size_t)it.n); p.px.resize(2 * (size_t)it.n);
        const int32_t m = front_guess_normalise(ids.data(), it.pixels, it.n, p.ids.data(), p.px.data());
        p.ids.resize((size_t)m); p.px.resize(2 * (size_t)m);
        p.pending = true; p.n_listed = it.n;
    }
    return VIO_OK;
}

vio_status vio_frame_clear_prediction(vio_frame *h, int32_t slot) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!FrameTable::slot_ok(slot)) return fail_check(h, "vio_frame_clear_prediction", FRAME_BAD_SLOT, 0, slot);
    h->pred[(size_t)slot].drop();
    return VIO_OK;
}

vio_status vio_frame_set_prediction_fallback(vio_frame *h, int32_t min_tracked) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (min_tracked < 0 || min_tracked > VIO_FRAME_MAX_TRACK_POINTS)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_set_prediction_fallback: min_tracked in [0, %d]", VIO_FRAME_MAX_TRACK_POINTS);
    h->min_tracked = min_tracked;
    return VIO_OK;
}

vio_status vio_frame_read_predict_info(const vio_frame *h, int32_t slot, int32_t *n_listed, int32_t *n_guessed, int32_t *n_ok_guessed,
                                       int32_t *fell_back) {
    if (!h || !FrameTable::slot_ok(slot)) return VIO_ERR_BAD_ARG;
    if (n_listed) *n_listed = h->pred_info[slot][0];
    if (n_guessed) *n_guessed = h->pred_info[slot][1];
    if (n_ok_guessed) *n_ok_guessed = h->pred_info[slot][2];
    if (fell_back) *fell_back = h->pred_info[slot][3];
    return VIO_OK;
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
    kd::DetTotals T;
    vio_status st;
    for (int i = 0; i < count; ++i) {
        const vio_frame_detect_item &it = items[i];
        if ((st = kd::det_check_counts(h->err, "vio_frame_detect_batch: ", i, it.n_tracked, it.max_total)) != VIO_OK) return st;
        const FrameCheck ck = h->tab.check_detect(it.slot);
        if (ck != FRAME_OK) return fail_check(h, "vio_frame_detect_batch", ck, i, it.slot);
        if ((it.n_tracked > 0 && (!it.tracked || !it.track_cnt || !it.keep_order)) || (it.max_total > 0 && !it.new_pts))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_detect_batch: item %d: tracked, track_cnt, keep_order, new_pts are required where they have rows", i);
        const FrameSlot &s = h->tab.slots[it.slot];
        kd::DetItemD &d = its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        if ((st = kd::det_check_tracked(h->err, "vio_frame_detect_batch: ", i, it.tracked, it.n_tracked, s.width, s.height, &d.active)) != VIO_OK) return st;
        det_item_of(h, d, T, s, it.n_tracked, it.max_total);
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const kd::DetSizes S = kd::det_sizes(count, T.n_trk, T.n_new);
    if ((st = h->dtab.ensure(h->err, S.b_tab)) != VIO_OK || (st = h->dout.ensure(h->err, S.b_out)) != VIO_OK ||
        (st = h->r.ensure(h->err, sizeof(double) * (size_t)T.n_r)) != VIO_OK ||
        (st = h->cand.ensure(h->err, sizeof(uint32_t) * (size_t)T.n_cand)) != VIO_OK || (st = h->scratch.ensure(h->err, S.b_scratch)) != VIO_OK)
        return st;
    kd::det_fill_table(h->dtab.h, S, count, items, its.data());
    const kd::DetArgs a = kd::det_args(h->dcfg, count, S, h->dtab.d, h->dout.d, h->scratch.d, h->r.d, h->cand.d);
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->dtab.d, h->dtab.h, S.b_tab, hipMemcpyHostToDevice, q) != hipSuccess || hipMemsetAsync(h->dout.d, 0, S.b_res, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[6], q);
    kd::det_launch(a, q, T.n_trk > 0, T.max_tiles > 0, T.max_tiles, nullptr);
    (void)hipEventRecord(h->q.ev[7], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    if (hipMemcpyAsync(h->dout.h, h->dout.d, S.b_out, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    h->counters[2] += S.b_tab; h->counters[3] += S.b_out;
    const vio_status ret = kd::det_unpack(h->err, h->dout.h, S, count, items, its.data(), results);
    h->timing[6] = elapsed_ms(h->q.ev[6], h->q.ev[7]);
    h->timing[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ret;
}

vio_status vio_frame_set_camera(vio_frame *h, const vio_reject_camera *cam, const vio_reject_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_reject_config c = cfg ? *cfg : kr::REJ_DEFAULTS;
    vio_status st;
    if ((st = kr::rej_check_camera(h->err, "vio_frame_set_camera", cam)) != VIO_OK || (st = kr::rej_check_config(h->err, "vio_frame_set_camera", &c)) != VIO_OK)
        return st;
    kr::rej_set_camera(*cam, h->camera, h->cam);
    h->rcfg = c;
    h->have_camera = true;
    h->cams.set_handle_camera(h->camera);
    return VIO_OK;
}

vio_status vio_frame_set_slot_camera(vio_frame *h, int32_t slot, const vio_camera_model *cam) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    return cam ? h->cams.set(h->err, slot, cam) : h->cams.clear(h->err, slot);
}

vio_status vio_frame_get_slot_camera(const vio_frame *h, int32_t slot, int32_t *is_set, vio_camera_model *cam) {
    if (!h || !FrameCameras::slot_ok(slot)) return VIO_ERR_BAD_ARG;
    if (is_set) *is_set = h->cams.own[slot];
    if (cam && h->cams.own[slot]) *cam = h->cams.model[slot];
    return VIO_OK;
}

vio_status vio_frame_set_reject_config(vio_frame *h, const vio_reject_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    const vio_status st = kr::rej_check_config(h->err, "vio_frame_set_reject_config", cfg);
    if (st != VIO_OK) return st;
    h->rcfg = *cfg;
    return VIO_OK;
}

vio_status vio_frame_read_lift_info(const vio_frame *h, int32_t slot, int32_t *n_clamped, int32_t *n_bad) {
    if (!h || !FrameCameras::slot_ok(slot)) return VIO_ERR_BAD_ARG;
    if (n_clamped) *n_clamped = h->cams.n_clamped[slot];
    if (n_bad) *n_bad = h->cams.n_bad[slot];
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
    if (!h->have_camera && h->cams.n_own == 0) return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_read_batch: no camera set");
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
    // the cameras: every listed slot needs one; a call without a slot camera among them is the handle's camera through the PINHOLE kernels
    const FrameCamPath path = h->cams.path(count, sl.data(), &bad);
    if (path == FRAME_CAM_MISSING)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_frame_read_batch: item %d: slot %d has no camera of its own, and the handle has none", bad, sl[(size_t)bad]);
    return path == FRAME_CAM_TABLE ? read_run<true>(h, count, items, publish, results, t0, sl, ww, hh, tt, push)
                                   : read_run<false>(h, count, items, publish, results, t0, sl, ww, hh, tt, push);
}

}  // extern "C"

namespace {

// The read of `count` checked items.  CAMS false: the handle's camera through the kr kernels and the joining kernels at file scope,
// the launches of include/vio_frame_read.h as they always were.  CAMS true: the camera table through the kq kernels and the joining
// kernels of namespace fq, a slot in every descriptor (include/vio_frame_camera.h).
template <bool CAMS> vio_status read_run(vio_frame *h, int32_t count, const vio_frame_read_item *items, int32_t publish, vio_frame_read_result *results,
                                         std::chrono::steady_clock::time_point t0, const std::vector<int32_t> &sl, const std::vector<int32_t> &ww,
                                         const std::vector<int32_t> &hh, const std::vector<double> &tt, const std::vector<vio_frame_push_item> &push) {
    using P = ReadPath<CAMS>;
    using RejPair = typename P::RejPair;
    using LiftItem = typename P::LiftItem;
    using RejRes = typename P::RejRes;
    using FrontItem = typename P::Item;
    using FrontRes = typename P::Res;
    using FrontArgs = typename P::Args;
    const size_t B = (size_t)count;
    vio_status st;
    // what the host knows of each slot before the roll
    std::vector<FrameSlot> was(B);
    int64_t total = 0, n_r = 0, n_cand = 0;
    int rows_cap = std::max(h->max_cnt, 1);
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
    const size_t o_pair = o_det + align256(sizeof(kd::DetItemD) * B), o_lift = o_pair + align256(sizeof(RejPair) * B);
    // ... and with them the predictions of the listed slots that have points to track (include/vio_frame_predict.h): an item table,
    // the ids, the pixels.  Without one the tables, the work space and the results are laid out as they always were.
    using GuessItem = typename P::GuessItem;
    using GuessRes = typename P::GuessRes;
    std::vector<uint8_t> guessed(B, 0);
    size_t g_rows = 0;
    for (size_t i = 0; i < B; ++i) {
        guessed[i] = h->pred[(size_t)sl[i]].pending && was[i].n_pts > 0;
        if (guessed[i]) g_rows += h->pred[(size_t)sl[i]].ids.size();
    }
    const bool guess = std::find(guessed.begin(), guessed.end(), 1) != guessed.end(), again = guess && h->min_tracked > 0;
    const size_t o_gitem = o_lift + align256(sizeof(LiftItem) * B), o_gids = o_gitem + (guess ? align256(sizeof(GuessItem) * B) : 0);
    const size_t o_gpx = o_gids + (guess ? align256(sizeof(long long) * g_rows) : 0);
    const size_t b_tab = o_gpx + (guess ? align256(sizeof(float) * 2 * g_rows) : 0);
    // the device work space, every per-point array at FRONT_CAP rows per item
    size_t b_work = 0;
    const auto carve = [&](size_t bytes) { const size_t at = b_work; b_work += align256(bytes); return at; };
    const size_t rowsN = B * CAP;
    const size_t w_dres = carve(sizeof(kd::DetRes) * B), w_rres = carve(sizeof(RejRes) * B), b_zero = b_work;
    const size_t w_fpts = carve(sizeof(kf::FlowPt) * rowsN), w_fout = carve(sizeof(kf::FlowOut) * rowsN);
    const size_t w_rstage = carve(sizeof(float) * 4 * rowsN), w_corr = carve(sizeof(double) * 4 * rowsN);
    const size_t w_flag = carve(sizeof(int32_t) * rowsN), w_rmask = carve(rowsN);
    const size_t w_fa = carve(sizeof(float) * 2 * rowsN), w_ida = carve(sizeof(long long) * rowsN), w_cnta = carve(sizeof(int32_t) * rowsN);
    const size_t w_fb = carve(sizeof(float) * 2 * rowsN), w_idb = carve(sizeof(long long) * rowsN), w_cntb = carve(sizeof(int32_t) * rowsN);
    const size_t w_trk = carve(sizeof(kd::DetTrk) * rowsN), w_tkey = carve(sizeof(unsigned long long) * rowsN);
    const size_t w_kxy = carve(sizeof(int32_t) * 2 * rowsN), w_keep = carve(sizeof(int32_t) * rowsN), w_new = carve(sizeof(float) * 2 * rowsN);
    const size_t w_lstage = carve(sizeof(float) * 4 * rowsN), w_lids = carve(sizeof(long long) * 2 * rowsN);
    const size_t w_un = carve(sizeof(float) * 2 * rowsN), w_vel = carve(sizeof(float) * 2 * rowsN), w_cntm = carve(sizeof(int32_t) * rowsN);
    const size_t w_lflag = CAMS ? carve(rowsN) : 0;        // k_reject_lift's flag byte per point
    const size_t w_fpts2 = again ? carve(sizeof(kf::FlowPt) * rowsN) : 0, w_fout2 = again ? carve(sizeof(kf::FlowOut) * rowsN) : 0;    // the fallback's pass
    const bool check = h->bcfg.enabled != 0;
    const size_t row_bytes = (36 * (size_t)rows_cap + 7) & ~(size_t)7;
    const size_t b_res = align256(sizeof(FrontRes) * B), o_gres = align256(b_res + row_bytes * B);
    const size_t b_out = guess ? o_gres + sizeof(GuessRes) * B : b_res + row_bytes * B;       // (GuessRes per item behind the rows)
    for (size_t i = 0; i < B; ++i) {
        n_r += (int64_t)ww[i] * hh[i];
        n_cand += (int64_t)std::max(ww[i] - 2, 0) * std::max(hh[i] - 2, 0);
    }
    if ((st = ensure_points(h)) != VIO_OK || (st = h->rtab.ensure(h->err, b_tab)) != VIO_OK || (st = h->rwork.ensure(h->err, b_work)) != VIO_OK ||
        (st = h->rout.ensure(h->err, b_out)) != VIO_OK || (CAMS && (st = ensure_cameras(h)) != VIO_OK) ||
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
    RejPair *rp = (RejPair *)(h->rtab.h + o_pair);
    LiftItem *li = (LiftItem *)(h->rtab.h + o_lift);
    kd::DetTotals T;
    int64_t flow_off = 0;
    for (size_t i = 0; i < B; ++i) {
        const FrameSlot &s = h->tab.slots[sl[i]];
        const SlotPts p = slot_pts(h, sl[i]);
        FrontItem &f = fr[i];
        f.cur_pts = p.cur; f.ids = p.ids; f.cnt = p.cnt; f.prev_un_ids = p.prev_ids; f.prev_un_pts = p.prev_pts; f.next_id = p.next_id;
        f.n = s.n_frames == 2 ? was[i].n_pts : 0; f.m = was[i].n_prev_un;
        f.w = s.width; f.h = s.height; f.flow_off = (int32_t)flow_off;
        flow_off += f.n;
        if (f.n > 0) {
            FrameLayout Y;
            frame_layout(s.width, s.height, L, Y);
            flow_item_of(h, fi[i], Y, s.prev, s.next);
        }
        kd::DetItemD &d = di[i];
        d.active = 1;
        det_item_of(h, d, T, s, 0, h->max_cnt);             // (n_tracked is k_front_after_reject's to write)
        d.trk = (int32_t)(i * CAP); d.newp = (int32_t)(i * CAP);    // (every per-point array has CAP rows per item here)
        RejPair &r = rp[i];
        r.pair = was[i].n_read; r.finite = 1;               // (n and active are k_front_filter's to write)
        r.o_pts = (int64_t)(i * 4 * CAP); r.o_corr = (int64_t)(i * 4 * CAP); r.o_pt = (int64_t)(i * CAP);
        LiftItem &u = li[i];
        u.active = 1;                                       // (n and m are k_front_merge's to write)
        u.o_pts = (int64_t)(i * 4 * CAP); u.o_prev = (int64_t)(i * 4 * CAP + 2 * CAP);
        u.o_ids = (int64_t)(i * 2 * CAP); u.o_out = (int64_t)(i * CAP);
        u.dt = was[i].n_prev_un > 0 ? tt[i] - was[i].time : 1.0;
        if constexpr (CAMS) { r.slot = sl[i]; u.slot = sl[i]; }
    }
    total = flow_off;
    // the listed slots' predictions are consumed here, whatever becomes of them: the slots have rolled
    std::vector<int32_t> n_listed(B, 0);
    size_t g_at = 0;
    for (size_t i = 0; i < B; ++i) {
        FramePrediction &p = h->pred[(size_t)sl[i]];
        if (p.pending) n_listed[i] = p.n_listed;
        if (guessed[i]) {
            GuessItem &g = ((GuessItem *)(h->rtab.h + o_gitem))[i];
            const size_t m = p.ids.size();
            g.off = (int32_t)g_at; g.m = (int32_t)m; g.guessed = 1;
            if (m > 0) {
                std::memcpy(h->rtab.h + o_gids + sizeof(long long) * g_at, p.ids.data(), sizeof(long long) * m);
                std::memcpy(h->rtab.h + o_gpx + sizeof(float) * 2 * g_at, p.px.data(), sizeof(float) * 2 * m);
            }
            g_at += m;
        }
        p.drop();
    }
    char *W = h->rwork.d;
    FrontArgs a;
    std::memset(&a, 0, sizeof(a));
    a.items = (const FrontItem *)h->rtab.d;
    a.fpts = (kf::FlowPt *)(W + w_fpts); a.fout = (const kf::FlowOut *)(W + w_fout);
    a.pairs = (RejPair *)(h->rtab.d + o_pair);
    a.rstage = (float *)(W + w_rstage); a.rmask = (const uint8_t *)(W + w_rmask); a.rres = (const RejRes *)(W + w_rres);
    a.fa = (float *)(W + w_fa); a.ida = (long long *)(W + w_ida); a.cnta = (int32_t *)(W + w_cnta);
    a.fb = (float *)(W + w_fb); a.idb = (long long *)(W + w_idb); a.cntb = (int32_t *)(W + w_cntb);
    a.ditems = (kd::DetItemD *)(h->rtab.d + o_det); a.dtrk = (kd::DetTrk *)(W + w_trk); a.dres = (const kd::DetRes *)(W + w_dres);
    a.keep_order = (const int32_t *)(W + w_keep); a.new_pts = (const float *)(W + w_new);
    a.litems = (LiftItem *)(h->rtab.d + o_lift);
    a.lstage = (float *)(W + w_lstage); a.lids = (long long *)(W + w_lids);
    a.un = (const float *)(W + w_un); a.vel = (const float *)(W + w_vel); a.cntm = (int32_t *)(W + w_cntm);
    a.res = (FrontRes *)h->rout.d; a.rows = h->rout.d + b_res; a.row_bytes = (int64_t)row_bytes; a.rows_cap = rows_cap;
    a.count = count; a.publish = publish; a.border = h->border;
    a.reject = h->reject_f; a.flow_back = check ? 1 : 0;
    if constexpr (CAMS) a.lflags = (const uint8_t *)(W + w_lflag);
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->rtab.d, h->rtab.h, b_tab, hipMemcpyHostToDevice, q) != hipSuccess || hipMemsetAsync(W, 0, b_zero, q) != hipSuccess)
        return fail_synced(h, "upload failed");
    if constexpr (CAMS) {                                    // the camera table, if a slot changed: on the stream, ahead of the kernels
        if (h->cams.take_dirty()) {
            std::memcpy(h->camtab.h, h->cams.table, sizeof(h->cams.table));
            if (hipMemcpyAsync(h->camtab.d, h->camtab.h, sizeof(h->cams.table), hipMemcpyHostToDevice, q) != hipSuccess) {
                h->cams.dirty = true;
                return fail_synced(h, "upload failed");
            }
            h->counters[2] += sizeof(h->cams.table);
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    const dim3 per_item((unsigned)count), fnt(FNT);
    const auto front = [&](auto kernel) { hipLaunchKernelGGL(kernel, per_item, fnt, 0, q, a); };
    // 2 - 4. the slot's points into the new frame, and those that stay
    if (guess) {
        // a listed slot has a prediction (include/vio_frame_predict.h): the guesses into k_front_begin's rows, the tracker; the count
        // of each item's status-0 rows and the decision; with a fallback armed the tracker again over the second list (its rows are
        // NaN for every item that keeps its guessed pass), and the rows of the items that fell back over the first pass's
        typename P::GuessArgs g;
        std::memset(&g, 0, sizeof(g));
        g.items = a.items; g.gitems = (const GuessItem *)(h->rtab.d + o_gitem);
        g.gids = (const long long *)(h->rtab.d + o_gids); g.gpx = (const float *)(h->rtab.d + o_gpx);
        g.fpts = a.fpts; g.fpts2 = again ? (kf::FlowPt *)(W + w_fpts2) : nullptr;
        g.fout = (kf::FlowOut *)(W + w_fout); g.fout2 = again ? (const kf::FlowOut *)(W + w_fout2) : nullptr;
        g.gres = (GuessRes *)(h->rout.d + o_gres);
        g.g_rows = (int32_t)g_rows; g.min_tracked = h->min_tracked;
        const kf::FlowItemD *fid = (const kf::FlowItemD *)(h->rtab.d + o_flow);
        const auto track = [&](const kf::FlowPt *pts, kf::FlowOut *out) {
            if (check) kf::flow_launch_track_back(q, kf::flow_back_args(fid, pts, out, nullptr, (size_t)total, L, h->fcfg, h->bcfg), h->fcfg.inverse != 0);
            else kf::flow_launch_track(q, kf::flow_args(fid, pts, out, (size_t)total, L, h->fcfg), h->fcfg.inverse != 0);
        };
        const auto joined = [&](auto kernel) { hipLaunchKernelGGL(kernel, per_item, fnt, 0, q, g); };
        front(P::begin);
        joined(P::guess);
        track(g.fpts, g.fout);
        joined(P::fallback);
        if (again) {
            track(g.fpts2, (kf::FlowOut *)(W + w_fout2));
            joined(P::take);
        }
    } else if (total > 0) {
        front(P::begin);
        const kf::FlowItemD *fid = (const kf::FlowItemD *)(h->rtab.d + o_flow);
        if (check)
            kf::flow_launch_track_back(q, kf::flow_back_args(fid, a.fpts, (kf::FlowOut *)(W + w_fout), nullptr, (size_t)total, L,
                                                             h->fcfg, h->bcfg), h->fcfg.inverse != 0);
        else
            kf::flow_launch_track(q, kf::flow_args(fid, a.fpts, (kf::FlowOut *)(W + w_fout), (size_t)total, L, h->fcfg), h->fcfg.inverse != 0);
    }
    front(P::filter);
    (void)hipEventRecord(h->rev[0], q);
    if (publish && !h->reject_f) {
        // no rejectWithF: the reject stage is an unpublished read's, and k_front_after_reject, which keeps every row of an inactive pair
        // and makes the detection's table, runs in the detection stage
        (void)hipEventRecord(h->rev[1], q);
        front(P::after_reject);
    } else if (publish) {
        // 5, 6. rejectWithF and what it keeps
        typename P::RansacArgs ra;
        if constexpr (CAMS) {
            std::memset(&ra, 0, sizeof(ra));
            ra.cams = h->camtab.d;
            ra.focal = h->rcfg.focal_length; ra.thr = h->rcfg.f_threshold * h->rcfg.f_threshold;
            ra.seed = h->rcfg.seed; ra.hyps = h->rcfg.ransac_hypotheses;
        } else {
            ra = kr::rej_ransac_args(h->cam, h->camera, h->rcfg);
        }
        ra.pairs = a.pairs; ra.pts = a.rstage;
        ra.corr = (double *)(W + w_corr); ra.flag = (int32_t *)(W + w_flag); ra.mask = (uint8_t *)(W + w_rmask); ra.res = (RejRes *)(W + w_rres);
        if (total > 0) hipLaunchKernelGGL(P::ransac, per_item, dim3(kr::NT), 0, q, ra);
        front(P::after_reject);
        (void)hipEventRecord(h->rev[1], q);
    }
    if (publish) {
        // 7. setMask and the detection
        kd::DetArgs da = kd::det_args(h->dcfg, count);
        da.items = a.ditems; da.trk = a.dtrk;
        da.r = h->r.d; da.cand = h->cand.d;
        da.tkey = (unsigned long long *)(W + w_tkey); da.kept_xy = (int32_t *)(W + w_kxy);
        da.res = (kd::DetRes *)(W + w_dres);
        da.keep_order = (int32_t *)(W + w_keep); da.new_pts = (float *)(W + w_new);
        kd::det_launch(da, q, total > 0, true, T.max_tiles, nullptr);
    } else {
        (void)hipEventRecord(h->rev[1], q);
    }
    (void)hipEventRecord(h->rev[2], q);
    // 8 - 10. the merged point set, undistortedPoints, updateID and the roll
    front(P::merge);
    typename P::LiftArgs la;
    std::memset(&la, 0, sizeof(la));
    la.items = a.litems; la.pts = a.lstage; la.ids = a.lids;
    la.un = (float *)(W + w_un); la.vel = (float *)(W + w_vel); la.lifted = nullptr;
    la.bare = 0; la.count = count;
    if constexpr (CAMS) {
        la.cams = h->camtab.d; la.flags = (uint8_t *)(W + w_lflag);
        kq::rej_launch_lift(q, la, rows_cap);
    } else {
        la.cam = h->cam;
        kr::rej_launch_lift(q, la, rows_cap);
    }
    front(P::finish);
    (void)hipEventRecord(h->rev[3], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    // 11. what is published comes down, and the call waits
    if (hipMemcpyAsync(h->rout.h, h->rout.d, b_out, hipMemcpyDeviceToHost, q) != hipSuccess) return fail_synced(h, "read-back failed");
    (void)hipEventRecord(h->rev[4], q);
    if (hipStreamSynchronize(q) != hipSuccess) return fail_synced(h, "kernel or read-back failed");
    h->counters[2] += b_tab; h->counters[3] += b_out;
    const FrontRes *res = (const FrontRes *)h->rout.h;
    vio_status ret = VIO_OK;
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
        int32_t n_clamped = 0, n_bad = 0;
        if constexpr (CAMS) { n_clamped = std::max(r.n_clamped, 0); n_bad = std::max(r.n_bad, 0); }
        const bool bad_lift = n_bad > 0 || r.reject_status == VIO_ERR_NOT_FINITE;       // (in undistortedPoints, in rejectWithF)
        if (bad_lift && ret == VIO_OK) ret = fail(h->err, VIO_ERR_NOT_FINITE, "item %d: slot %d: a lift is not finite", (int)i, it.slot);
        h->cams.lift_info_set(it.slot, n_clamped, n_bad);
        h->back_info[it.slot][0] = front_clamp(r.n_checked, 0, FRONT_CAP); h->back_info[it.slot][1] = front_clamp(r.n_back_lost, 0, FRONT_CAP);
        h->back_info[it.slot][2] = front_clamp(r.n_back_far, 0, FRONT_CAP);
        int32_t *pinfo = h->pred_info[it.slot];
        pinfo[0] = n_listed[i]; pinfo[1] = pinfo[2] = pinfo[3] = 0;
        if (guess) {
            const GuessRes &gr = ((const GuessRes *)(h->rout.h + o_gres))[i];
            pinfo[1] = front_clamp(gr.n_guessed, 0, FRONT_CAP); pinfo[2] = front_clamp(gr.n_ok_guessed, 0, FRONT_CAP); pinfo[3] = gr.fell_back != 0;
        }
        o.status = bad_lift ? VIO_ERR_NOT_FINITE : VIO_OK; o.n = (int32_t)n; o.n_new = front_clamp(r.n_new, 0, (int32_t)n);
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
    return ret;
}

}  // namespace
