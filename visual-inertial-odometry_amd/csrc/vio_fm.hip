// vio_fm.hip — libvio_fm_hip.so: the FeatureManager of many streams in one call, each stream's track list resident on the device
// (include/vio_fm.h).
// Contraction is off (vio_fm_math.h): the parallax term and the depth shift are evaluated as written.  No floating-point atomics.
// The kernels, described where they are, are in vio_fm_body.inc, (include/vio_fm_stream.h's two) vio_fm_stream_body.inc and
// (include/vio_fm_outlier.h's one) vio_fm_outlier_body.inc and (include/vio_fm_predict.h's one) vio_fm_predict_body.inc; the triangulation is vio_triangulate_body.h, a function around the
// text (vio_triangulate_body.inc) that k_triangulate of libvio_hip includes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_fm.h"
#include "../../include/vio_fm_stream.h"
#include "../../include/vio_fm_outlier.h"
#include "../../include/vio_fm_predict.h"
#include "vio_companion.h"
#include "vio_device_math.h"
#include "vio_types.h"

#include "vio_triangulate_body.h"        // (before vio_fm_math.h's pragma: compiled as vio_kernels.hip compiles it)

#include "vio_fm_math.h"

#include "vio_fm_body.inc"
#include "vio_fm_stream_body.inc"
#include "vio_fm_outlier_math.h"
#include "vio_fm_outlier_body.inc"
#include "vio_fm_predict_math.h"
#include "vio_fm_predict_body.inc"

static_assert(FM_MAX_TRACKS == VIO_FM_MAX_TRACKS && FM_MAX_OBS == VIO_FM_MAX_OBS && FM_MAX_POINTS == VIO_FM_MAX_POINTS &&
              FM_BACK_SHIFT_DEPTH == VIO_FM_BACK_SHIFT_DEPTH && FM_BACK == VIO_FM_BACK && FM_FRONT == VIO_FM_FRONT &&
              FM_MAX_OBS == VIO_NF && FM_WINDOW == VIO_NF - 1, "vio_fm_math.h restates include/vio_fm.h");

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct FmSlot {
    char *d = nullptr;                                   // the table, allocated at the slot's first use
    int32_t n_tracks = 0, n_landmarks = 0, n_observations = 0;      // as the last call's read-back left them
};

struct vio_fm {
    int device = 0;
    ErrText err = {0};
    vio_fm_config cfg = {VIO_FM_DEFAULT_INIT_DEPTH, VIO_FM_DEFAULT_MIN_PARALLAX};
    FmSlot slots[VIO_FM_MAX_SLOTS];
    Twin<char> up;                                       // item descriptors | payloads
    Twin<char> out;                                      // results | the items' arrays
    Twin<char> img;                                      // one table, for vio_fm_tracks_set / _get
    StreamEvents<4> q;                                   // events: upload, kernel, read-back start; end
    double timing[4] = {NAN, NAN, NAN, NAN};
    std::vector<FmItemD> its;
    std::vector<int64_t> scratch_ids;
    std::vector<int32_t> scratch_perm;                   // vio_fm_remove_batch: every item's sort permutation
};

namespace {

typedef std::chrono::steady_clock::time_point Tick;

bool all_finite(const double *v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// every item's slot in range and listed once; the descriptors start from the slots' mirrors
template <class Item> vio_status begin_call(vio_fm *h, const char *what, int32_t count, const Item *items, const vio_fm_result *results) {
    h->err[0] = 0;
    if (count < 0 || count > VIO_FM_MAX_SLOTS || (count > 0 && (!items || !results)))
        return fail(h->err, VIO_ERR_BAD_ARG, "%s: count outside [0, %d] or a NULL array", what, VIO_FM_MAX_SLOTS);
    bool seen[VIO_FM_MAX_SLOTS] = {false};
    h->its.assign((size_t)count, FmItemD());
    for (int i = 0; i < count; ++i) {
        const int s = items[i].slot;
        if (s < 0 || s >= VIO_FM_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d outside [0, %d)", what, i, s, VIO_FM_MAX_SLOTS);
        if (seen[s]) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d is listed twice", what, i, s);
        seen[s] = true;
        FmItemD &d = h->its[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        d.n_tracks = h->slots[s].n_tracks;
    }
    return VIO_OK;
}

vio_status slot_table(vio_fm *h, int s) {
    if (h->slots[s].d) return VIO_OK;
    return hip_ck(h->err, hipMalloc((void **)&h->slots[s].d, FM_TAB_BYTES), "hipMalloc");
}

typedef void (*FmKernel)(FmArgs);

// The part every batched call shares once its arguments are checked and its descriptors (a, b, c, o_in, o_out) are filled: `pack`
// writes the payloads into the pinned upload, one launch of `kern`, one read-back, one wait; the results and the mirrors; `unpack`
// copies the items' arrays out of the pinned read-back.
template <class Item, class Pack, class Unpack>
vio_status run_call(vio_fm *h, Tick t0, int32_t count, const Item *items, vio_fm_result *results, size_t b_in, size_t b_out, FmKernel kern,
                    int threads, Pack pack, Unpack unpack) {
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    for (int i = 0; i < count; ++i) {
        if ((st = slot_table(h, items[i].slot)) != VIO_OK) return st;
        h->its[(size_t)i].tab = h->slots[items[i].slot].d;
    }
    const size_t b_items = align256(sizeof(FmItemD) * (size_t)count), b_res = align256(sizeof(vio_fm_result) * (size_t)count);
    if ((st = h->up.ensure(h->err, b_items + b_in)) != VIO_OK || (st = h->out.ensure(h->err, b_res + b_out)) != VIO_OK) return st;
    std::memcpy(h->up.h, h->its.data(), sizeof(FmItemD) * (size_t)count);
    pack(h->up.h + b_items);
    FmArgs a;
    a.items = (const FmItemD *)h->up.d;
    a.in = h->up.d + b_items;
    a.res = (vio_fm_result *)h->out.d;
    a.out = h->out.d + b_res;
    a.init_depth = h->cfg.init_depth;
    a.min_parallax = h->cfg.min_parallax;
    const Tick t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->up.d, h->up.h, b_items + b_in, hipMemcpyHostToDevice, q) != hipSuccess) return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    hipLaunchKernelGGL(kern, dim3((unsigned)count), dim3((unsigned)threads), 0, q, a);
    (void)hipEventRecord(h->q.ev[2], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, b_res + b_out, hipMemcpyDeviceToHost, q) != hipSuccess) return fail_synced(h, "read-back failed");
    (void)hipEventRecord(h->q.ev[3], q);
    if (hipStreamSynchronize(q) != hipSuccess) return fail_synced(h, "kernel or read-back failed");
    std::memcpy(results, h->out.h, sizeof(vio_fm_result) * (size_t)count);
    for (int i = 0; i < count; ++i) {                    // the mirrors, held to what a table can be
        FmSlot &s = h->slots[items[i].slot];
        s.n_tracks = fm_clamp(results[i].n_tracks, 0, FM_MAX_TRACKS);
        s.n_landmarks = fm_clamp(results[i].n_landmarks, 0, s.n_tracks);
        s.n_observations = fm_clamp(results[i].n_observations, 0, s.n_landmarks * (FM_MAX_OBS - 1));
    }
    unpack(h->out.h + b_res);
    const Tick t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    h->timing[2] = elapsed_ms(h->q.ev[2], h->q.ev[3]);
    h->timing[3] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return VIO_OK;
}

void free_slots(vio_fm *h) {
    for (FmSlot &s : h->slots)
        if (s.d) { (void)hipFree(s.d); s.d = nullptr; }
}

}  // namespace

extern "C" {

int32_t vio_fm_version(void) { return VIO_FM_VERSION; }

const char *vio_fm_last_error(const vio_fm *h) { return h ? h->err : "NULL handle"; }

vio_status vio_fm_create(int32_t device, void *stream, vio_fm **out) { return create_handle(device, stream, out, vio_fm_destroy); }

void vio_fm_destroy(vio_fm *h) { destroy_handle(h, free_slots); }

vio_status vio_fm_set_config(vio_fm *h, const vio_fm_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg || !std::isfinite(cfg->init_depth) || !(cfg->init_depth > 0) || !std::isfinite(cfg->min_parallax) || !(cfg->min_parallax >= 0))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_set_config: init_depth must be finite and > 0, min_parallax finite and >= 0");
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_fm_reset(vio_fm *h, int32_t slot) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_FM_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_reset: slot %d outside [0, %d)", slot, VIO_FM_MAX_SLOTS);
    FmSlot &s = h->slots[slot];
    s.n_tracks = 0; s.n_landmarks = 0; s.n_observations = 0;         // (every kernel reads the rows the mirror counts, no more)
    return VIO_OK;
}

vio_status vio_fm_counts(const vio_fm *h, int32_t slot, int32_t *n_tracks, int32_t *n_landmarks, int32_t *n_observations) {
    if (!h || slot < 0 || slot >= VIO_FM_MAX_SLOTS) return VIO_ERR_BAD_ARG;
    const FmSlot &s = h->slots[slot];
    if (n_tracks) *n_tracks = s.n_tracks;
    if (n_landmarks) *n_landmarks = s.n_landmarks;
    if (n_observations) *n_observations = s.n_observations;
    return VIO_OK;
}

vio_status vio_fm_timing(const vio_fm *h, double *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_fm_add_batch(vio_fm *h, int32_t count, const vio_fm_add_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_add_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    size_t b_in = 0;
    for (int i = 0; i < count; ++i) {
        const vio_fm_add_item &it = items[i];
        if (it.frame_count < 0 || it.frame_count > FM_WINDOW || it.n < 0 || it.n > VIO_FM_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_add_batch: item %d: frame_count must be in [0, %d] and n in [0, %d]", i, FM_WINDOW, VIO_FM_MAX_POINTS);
        if (it.n > 0 && (!it.ids || !it.pts)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_add_batch: item %d: ids and pts are required", i);
        if (!all_finite(it.pts, 2 * (int64_t)it.n)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_add_batch: item %d: a point is not finite", i);
        h->scratch_ids.assign(it.ids, it.ids + it.n);
        std::sort(h->scratch_ids.begin(), h->scratch_ids.end());
        if (std::adjacent_find(h->scratch_ids.begin(), h->scratch_ids.end()) != h->scratch_ids.end())
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_add_batch: item %d: an id is listed twice", i);
        FmItemD &d = h->its[(size_t)i];
        d.a = it.frame_count; d.b = it.n;
        d.o_in = (int64_t)b_in;
        b_in += align256(24 * (size_t)it.n);
    }
    return run_call(h, t0, count, items, results, b_in, 0, k_fm_add, FM_NT,
                    [&](char *in) {
                        for (int i = 0; i < count; ++i) {
                            char *p = in + h->its[(size_t)i].o_in;
                            std::memcpy(p, items[i].ids, 8 * (size_t)items[i].n);
                            std::memcpy(p + 8 * (size_t)items[i].n, items[i].pts, 16 * (size_t)items[i].n);
                        }
                    },
                    [](const char *) {});
}

vio_status vio_fm_export_batch(vio_fm *h, int32_t count, const vio_fm_export_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_export_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    size_t b_out = 0;
    const size_t b_pose = align256(8 * (7 * VIO_NF + 7));
    for (int i = 0; i < count; ++i) {
        const vio_fm_export_item &it = items[i];
        const FmSlot &s = h->slots[it.slot];
        if (!it.poses || !it.ext) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_export_batch: item %d: poses and ext are required", i);
        if (!all_finite(it.poses, 7 * VIO_NF) || !all_finite(it.ext, 7)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_export_batch: item %d: a pose is not finite", i);
        if (it.cap_landmarks < s.n_landmarks || it.cap_observations < s.n_observations)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_export_batch: item %d: the arrays hold %d landmarks and %d observations, the slot has %d and %d", i,
                        it.cap_landmarks, it.cap_observations, s.n_landmarks, s.n_observations);
        if ((s.n_landmarks > 0 && (!it.feature_ids || !it.inv_depth)) ||
            (s.n_observations > 0 && (!it.lm || !it.host || !it.target || !it.pts_i || !it.pts_j)))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_export_batch: item %d: an output array is NULL", i);
        FmItemD &d = h->its[(size_t)i];
        d.a = it.triangulate != 0; d.b = s.n_landmarks; d.c = s.n_observations;
        d.o_in = (int64_t)(b_pose * (size_t)i);
        d.o_out = (int64_t)b_out;
        b_out += align256(16 * (size_t)s.n_landmarks + 44 * (size_t)s.n_observations);
    }
    return run_call(h, t0, count, items, results, b_pose * (size_t)count, b_out, k_fm_export, FM_EXPORT_NT,
                    [&](char *in) {
                        for (int i = 0; i < count; ++i) {
                            double *p = (double *)(in + h->its[(size_t)i].o_in);
                            std::memcpy(p, items[i].poses, 8 * 7 * VIO_NF);
                            std::memcpy(p + 7 * VIO_NF, items[i].ext, 8 * 7);
                        }
                    },
                    [&](const char *out) {
                        for (int i = 0; i < count; ++i) {
                            const vio_fm_export_item &it = items[i];
                            const FmItemD &d = h->its[(size_t)i];
                            const size_t nl = (size_t)d.b, no = (size_t)d.c;     // (the kernel's layout: the counts the call began with)
                            const char *p = out + d.o_out;
                            if (nl) { std::memcpy(it.feature_ids, p, 8 * nl); std::memcpy(it.inv_depth, p + 8 * nl, 8 * nl); }
                            p += 16 * nl;
                            if (no) {
                                std::memcpy(it.pts_i, p, 16 * no); std::memcpy(it.pts_j, p + 16 * no, 16 * no);
                                p += 32 * no;
                                std::memcpy(it.lm, p, 4 * no); std::memcpy(it.host, p + 4 * no, 4 * no); std::memcpy(it.target, p + 8 * no, 4 * no);
                            }
                        }
                    });
}

vio_status vio_fm_set_depth_batch(vio_fm *h, int32_t count, const vio_fm_depth_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_set_depth_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    size_t b_in = 0;
    for (int i = 0; i < count; ++i) {
        const vio_fm_depth_item &it = items[i];
        if (it.mode != VIO_FM_DEPTH_SET && it.mode != VIO_FM_DEPTH_CLEAR) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_set_depth_batch: item %d: mode %d", i, it.mode);
        if (it.n != h->slots[it.slot].n_landmarks)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_set_depth_batch: item %d: n = %d, the slot has %d landmarks", i, it.n, h->slots[it.slot].n_landmarks);
        if (it.n > 0 && !it.x) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_set_depth_batch: item %d: x is required", i);
        if (!all_finite(it.x, it.n)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_set_depth_batch: item %d: a depth is not finite", i);
        FmItemD &d = h->its[(size_t)i];
        d.a = it.mode; d.b = it.remove_failures != 0; d.c = it.n;
        d.o_in = (int64_t)b_in;
        b_in += align256(8 * (size_t)it.n);
    }
    return run_call(h, t0, count, items, results, b_in, 0, k_fm_set_depth, FM_NT,
                    [&](char *in) {
                        for (int i = 0; i < count; ++i)
                            if (items[i].n) std::memcpy(in + h->its[(size_t)i].o_in, items[i].x, 8 * (size_t)items[i].n);
                    },
                    [](const char *) {});
}

vio_status vio_fm_slide_batch(vio_fm *h, int32_t count, const vio_fm_slide_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_slide_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    for (int i = 0; i < count; ++i) {
        const vio_fm_slide_item &it = items[i];
        if (it.kind != VIO_FM_BACK_SHIFT_DEPTH && it.kind != VIO_FM_BACK && it.kind != VIO_FM_FRONT)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_slide_batch: item %d: kind %d", i, it.kind);
        if (it.kind == VIO_FM_FRONT && (it.frame_count < 1 || it.frame_count > FM_WINDOW))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_slide_batch: item %d: frame_count must be in [1, %d]", i, FM_WINDOW);
        if (it.kind == VIO_FM_BACK_SHIFT_DEPTH) {
            if (!it.marg_R || !it.marg_P || !it.new_R || !it.new_P) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_slide_batch: item %d: the four matrices are required", i);
            if (!all_finite(it.marg_R, 9) || !all_finite(it.marg_P, 3) || !all_finite(it.new_R, 9) || !all_finite(it.new_P, 3))
                return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_slide_batch: item %d: a pose is not finite", i);
        }
        FmItemD &d = h->its[(size_t)i];
        d.a = it.kind; d.b = it.frame_count;
        d.o_in = 256 * (int64_t)i;
    }
    return run_call(h, t0, count, items, results, 256 * (size_t)count, 0, k_fm_slide, FM_NT,
                    [&](char *in) {
                        for (int i = 0; i < count; ++i) {
                            double *p = (double *)(in + 256 * (size_t)i);
                            std::memset(p, 0, 24 * 8);
                            if (items[i].kind != VIO_FM_BACK_SHIFT_DEPTH) continue;
                            std::memcpy(p, items[i].marg_R, 72); std::memcpy(p + 9, items[i].marg_P, 24);
                            std::memcpy(p + 12, items[i].new_R, 72); std::memcpy(p + 21, items[i].new_P, 24);
                        }
                    },
                    [](const char *) {});
}

vio_status vio_fm_corresponding_batch(vio_fm *h, int32_t count, const vio_fm_corr_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_corresponding_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    size_t b_out = 0;
    for (int i = 0; i < count; ++i) {
        const vio_fm_corr_item &it = items[i];
        const int n = h->slots[it.slot].n_tracks;
        if (it.l < 0 || it.l > it.r || it.r > FM_WINDOW) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_corresponding_batch: item %d: 0 <= l <= r <= %d is required", i, FM_WINDOW);
        if (it.cap_rows < n || (n > 0 && !it.rows))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_corresponding_batch: item %d: rows holds %d rows, the slot has %d tracks", i, it.cap_rows, n);
        FmItemD &d = h->its[(size_t)i];
        d.a = it.l; d.b = it.r; d.c = n;
        d.o_out = (int64_t)b_out;
        b_out += align256(32 * (size_t)n);
    }
    return run_call(h, t0, count, items, results, 0, b_out, k_fm_corresponding, FM_NT, [](char *) {},
                    [&](const char *out) {
                        for (int i = 0; i < count; ++i) {
                            const int nr = fm_clamp(results[i].n_rows, 0, h->its[(size_t)i].c);
                            results[i].n_rows = nr;
                            if (nr) std::memcpy(items[i].rows, out + h->its[(size_t)i].o_out, 32 * (size_t)nr);
                        }
                    });
}

vio_status vio_fm_tracks_set(vio_fm *h, int32_t slot, int32_t n, const int64_t *ids, const int32_t *start, const double *depth,
                             const int32_t *flag, const int64_t *off, const double *pts) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_FM_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_set: slot %d outside [0, %d)", slot, VIO_FM_MAX_SLOTS);
    if (n < 0 || n > VIO_FM_MAX_TRACKS) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_set: %d rows, a table has %d", n, VIO_FM_MAX_TRACKS);
    if (n > 0 && (!ids || !start || !depth || !flag || !off || !pts)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_set: a NULL array");
    if (n > 0 && off[0] != 0) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_set: off must start at 0");
    for (int i = 0; i < n; ++i) {
        const int64_t k = off[i + 1] - off[i];
        if (k < 1 || k > VIO_FM_MAX_OBS) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_set: row %d has %lld observations, outside [1, %d]", i, (long long)k, VIO_FM_MAX_OBS);
        if (start[i] < 0 || start[i] + k - 1 > FM_WINDOW)
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_set: row %d: start %d with %lld observations leaves the window", i, start[i], (long long)k);
        if (!std::isfinite(depth[i]) || !all_finite(pts + 2 * off[i], 2 * k)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_set: row %d: a point or the depth is not finite", i);
    }
    h->scratch_ids.assign(ids, ids + n);
    std::sort(h->scratch_ids.begin(), h->scratch_ids.end());
    if (std::adjacent_find(h->scratch_ids.begin(), h->scratch_ids.end()) != h->scratch_ids.end())
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_set: an id is listed twice");
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    if ((st = slot_table(h, slot)) != VIO_OK || (st = h->img.ensure(h->err, FM_TAB_BYTES)) != VIO_OK) return st;
    std::memset(h->img.h, 0, FM_TAB_BYTES);
    const FmTab T = fm_tab(h->img.h);
    int32_t nl = 0, no = 0;
    for (int i = 0; i < n; ++i) {
        const int k = (int)(off[i + 1] - off[i]);
        T.id[i] = ids[i]; T.depth[i] = depth[i]; T.start[i] = start[i]; T.nobs[i] = k; T.flag[i] = flag[i];
        for (int j = 0; j < k; ++j) {
            T.ox[j * FM_T + i] = pts[2 * (off[i] + j)];
            T.oy[j * FM_T + i] = pts[2 * (off[i] + j) + 1];
        }
        if (fm_usable(start[i], k)) { nl += 1; no += k - 1; }
    }
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->slots[slot].d, h->img.h, FM_TAB_BYTES, hipMemcpyHostToDevice, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "upload failed");
    FmSlot &s = h->slots[slot];
    s.n_tracks = n; s.n_landmarks = nl; s.n_observations = no;
    return VIO_OK;
}

vio_status vio_fm_tracks_get(vio_fm *h, int32_t slot, int32_t cap, int64_t cap_pts, int32_t *n_out, int64_t *ids, int32_t *start,
                             double *depth, int32_t *flag, int64_t *off, double *pts) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_FM_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_get: slot %d outside [0, %d)", slot, VIO_FM_MAX_SLOTS);
    const int n = h->slots[slot].n_tracks;
    if (!n_out || !off) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_get: a NULL array");
    if (cap < n || (n > 0 && (!ids || !start || !depth || !flag || !pts)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_get: room for %d rows, the slot has %d", cap, n);
    *n_out = n;
    off[0] = 0;
    if (n == 0) return VIO_OK;
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    if ((st = h->img.ensure(h->err, FM_TAB_BYTES)) != VIO_OK) return st;
    hipStream_t q = h->q.stream;
    if (hipMemcpyAsync(h->img.h, h->slots[slot].d, FM_TAB_BYTES, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "read-back failed");
    const FmTab T = fm_tab(h->img.h);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) total += fm_clamp(T.nobs[i], 0, FM_MAX_OBS);
    if (cap_pts < total) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_get: room for %lld observations, the slot has %lld", (long long)cap_pts, (long long)total);
    for (int i = 0; i < n; ++i) {
        const int k = fm_clamp(T.nobs[i], 0, FM_MAX_OBS);
        ids[i] = T.id[i]; depth[i] = T.depth[i]; start[i] = T.start[i]; flag[i] = T.flag[i];
        for (int j = 0; j < k; ++j) {
            pts[2 * (off[i] + j)] = T.ox[j * FM_T + i];
            pts[2 * (off[i] + j) + 1] = T.oy[j * FM_T + i];
        }
        off[i + 1] = off[i] + k;
    }
    return VIO_OK;
}

// ---- include/vio_fm_stream.h ---------------------------------------------------------------------------------

vio_status vio_fm_init_depth_batch(vio_fm *h, int32_t count, const vio_fm_init_depth_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_init_depth_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    const size_t b_pose = align256(8 * (FM_INIT_S + 1));
    for (int i = 0; i < count; ++i) {
        const vio_fm_init_depth_item &it = items[i];
        if (!it.poses || !it.ext) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_init_depth_batch: item %d: poses and ext are required", i);
        if (!all_finite(it.poses, 7 * VIO_NF) || !all_finite(it.ext, 7)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_init_depth_batch: item %d: a pose is not finite", i);
        if (!std::isfinite(it.s) || !(it.s > 0)) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_init_depth_batch: item %d: s must be finite and > 0", i);
        h->its[(size_t)i].o_in = (int64_t)(b_pose * (size_t)i);
    }
    return run_call(h, t0, count, items, results, b_pose * (size_t)count, 0, k_fm_init_depth, FM_EXPORT_NT,
                    [&](char *in) {
                        for (int i = 0; i < count; ++i) {
                            double *p = (double *)(in + h->its[(size_t)i].o_in);
                            std::memcpy(p, items[i].poses, 8 * 7 * VIO_NF);
                            std::memcpy(p + 7 * VIO_NF, items[i].ext, 8 * 7);
                            p[FM_INIT_S] = items[i].s;
                        }
                    },
                    [](const char *) {});
}

vio_status vio_fm_tracks_batch(vio_fm *h, int32_t count, const vio_fm_tracks_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_tracks_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    size_t b_out = 0;
    for (int i = 0; i < count; ++i) {
        const vio_fm_tracks_item &it = items[i];
        if (it.cap_tracks < 0 || it.cap_obs < 0) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_batch: item %d: a negative capacity", i);
        if (!it.off || (it.cap_tracks > 0 && (!it.ids || !it.start || !it.depth || !it.flag)) || (it.cap_obs > 0 && !it.pts))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_tracks_batch: item %d: a NULL array", i);
        FmItemD &d = h->its[(size_t)i];
        d.b = std::min<int32_t>(it.cap_tracks, FM_MAX_TRACKS);
        d.c = (int32_t)std::min<int64_t>(it.cap_obs, (int64_t)FM_MAX_TRACKS * FM_MAX_OBS);
        d.o_out = (int64_t)b_out;
        const size_t nt = (size_t)std::min(d.n_tracks, d.b), no = (size_t)std::min(d.n_tracks * FM_MAX_OBS, d.c);   // (the kernel's layout)
        b_out += align256(fm_tracks_bytes(nt, no));
    }
    return run_call(h, t0, count, items, results, 0, b_out, k_fm_tracks, FM_NT, [](char *) {},
                    [&](const char *out) {
                        for (int i = 0; i < count; ++i) {
                            const vio_fm_tracks_item &it = items[i];
                            const FmItemD &d = h->its[(size_t)i];
                            if (results[i].status != VIO_FM_STATUS_OK) continue;         // (nothing is written for a refused slot)
                            const size_t nt = (size_t)std::min(d.n_tracks, d.b), no = (size_t)std::min(d.n_tracks * FM_MAX_OBS, d.c);
                            const size_t n = (size_t)d.n_tracks;
                            if (n > nt) continue;                                        // (the kernel refused it)
                            const char *p = out + d.o_out;
                            const int64_t *off = (const int64_t *)(p + 16 * nt);
                            const size_t total = (size_t)fm_clamp((int32_t)off[n], 0, (int32_t)no);
                            std::memcpy(it.off, off, 8 * (n + 1));
                            if (n) { std::memcpy(it.ids, p, 8 * n); std::memcpy(it.depth, p + 8 * nt, 8 * n); }
                            p += 8 * (3 * nt + 1);
                            if (total) std::memcpy(it.pts, p, 16 * total);
                            p += 16 * no;
                            if (n) { std::memcpy(it.start, p, 4 * n); std::memcpy(it.flag, p + 4 * nt, 4 * n); }
                        }
                    });
}

// ---- include/vio_fm_outlier.h --------------------------------------------------------------------------------

vio_status vio_fm_remove_batch(vio_fm *h, int32_t count, const vio_fm_remove_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_remove_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    size_t total = 0;
    for (int i = 0; i < count; ++i) {
        const vio_fm_remove_item &it = items[i];
        if (it.n < 0 || it.n > VIO_FM_MAX_TRACKS) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_remove_batch: item %d: n = %d outside [0, %d]", i, it.n, VIO_FM_MAX_TRACKS);
        if (it.n > 0 && !it.ids) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_remove_batch: item %d: ids is required", i);
        total += (size_t)it.n;
    }
    h->scratch_ids.resize(total);                        // every item's ids, sorted, one item behind the other (c: where)
    h->scratch_perm.resize(total);
    size_t b_in = 0, b_out = 0, at = 0;
    for (int i = 0; i < count; ++i) {
        const vio_fm_remove_item &it = items[i];
        if (!fm_sort_ids(it.ids, it.n, h->scratch_ids.data() + at, h->scratch_perm.data() + at))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_remove_batch: item %d: an id is listed twice", i);
        FmItemD &d = h->its[(size_t)i];
        d.b = it.n; d.c = (int32_t)at;
        d.o_in = (int64_t)b_in; d.o_out = (int64_t)b_out;
        b_in += align256(8 * (size_t)it.n);
        b_out += align256((size_t)it.n);
        at += (size_t)it.n;
    }
    return run_call(h, t0, count, items, results, b_in, b_out, k_fm_remove, FM_NT,
                    [&](char *in) {
                        for (int i = 0; i < count; ++i)
                            if (items[i].n) std::memcpy(in + h->its[(size_t)i].o_in, h->scratch_ids.data() + h->its[(size_t)i].c, 8 * (size_t)items[i].n);
                    },
                    [&](const char *out) {
                        for (int i = 0; i < count; ++i) {
                            const FmItemD &d = h->its[(size_t)i];
                            results[i].n_rows = fm_clamp(results[i].n_rows, 0, d.n_tracks < d.b ? d.n_tracks : d.b);
                            if (items[i].erased) fm_unpermute_hits((const uint8_t *)out + d.o_out, h->scratch_perm.data() + d.c, d.b, items[i].erased);
                        }
                    });
}

// ---- include/vio_fm_predict.h --------------------------------------------------------------------------------

vio_status vio_fm_predict_batch(vio_fm *h, int32_t count, const vio_fm_predict_item *items, vio_fm_result *results) {
    if (!h) return VIO_ERR_BAD_ARG;
    const Tick t0 = std::chrono::steady_clock::now();
    vio_status st = begin_call(h, "vio_fm_predict_batch", count, items, results);
    if (st != VIO_OK || count == 0) return st;
    size_t b_out = 0;
    const size_t b_pose = align256(8 * FMP_IN);
    for (int i = 0; i < count; ++i) {
        const vio_fm_predict_item &it = items[i];
        const int n = h->slots[it.slot].n_tracks;
        if (it.frame_count < 0 || it.frame_count > FM_WINDOW) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_predict_batch: item %d: frame_count must be in [0, %d]", i, FM_WINDOW);
        if (!it.poses || !it.ext) return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_predict_batch: item %d: poses and ext are required", i);
        if (!all_finite(it.poses, 7 * VIO_NF) || !all_finite(it.ext, 7) || (it.next_pose && !all_finite(it.next_pose, 7)))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_predict_batch: item %d: a pose is not finite", i);
        if (it.cap_rows < n || (n > 0 && (!it.ids || !it.pts_cam)))
            return fail(h->err, VIO_ERR_BAD_ARG, "vio_fm_predict_batch: item %d: ids and pts_cam hold %d rows, the slot has %d tracks", i, it.cap_rows, n);
        FmItemD &d = h->its[(size_t)i];
        d.a = it.frame_count; d.b = n; d.c = it.next_pose != nullptr;
        d.o_in = (int64_t)(b_pose * (size_t)i);
        d.o_out = (int64_t)b_out;
        b_out += align256(32 * (size_t)n);
    }
    return run_call(h, t0, count, items, results, b_pose * (size_t)count, b_out, k_fm_predict, FM_NT,
                    [&](char *in) {
                        for (int i = 0; i < count; ++i) {
                            double *p = (double *)(in + h->its[(size_t)i].o_in);
                            std::memcpy(p, items[i].poses, 8 * 7 * VIO_NF);
                            std::memcpy(p + 7 * VIO_NF, items[i].ext, 8 * 7);
                            if (items[i].next_pose) std::memcpy(p + 7 * VIO_NF + 7, items[i].next_pose, 8 * 7);
                            else std::memset(p + 7 * VIO_NF + 7, 0, 8 * 7);
                        }
                    },
                    [&](const char *out) {
                        for (int i = 0; i < count; ++i) {
                            const FmItemD &d = h->its[(size_t)i];
                            const size_t n = (size_t)d.b;                        // (the kernel's layout: the rows the call began with)
                            const int nr = fm_clamp(results[i].n_rows, 0, d.b);
                            results[i].n_rows = nr;
                            const char *p = out + d.o_out;
                            if (nr) { std::memcpy(items[i].ids, p, 8 * (size_t)nr); std::memcpy(items[i].pts_cam, p + 8 * n, 24 * (size_t)nr); }
                        }
                    });
}

}  // extern "C"
