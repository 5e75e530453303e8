// vio_flow_host.h — the host side of the tracking stage that needs no HIP call: the descriptor tables of the kernels in
// vio_flow_body.inc, the defaults, the checks, the fills and the unpacking of the results.  libvio_flow_hip (vio_flow.hip, at file
// scope) and libvio_frame_hip (vio_frame.hip, in namespace kf) include it ahead of the body; so does tests/cpp/front_host_main.cpp, with
// a plain C++ compiler.  It includes nothing itself: the including file has included <cstdint>, ../../include/vio_flow.h and
// vio_host_base.h.
// An Item is a vio_flow_item or a vio_frame_track_item (n_pts, prev_pts, guess).
// The forward-backward check (include/vio_flow_back.h) adds FlowBackOut, FlowBackArgs, flow_check_back, flow_back_args and
// flow_unpack_back beside what the forward pass has; tests/cpp/flow_back_host_main.cpp builds them with a plain C++ compiler.
constexpr int MAXL = VIO_FLOW_MAX_LEVELS;

struct FlowItemD {
    int32_t w[MAXL], h[MAXL];
    int32_t pitch[MAXL];                // bytes between the rows of a level, the same for both images
    uint8_t *prev[MAXL], *next[MAXL];   // the levels' device addresses
    int32_t active, pad;                // 0: an item without keypoints, nothing of it is staged
};

struct FlowPt {
    int32_t item, has_guess;
    float px, py, gx, gy;
};

struct FlowOut {
    float x, y;
    int32_t status, iterations;
    double cost;
};

// the backward row of a keypoint (include/vio_flow_back.h): vio_flow_back_info's fields
struct FlowBackOut {
    float x, y;
    int32_t status, iterations;
    double cost, d2;
};

struct PyrArgs {
    const FlowItemD *items;
    int32_t level;                      // the source level
    int32_t nimg;
    int32_t both, pad;                  // 1: image 2 i is item i's prev and image 2 i + 1 its next; 0: image i is item i's next
};

struct FlowArgs {
    const FlowItemD *items;
    const FlowPt *pts;
    FlowOut *out;
    int32_t npts, levels, half_patch, max_iter, border, early_stop;
};

// k_flow_track<INV, true>'s arguments: the forward pass's, the backward rows (NULL: none are written), the top level of the backward pass and max_dist squared
struct FlowBackArgs {
    FlowArgs f;
    FlowBackOut *back;
    int32_t back_levels, pad;
    double max_d2;
};

constexpr vio_flow_back_config FLOW_BACK_DEFAULTS = {0, 0, VIO_FLOW_BACK_DEFAULT_MAX_DIST};

constexpr vio_flow_config FLOW_DEFAULTS = {VIO_FLOW_DEFAULT_LEVELS, VIO_FLOW_DEFAULT_HALF_PATCH, VIO_FLOW_DEFAULT_MAX_ITER, 0, VIO_FLOW_DEFAULT_BORDER, 0};

inline vio_status flow_check_config(ErrText &err, const char *fn, const vio_flow_config *c) {
    if (!c || c->levels < 1 || c->levels > VIO_FLOW_MAX_LEVELS || c->half_patch < 1 || c->half_patch > VIO_FLOW_MAX_HALF_PATCH || c->max_iter < 1 ||
        c->max_iter > 1000 || (c->inverse != 0 && c->inverse != 1) || c->border < 0 || (c->early_stop != 0 && c->early_stop != 1))
        return fail(err, VIO_ERR_BAD_ARG, "%s: levels in [1, %d], half_patch in [1, %d], max_iter in [1, 1000], "
                    "inverse and early_stop 0 or 1, border >= 0", fn, VIO_FLOW_MAX_LEVELS, VIO_FLOW_MAX_HALF_PATCH);
    return VIO_OK;
}

// the settings of the check against the flow levels they run under; c NULL is the check off
inline vio_status flow_check_back(ErrText &err, const char *fn, const vio_flow_back_config *c, int flow_levels) {
    if (!c) return VIO_OK;
    if ((c->enabled != 0 && c->enabled != 1) || c->levels < 0 || c->levels > flow_levels || !(c->max_dist >= 0.0) || !(c->max_dist <= 1.7976931348623157e308))
        return fail(err, VIO_ERR_BAD_ARG, "%s: the check's enabled 0 or 1, its levels in [0, %d] (the flow levels), max_dist finite and >= 0", fn, flow_levels);
    return VIO_OK;
}

// the levels the backward pass runs over under `flow_levels` flow levels
inline int flow_back_levels(const vio_flow_back_config &b, int flow_levels) { return b.levels > 0 ? b.levels : flow_levels; }

// the sizes of the levels of a width x height image; false if one is smaller than 2 x 2
inline bool flow_level_dims(int width, int height, int levels, int32_t *w, int32_t *hh) {
    for (int l = 0; l < levels; ++l) {
        w[l] = l ? w[l - 1] / 2 : width;
        hh[l] = l ? hh[l - 1] / 2 : height;
        if (w[l] < 2 || hh[l] < 2) return false;
    }
    return true;
}

// an active item of `levels` levels of these sizes and pitches; the addresses are the caller's to fill in
inline void flow_item(FlowItemD &d, int levels, const int32_t *w, const int32_t *h, const int32_t *pitch) {
    d.active = 1;
    for (int l = 0; l < levels; ++l) {
        const int32_t wl = w[l], hl = h[l], pl = pitch[l];       // (the arrays may be d's own)
        d.w[l] = wl; d.h[l] = hl; d.pitch[l] = pl;
    }
}

// item i's keypoints, and their guesses where it has some
template <class Item> void flow_fill_pts(FlowPt *hp, int i, const Item &it) {
    for (int k = 0; k < it.n_pts; ++k) {
        FlowPt &p = hp[k];
        p.item = i; p.has_guess = it.guess != nullptr;
        p.px = it.prev_pts[2 * k]; p.py = it.prev_pts[2 * k + 1];
        p.gx = it.guess ? it.guess[2 * k] : 0.f; p.gy = it.guess ? it.guess[2 * k + 1] : 0.f;
    }
}

inline FlowArgs flow_args(const FlowItemD *items, const FlowPt *pts, FlowOut *out, size_t total, int levels, const vio_flow_config &cfg) {
    FlowArgs a;
    a.items = items; a.pts = pts; a.out = out;
    a.npts = (int32_t)total; a.levels = levels; a.half_patch = cfg.half_patch; a.max_iter = cfg.max_iter;
    a.border = cfg.border; a.early_stop = cfg.early_stop;
    return a;
}

inline FlowBackArgs flow_back_args(const FlowItemD *items, const FlowPt *pts, FlowOut *out, FlowBackOut *back, size_t total, int levels,
                                   const vio_flow_config &cfg, const vio_flow_back_config &bcfg) {
    FlowBackArgs a;
    a.f = flow_args(items, pts, out, total, levels, cfg);
    a.back = back; a.back_levels = flow_back_levels(bcfg, levels); a.pad = 0;
    a.max_d2 = bcfg.max_dist * bcfg.max_dist;
    return a;
}

// The results in the order of the keypoints of the call, into next_pts and (unless NULL) info.  VIO_ERR_NOT_FINITE, with the first
// such keypoint named in err, if one or its guess was not finite.
template <class Item> vio_status flow_unpack(ErrText &err, const FlowOut *out_h, int count, const Item *items, float *next_pts, vio_flow_pt_info *info) {
    vio_status ret = VIO_OK;
    size_t row = 0;
    for (int i = 0; i < count; ++i) {
        for (int k = 0; k < items[i].n_pts; ++k) {
            const FlowOut &o = out_h[row + (size_t)k];
            next_pts[2 * (row + k)] = o.x; next_pts[2 * (row + k) + 1] = o.y;
            if (info) {
                vio_flow_pt_info &fi = info[row + k];
                fi.status = o.status; fi.iterations = o.iterations; fi.cost = o.cost;
            }
            if (o.status == VIO_ERR_NOT_FINITE) {
                if (ret == VIO_OK) fail(err, VIO_ERR_NOT_FINITE, "item %d: keypoint %d or its guess is not finite", i, k);
                ret = VIO_ERR_NOT_FINITE;
            }
        }
        row += (size_t)items[i].n_pts;
    }
    return ret;
}

// The backward rows in the order of the keypoints of the call, into back (one vio_flow_back_info per keypoint).
template <class Item> void flow_unpack_back(const FlowBackOut *back_h, int count, const Item *items, vio_flow_back_info *back) {
    size_t row = 0;
    for (int i = 0; i < count; ++i) {
        for (int k = 0; k < items[i].n_pts; ++k) {
            const FlowBackOut &o = back_h[row + (size_t)k];
            vio_flow_back_info &bi = back[row + (size_t)k];
            bi.x = o.x; bi.y = o.y; bi.status = o.status; bi.iterations = o.iterations; bi.cost = o.cost; bi.d2 = o.d2;
        }
        row += (size_t)items[i].n_pts;
    }
}
