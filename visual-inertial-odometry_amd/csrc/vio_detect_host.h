// vio_detect_host.h — the host side of the detection stage that needs no HIP call: the descriptor tables of the kernels in
// vio_detect_body.inc, the defaults, the checks, the table sizes, the fills and the unpacking of the results.  libvio_detect_hip
// (vio_detect.hip, at file scope) and libvio_frame_hip (vio_frame.hip, in namespace kd) include it ahead of the body; so does
// tests/cpp/front_host_main.cpp, with a plain C++ compiler.  It includes nothing itself: the including file has included <algorithm>,
// <cmath>, <cstdint>, <cstring>, ../../include/vio_detect.h, vio_host_base.h and vio_detect_math.h.
// An Item is a vio_detect_item or a vio_frame_detect_item (n_tracked, max_total, tracked, track_cnt, keep_order, new_pts).
// `pre` is what an entry point puts in front of its texts: "" in libvio_detect_hip, "vio_frame_detect_batch: " in libvio_frame_hip.
constexpr int TX = VIO_DETECT_TILE_X, TY = VIO_DETECT_TILE_Y;

struct DetItemD {
    int32_t w, h, n_tracked, max_total;
    int32_t active, has_mask, tiles_x, tiles;
    const uint8_t *img, *mask;          // device addresses of the image and of the mask (NULL without one)
    int64_t r;                          // the response map's offset, in doubles
    int64_t cand;                       // the candidate list's offset, in entries
    int32_t trk;                        // the first tracked point, in the tables of the call
    int32_t newp;                       // the first row of new_pts, in the call's
    int32_t pitch, pad;                 // bytes between the rows of the image and of the mask
};

struct DetTrk {
    int32_t cx, cy, cnt, pad;
};

struct DetRes {
    int32_t n_kept, n_new, n_cand, pad;
    unsigned long long maxbits;         // the bits of maxR
};

struct DetArgs {
    const DetItemD *items;
    const DetTrk *trk;
    double *r;
    uint32_t *cand;
    unsigned long long *tkey;           // [tracked points of the call]: the keys of the setMask loop, 0 once struck
    int32_t *kept_xy;                   // [tracked points of the call][2]: the kept centres in output order
    DetRes *res;
    int32_t *keep_order;
    float *new_pts;
    double quality;
    int32_t d2, count;
};

constexpr vio_detect_config DET_DEFAULTS = {VIO_DETECT_DEFAULT_QUALITY, VIO_DETECT_DEFAULT_MIN_DISTANCE, 0};

inline vio_status det_check_config(ErrText &err, const char *fn, const vio_detect_config *c) {
    if (!c || !(c->quality > 0.0 && c->quality <= 1.0) || c->min_distance < 0)
        return fail(err, VIO_ERR_BAD_ARG, "%s: quality in (0, 1], min_distance >= 0", fn);
    return VIO_OK;
}

inline vio_status det_check_counts(ErrText &err, const char *pre, int i, int n_tracked, int max_total) {
    if (n_tracked < 0 || n_tracked > VIO_DETECT_MAX_POINTS || max_total < 0 || max_total > VIO_DETECT_MAX_POINTS)
        return fail(err, VIO_ERR_BAD_ARG, "%sitem %d: n_tracked and max_total must be in [0, %d]", pre, i, VIO_DETECT_MAX_POINTS);
    return VIO_OK;
}

// The tracked points of item i against its width x height image: one that is not finite makes the item inactive (*active = 0, no
// error), one that rounds to a pixel outside the image is an error.
inline vio_status det_check_tracked(ErrText &err, const char *pre, int i, const float *tracked, int n_tracked, int width, int height,
                                    int32_t *active) {
    *active = 1;
    for (int k = 0; k < n_tracked; ++k) {
        const double x = tracked[2 * k], y = tracked[2 * k + 1];
        if (!std::isfinite(x) || !std::isfinite(y)) { *active = 0; continue; }
        const double rx = std::nearbyint(x), ry = std::nearbyint(y);
        if (rx < 0.0 || rx >= (double)width || ry < 0.0 || ry >= (double)height)
            return fail(err, VIO_ERR_BAD_ARG, "%sitem %d: tracked point %d (%g, %g) rounds to a pixel outside the %d x %d image", pre, i, k, x, y,
                        width, height);
    }
    return VIO_OK;
}

// what a call's items add up to
struct DetTotals {
    int64_t n_r = 0, n_cand = 0, n_trk = 0, n_new = 0;
    int max_tiles = 0;
};

// Item d (zeroed, then d.active decided) of a width x height image with rows at `pitch`: its geometry, its rows in the tables of the
// call and, if it is active, its response map and its candidate list.
inline void det_item(DetItemD &d, DetTotals &T, int width, int height, int pitch, int n_tracked, int max_total, bool has_mask) {
    d.w = width; d.h = height; d.pitch = pitch;
    d.tiles_x = (width + TX - 1) / TX;
    d.tiles = d.tiles_x * ((height + TY - 1) / TY);
    d.n_tracked = n_tracked; d.max_total = max_total;
    d.has_mask = has_mask;
    d.trk = (int32_t)T.n_trk; d.newp = (int32_t)T.n_new;
    T.n_trk += n_tracked; T.n_new += max_total;
    if (!d.active) return;                               // (nothing of it is staged)
    d.r = T.n_r; T.n_r += (int64_t)width * height;
    d.cand = T.n_cand; T.n_cand += (int64_t)std::max(width - 2, 0) * std::max(height - 2, 0);
    T.max_tiles = std::max(T.max_tiles, d.tiles);
}

// The tables of a call.  Uploaded: DetItemD per item | DetTrk per tracked point (b_it, b_tab in all).  Read back: DetRes per item |
// keep_order | new_pts (b_res, b_keep, b_out in all).  Device scratch: tkey | kept_xy (b_key, b_scratch in all).
struct DetSizes {
    size_t b_it, b_tab, b_res, b_keep, b_out, b_key, b_scratch;
};

inline DetSizes det_sizes(int count, int64_t n_trk, int64_t n_new) {
    DetSizes S;
    S.b_it = align256(sizeof(DetItemD) * (size_t)count); S.b_tab = S.b_it + sizeof(DetTrk) * (size_t)n_trk;
    S.b_res = align256(sizeof(DetRes) * (size_t)count); S.b_keep = align256(sizeof(int32_t) * (size_t)n_trk);
    S.b_out = S.b_res + S.b_keep + sizeof(float) * 2 * (size_t)n_new;
    S.b_key = align256(sizeof(unsigned long long) * (size_t)n_trk);
    S.b_scratch = S.b_key + sizeof(int32_t) * 2 * (size_t)n_trk;
    return S;
}

// the host half of the uploaded table: the descriptors, and every item's tracked points rounded to their pixels
template <class Item> void det_fill_table(char *tab_h, const DetSizes &S, int count, const Item *items, const DetItemD *its) {
    std::memcpy(tab_h, its, sizeof(DetItemD) * (size_t)count);
    DetTrk *ht = (DetTrk *)(tab_h + S.b_it);
    for (int i = 0; i < count; ++i) {
        const Item &it = items[i];
        const DetItemD &d = its[i];
        for (int k = 0; k < it.n_tracked; ++k) {
            DetTrk &t = ht[d.trk + k];
            t.cx = 0; t.cy = 0; t.cnt = 0; t.pad = 0;
            if (!d.active) continue;
            t.cx = (int32_t)std::nearbyint((double)it.tracked[2 * k]); t.cy = (int32_t)std::nearbyint((double)it.tracked[2 * k + 1]);
            t.cnt = it.track_cnt[k];
        }
    }
}

// the settings of a call; the addresses are the caller's to fill in
inline DetArgs det_args(const vio_detect_config &cfg, int count) {
    DetArgs a;
    std::memset(&a, 0, sizeof(a));
    a.quality = cfg.quality; a.d2 = det_d2(cfg.min_distance); a.count = count;
    return a;
}

// ... with the addresses of the tables above in their three device buffers
inline DetArgs det_args(const vio_detect_config &cfg, int count, const DetSizes &S, char *tab_d, char *out_d, char *scratch_d, double *r,
                        uint32_t *cand) {
    DetArgs a = det_args(cfg, count);
    a.items = (const DetItemD *)tab_d;
    a.trk = (const DetTrk *)(tab_d + S.b_it);
    a.r = r; a.cand = cand;
    a.tkey = (unsigned long long *)scratch_d;
    a.kept_xy = (int32_t *)(scratch_d + S.b_key);
    a.res = (DetRes *)out_d;
    a.keep_order = (int32_t *)(out_d + S.b_res);
    a.new_pts = (float *)(out_d + S.b_res + S.b_keep);
    return a;
}

// The results out of the host half of the read-back table, into the caller's arrays.  VIO_ERR_NOT_FINITE, with the first such item
// named in err, if an item was inactive.
template <class Item> vio_status det_unpack(ErrText &err, const char *out_h, const DetSizes &S, int count, const Item *items, const DetItemD *its,
                                            vio_detect_result *results) {
    vio_status ret = VIO_OK;
    const DetRes *res = (const DetRes *)out_h;
    const int32_t *keep = (const int32_t *)(out_h + S.b_res);
    const float *newp = (const float *)(out_h + S.b_res + S.b_keep);
    for (int i = 0; i < count; ++i) {
        const Item &it = items[i];
        const DetItemD &d = its[i];
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
            if (ret == VIO_OK) fail(err, VIO_ERR_NOT_FINITE, "item %d: a tracked point is not finite", i);
            ret = VIO_ERR_NOT_FINITE;
        }
        for (int k = 0; k < it.n_tracked; ++k) it.keep_order[k] = k < o.n_kept ? keep[d.trk + k] : -1;
        if (o.n_new > 0) std::memcpy(it.new_pts, newp + 2 * (size_t)d.newp, sizeof(float) * 2 * (size_t)o.n_new);
    }
    return ret;
}
