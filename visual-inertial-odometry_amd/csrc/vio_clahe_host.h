// vio_clahe_host.h — the host side of the CLAHE stage that needs no HIP call: the descriptor tables of the kernels in
// vio_clahe_body.inc, the defaults, the config check and the descriptor fill.  libvio_clahe_hip (vio_clahe.hip, at file scope) and
// libvio_frame_hip (vio_frame.hip, in namespace kc) include it ahead of the body; so does tests/cpp/front_host_main.cpp, with a plain C++
// compiler.  It includes nothing itself: the including file has included <cmath>, <cstdint>, ../../include/vio_clahe.h, vio_host_base.h
// and vio_clahe_math.h.
constexpr int TX = VIO_CLAHE_TILE_X, TY = VIO_CLAHE_TILE_Y;
constexpr int PX = 4;                   // pixels of a thread per pass

struct ClaheItemD {
    int32_t w, h, pitch, ext;           // pitch: bytes between rows of the source and of the result, a multiple of PX
    int32_t tile_w, tile_h, area, clip;
    int32_t ptiles_x, ptiles;           // the blocks of pixels of k_clahe_apply: across, and in all
    float lut_scale, inv_tile_w, inv_tile_h;
    int32_t pad;
    const uint8_t *src;                 // device addresses, 4-byte aligned
    uint8_t *dst;
};

struct ClaheArgs {
    const ClaheItemD *items;
    uint8_t *luts;                      // [count][tiles_y][tiles_x][256]
    int32_t tiles_x, tiles_y, count;
};

constexpr vio_clahe_config CLAHE_DEFAULTS = {VIO_CLAHE_DEFAULT_CLIP_LIMIT, VIO_CLAHE_DEFAULT_TILES, VIO_CLAHE_DEFAULT_TILES};

inline vio_status clahe_check_config(ErrText &err, const char *fn, const vio_clahe_config *c) {
    if (!c || !std::isfinite(c->clip_limit) || c->clip_limit < 0.0 || c->tiles_x < 1 || c->tiles_x > VIO_CLAHE_MAX_TILES || c->tiles_y < 1 ||
        c->tiles_y > VIO_CLAHE_MAX_TILES)
        return fail(err, VIO_ERR_BAD_ARG, "%s: clip_limit finite and >= 0, tiles_x and tiles_y in [1, %d]", fn, VIO_CLAHE_MAX_TILES);
    return VIO_OK;
}

// the pitch of the library's own device copies
inline int clahe_pitch(int width) { return (width + PX - 1) / PX * PX; }

// item d (zeroed) of a width x height image with source and result rows at `pitch`; the addresses are the caller's to fill in
inline void clahe_item(ClaheItemD &d, int width, int height, int pitch, const vio_clahe_config &cfg) {
    const ClaheGeom g = clahe_geometry(width, height, cfg.tiles_x, cfg.tiles_y, cfg.clip_limit);
    d.w = width; d.h = height; d.pitch = pitch;
    d.ext = g.ext; d.tile_w = g.tile_w; d.tile_h = g.tile_h; d.area = g.area; d.clip = g.clip;
    d.ptiles_x = (width + TX - 1) / TX;
    d.ptiles = d.ptiles_x * ((height + TY - 1) / TY);
    d.lut_scale = g.lut_scale; d.inv_tile_w = g.inv_tile_w; d.inv_tile_h = g.inv_tile_h;
}

inline ClaheArgs clahe_args(const ClaheItemD *items, uint8_t *luts, const vio_clahe_config &cfg, int count) {
    ClaheArgs a;
    a.items = items; a.luts = luts;
    a.tiles_x = cfg.tiles_x; a.tiles_y = cfg.tiles_y; a.count = count;
    return a;
}
