// vio_clahe_math.h — the arithmetic of CLAHE (include/vio_clahe.h): the geometry of an image, BORDER_REFLECT_101 with its full period,
// a bin's share of the redistributed excess, a LUT entry, an axis' tile pair and weights, the blend.  Device code of
// csrc/vio_clahe.hip; plain C++ otherwise (the host side of vio_clahe.hip uses clahe_geometry too), so that
// tests/test_clahe_host_mirror.py can compile it into a program for the host and hold it to tests/clahe_reference.py byte for byte.
// Histograms and redistribution are integers; the float32 operations are single products, sums and differences in a fixed order, and
// they are compiled with contraction off: a fused multiply-add in clahe_blend changes output bytes.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/vio_clahe.h"

#if defined(__HIPCC__)
#define CLAHE_FN __host__ __device__ __forceinline__
#else
#define CLAHE_FN inline
#endif

// steps 1 and 2 for one image
struct ClaheGeom {
    int32_t ext;                    // the histograms are taken of the extended image
    int32_t w_ext, h_ext, tile_w, tile_h, area, clip;
    float lut_scale, inv_tile_w, inv_tile_h;
};

CLAHE_FN ClaheGeom clahe_geometry(int32_t w, int32_t h, int32_t tiles_x, int32_t tiles_y, double clip_limit) {
    ClaheGeom g;
    g.ext = !(w % tiles_x == 0 && h % tiles_y == 0);
    g.w_ext = g.ext ? w + (tiles_x - w % tiles_x) : w;
    g.h_ext = g.ext ? h + (tiles_y - h % tiles_y) : h;
    g.tile_w = g.w_ext / tiles_x;
    g.tile_h = g.h_ext / tiles_y;
    g.area = g.tile_w * g.tile_h;
    g.clip = 0;
    if (clip_limit != 0.0) {
        const double c = clip_limit * (double)g.area / 256.0, top = (double)g.area;
        g.clip = (int32_t)(c < top ? c : top);
        if (g.clip < 1) g.clip = 1;
    }
    g.lut_scale = (float)255 / (float)g.area;
    g.inv_tile_w = 1.0f / (float)g.tile_w;
    g.inv_tile_h = 1.0f / (float)g.tile_h;
    return g;
}

// BORDER_REFLECT_101 of a position i >= 0 on an axis of n pixels, however far out
CLAHE_FN int32_t clahe_refl(int32_t i, int32_t n) {
    if (n == 1) return 0;
    const int32_t p = 2 * (n - 1), m = i % p;
    return m < n ? m : p - m;
}

// bin b after clipping and redistribution: hist is the bin's count, excess the tile's sum of max(hist - clip, 0); clip > 0
CLAHE_FN int32_t clahe_redistribute(int32_t hist, int32_t b, int32_t clip, int32_t excess) {
    int32_t v = hist < clip ? hist : clip;
    const int32_t batch = excess / VIO_CLAHE_BINS, residual = excess - VIO_CLAHE_BINS * batch;
    v += batch;
    if (residual > 0) {
        int32_t step = VIO_CLAHE_BINS / residual;
        if (step < 1) step = 1;
        if (b % step == 0 && b / step < residual) v += 1;
    }
    return v;
}

// saturate_u8(rint(r)): nearest, ties to even
CLAHE_FN uint8_t clahe_round_u8(float r) {
    const float q = rintf(r);
    return (uint8_t)(q < 0.0f ? 0.0f : (q > 255.0f ? 255.0f : q));
}

CLAHE_FN uint8_t clahe_lut_value(int32_t sum, float lut_scale) { return clahe_round_u8((float)sum * lut_scale); }

// the tile pair and the weights of position p on an axis of `tiles` tiles.  t1 lies in [-1, tiles - 1] before it is clamped (p is
// below tiles * tile); the upper bound is enforced all the same, so that an index stays inside the LUTs whatever comes.
CLAHE_FN void clahe_axis(int32_t p, float inv_tile, int32_t tiles, int32_t &t1, int32_t &t2, float &a, float &a1) {
    const float tf = (float)p * inv_tile - 0.5f;
    const float fl = floorf(tf);
    int32_t t = (int32_t)fl;
    a = tf - fl;
    a1 = 1.0f - a;
    if (t > tiles - 1) t = tiles - 1;
    t2 = t + 1 < tiles - 1 ? t + 1 : tiles - 1;
    t1 = t > 0 ? t : 0;
}

// step 5's res and its rounding
CLAHE_FN uint8_t clahe_blend(uint8_t l11, uint8_t l12, uint8_t l21, uint8_t l22, float xa, float xa1, float ya, float ya1) {
    const float top = (float)l11 * xa1 + (float)l12 * xa;
    const float bot = (float)l21 * xa1 + (float)l22 * xa;
    return clahe_round_u8(top * ya1 + bot * ya);
}
