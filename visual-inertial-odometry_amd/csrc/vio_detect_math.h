// vio_detect_math.h — the per-pixel arithmetic of the corner detector (include/vio_detect.h): BORDER_REFLECT_101, the 3 x 3 Sobel of a
// neighbourhood, the response R of the box sums, the disc tests and the order of the keys.  Device code of csrc/vio_detect.hip; plain
// C++ otherwise (the host side of vio_detect.hip uses det_d2 too), so that tests/test_detect_host_mirror.py can compile it for the host
// and hold it to tests/detect_reference.py bit for bit.  Everything is an integer up to the one sqrt of det_response, whose
// operand is exact; no product is followed by a sum in double, so contraction has nothing to fuse.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/vio_detect.h"

#if defined(__HIPCC__)
#define DET_FN __host__ __device__ __forceinline__
#else
#define DET_FN inline
#endif

// BORDER_REFLECT_101 for an index at most one image away, kept inside [0, n) whatever comes
DET_FN int det_refl(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    if (i < 0) i = 0;
    return i < n ? i : n - 1;
}

// the Sobel pair of the 3 x 3 neighbourhood v[row][column]
DET_FN void det_sobel(const int v[3][3], int &gx, int &gy) {
    gx = (v[0][2] + 2 * v[1][2] + v[2][2]) - (v[0][0] + 2 * v[1][0] + v[2][0]);
    gy = (v[2][0] + 2 * v[2][1] + v[2][2]) - (v[0][0] + 2 * v[0][1] + v[0][2]);
}

// R of the box sums a = sum gx^2, b = sum gx gy, c = sum gy^2: the smaller eigenvalue of [a b; b c], un-normalised
DET_FN double det_response(int32_t a, int32_t b, int32_t c) {
    const int64_t d = (int64_t)a - (int64_t)c;
    const int64_t rad = d * d + 4 * (int64_t)b * (int64_t)b;
    return 0.5 * ((double)(a + c) - sqrt((double)rad));
}

// A key of the greedy loops.  k == 0: none.  Candidates: k = the bits of R (> 0), (x, y) the pixel; tracked points: k = track_cnt
// (biased to unsigned) in the high word and 0xFFFFFFFF - index in the low one, (x, y) the rounded centre.
struct DetKey {
    unsigned long long k;
    int32_t x, y;
};

DET_FN unsigned long long det_track_key(int32_t cnt, int32_t index) {
    return ((unsigned long long)((uint32_t)cnt ^ 0x80000000u) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)index);
}

// a comes before b: k descending, then the pixel index y W + x descending (x < W: the same as y, then x)
DET_FN bool det_key_before(const DetKey &a, const DetKey &b) {
    if (a.k != b.k) return a.k > b.k;
    if (a.y != b.y) return a.y > b.y;
    return a.x > b.x;
}

// min_distance^2 for the disc tests; dx^2 + dy^2 < 2^30 for every pair of pixels, so larger values test the same
DET_FN int32_t det_d2(int32_t min_distance) {
    const int64_t d2 = (int64_t)min_distance * (int64_t)min_distance;
    return (int32_t)(d2 < ((int64_t)1 << 30) ? d2 : ((int64_t)1 << 30));
}

// setMask's disc (<=) and the selection's (<, and the corner itself)
template <bool STRICT> DET_FN bool det_struck(int32_t x, int32_t y, int32_t cx, int32_t cy, int32_t d2) {
    const int32_t dx = x - cx, dy = y - cy, dd = dx * dx + dy * dy;
    return STRICT ? (dd < d2 || dd == 0) : dd <= d2;
}
