// vio_front_math.h — the index arithmetic of the device-side join of libvio_frame_hip (include/vio_frame.h): the
// rounding and the border test of readImage's inBorder, the destination of a kept row in a stable compaction, and updateID's id
// assignment.  Device code of csrc/vio_front_body.inc; plain C++ otherwise, so that tests/cpp/front_math_main.cpp can run it on the
// host and tests/test_front_cpu.py can hold it to a numpy restatement.  Integers and comparisons only, besides the one rounding.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FRONT_FN __host__ __device__ __forceinline__
#else
#define FRONT_FN inline
#endif

constexpr int FRONT_WAVE = 64;                      // rows of one ballot
constexpr int FRONT_CAP = 1024;                     // VIO_FRAME_MAX_TRACK_POINTS: the rows of a slot's table, one workgroup
constexpr int FRONT_WAVES = FRONT_CAP / FRONT_WAVE;

// cvRound on a coordinate: to the nearest integer, ties to even (the default rounding mode on the host, the only one on the device)
FRONT_FN double front_rint(float v) { return rint((double)v); }

// readImage's inBorder on the rounded position, as FeatureTracker.in_border has it: b <= x < w - b and b <= y < h - b.  A NaN
// compares false; an infinity is outside.
FRONT_FN bool front_in_border(float x, float y, int32_t w, int32_t h, int32_t b) {
    const double rx = front_rint(x), ry = front_rint(y);
    return (double)b <= rx && rx < (double)(w - b) && (double)b <= ry && ry < (double)(h - b);
}

// the pixel a point known to round inside the image rounds to
FRONT_FN int32_t front_pixel(float v) { return (int32_t)front_rint(v); }

// A stable compaction of up to FRONT_CAP rows, 64 to a ballot: row r = 64 wave + lane is kept if bit `lane` of its wave's ballot is set,
// and goes to (kept rows of the waves before) + (kept rows of its wave before its lane).
FRONT_FN int32_t front_lane_rank(uint64_t ballot, int32_t lane) { return (int32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull)); }
FRONT_FN int32_t front_wave_count(uint64_t ballot) { return (int32_t)__builtin_popcountll(ballot); }
FRONT_FN int32_t front_wave_base(const int32_t *wave_counts, int32_t wave) {
    int32_t s = 0;
    for (int32_t w = 0; w < wave; ++w) s += wave_counts[w];
    return s;
}

// updateID: a row without an id (-1) takes the counter plus the number of such rows before it; the counter moves by their total
FRONT_FN int64_t front_new_id(int64_t id, int64_t next_id, int32_t rank) { return id == -1 ? next_id + (int64_t)rank : id; }

// a count the device wrote, held to the rows there are
FRONT_FN int32_t front_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
