// vio_fm_math.h — the arithmetic of the batched FeatureManager (include/vio_fm.h) that a host compiler can build
// too: the usable test, the destination of a kept row in a chunked stable compaction, the three slide rules as one row transform, the
// parallax term and the depth shift.  Device code of csrc/vio_fm_body.inc; plain C++ otherwise, so that tests/cpp/fm_math_main.cpp can
// run it on the host and tests/test_fm_cpu.py can hold it to tests/fm_reference.py.  Contraction is off here for every includer: the
// two floating-point functions are evaluated exactly as written, left to right.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define FM_FN __host__ __device__ __forceinline__
#else
#define FM_FN inline
#endif

constexpr int FM_WAVE = 64;                         // rows of one ballot
constexpr int FM_NT = 1024;                         // threads of a workgroup: one chunk of rows
constexpr int FM_WAVES = FM_NT / FM_WAVE;
constexpr int FM_MAX_TRACKS = 2048;                 // VIO_FM_MAX_TRACKS
constexpr int FM_CHUNKS = FM_MAX_TRACKS / FM_NT;
constexpr int FM_MAX_OBS = 11;                      // VIO_FM_MAX_OBS
constexpr int FM_MAX_POINTS = 1024;                 // VIO_FM_MAX_POINTS
constexpr int FM_WINDOW = 10;                       // WINDOW_SIZE
constexpr int FM_BACK_SHIFT_DEPTH = 0, FM_BACK = 1, FM_FRONT = 2;

FM_FN int32_t fm_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// used_num >= 2 && start_frame < WINDOW_SIZE - 2: the tracks getFeatureCount counts
FM_FN bool fm_usable(int32_t start, int32_t n_obs) { return n_obs >= 2 && start < FM_WINDOW - 2; }

// A stable compaction of up to FM_MAX_TRACKS rows in chunks of FM_NT, 64 rows to a ballot: row r = FM_NT chunk + 64 wave + lane is kept
// if bit `lane` of its wave's ballot is set, and goes to (kept rows of the chunks before) + (kept rows of the chunk's waves before)
// + (kept rows of its wave before its lane).
FM_FN int32_t fm_lane_rank(uint64_t ballot, int32_t lane) { return (int32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull)); }
FM_FN int32_t fm_wave_count(uint64_t ballot) { return (int32_t)__builtin_popcountll(ballot); }
FM_FN int32_t fm_wave_base(const int32_t *wave_counts, int32_t wave) {
    int32_t s = 0;
    for (int32_t w = 0; w < wave; ++w) s += wave_counts[w];
    return s;
}
FM_FN int32_t fm_dest(int32_t chunk_base, const int32_t *wave_counts, int32_t wave, uint64_t ballot, int32_t lane) {
    return chunk_base + fm_wave_base(wave_counts, wave) + fm_lane_rank(ballot, lane);
}

// What a slide does to one row: the new start_frame, the observation it erases (-1: none), whether the row stays, whether its depth is
// re-hosted (removeBackShiftDepth's else branch).
struct FmSlide {
    int32_t start, erase, keep, shift;
};

FM_FN FmSlide fm_slide_row(int32_t kind, int32_t frame_count, int32_t start, int32_t n_obs) {
    FmSlide s;
    s.start = start; s.erase = -1; s.keep = 1; s.shift = 0;
    if (kind == FM_FRONT) {                              // removeFront (:334-354)
        if (start == frame_count) { s.start = start - 1; return s; }
        const int32_t j = FM_WINDOW - 1 - start;
        if (start + n_obs - 1 < frame_count - 1) return s;          // endFrame() < frame_count - 1
        if (j < 0 || j >= n_obs) return s;               // (the reference would erase past the end: the row is left alone)
        s.erase = j;
        s.keep = n_obs - 1 != 0;
        return s;
    }
    if (start != 0) { s.start = start - 1; return s; }  // removeBack, removeBackShiftDepth (:276-332)
    s.erase = 0;
    if (kind == FM_BACK_SHIFT_DEPTH) {
        s.keep = !(n_obs - 1 < 2);
        s.shift = s.keep;
    } else {
        s.keep = n_obs - 1 != 0;
    }
    return s;
}

// compensatedParallax2 (:356-389) with its identity compensation: u_i = x / dep_i with dep_i = 1.0
FM_FN double fm_parallax(double xi, double yi, double xj, double yj) {
    const double ui = xi / 1.0, vi = yi / 1.0;
    const double du = ui - xj, dv = vi - yj;
    const double a = du * du;
    const double b = dv * dv;
    return sqrt(a + b);
}

// whether addFeatureCheckParallax's loop takes the row (:79-80)
FM_FN bool fm_parallax_row(int32_t frame_count, int32_t start, int32_t n_obs) {
    return start <= frame_count - 2 && start + n_obs - 1 >= frame_count - 1;
}

// removeBackShiftDepth (:296-303): pts_i = uv_i * depth, w = marg_R pts_i + marg_P, dep_j = (new_R^T (w - new_P))[2]; every row sum
// from column 0 upwards, (a + b) + c.  R row-major.
FM_FN double fm_shift_depth(double x, double y, double depth, const double *mR, const double *mP, const double *nR, const double *nP,
                            double init_depth) {
    const double p0 = x * depth, p1 = y * depth, p2 = 1.0 * depth;
    double d[3];
    for (int r = 0; r < 3; ++r) {
        const double a = mR[3 * r] * p0, b = mR[3 * r + 1] * p1, c = mR[3 * r + 2] * p2;
        const double w = ((a + b) + c) + mP[r];
        d[r] = w - nP[r];
    }
    const double a = nR[2] * d[0], b = nR[5] * d[1], c = nR[8] * d[2];
    const double dep = (a + b) + c;
    return dep > 0 ? dep : init_depth;
}
