// vio_aif_math.h — the arithmetic of the resident all_image_frame (include/vio_aif.h) that a host compiler can
// build too: the rank that sorts a frame's points by feature id, the search of the erase, the admission rules and the offsets after
// an erase, and initialStructure's excitation sums, key walk, Eigen's toRotationMatrix, the product with ric^T and the bisection of
// the sorted tracks.  Device code of csrc/vio_aif.hip; plain C++ otherwise, so that tests/cpp/aif_math_main.cpp can run it on the host and
// tests/test_aif_reference.py can hold it to tests/aif_reference.py.  Contraction is off here for every includer: every product and
// sum is evaluated as written.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define AIF_FN __host__ __device__ __forceinline__
#else
#define AIF_FN inline
#endif

constexpr int AIF_MAX_SLOTS = 256;                  // VIO_AIF_MAX_SLOTS
constexpr int AIF_MAX_FRAMES = 32;                  // VIO_AIF_MAX_FRAMES
constexpr int AIF_MAX_FRAME_POINTS = 1024;          // VIO_AIF_MAX_FRAME_POINTS
constexpr int AIF_MAX_POINTS = 8192;                // VIO_AIF_MAX_POINTS
constexpr int AIF_MAX_SAMPLES = 4096;               // VIO_AIF_MAX_SAMPLES
constexpr int AIF_OFFS = 34;                        // VIO_AIF_OFFS
constexpr int AIF_STATUS_OK = 0, AIF_STATUS_POOL_FULL = 1, AIF_STATUS_FRAMES_FULL = 2, AIF_STATUS_NO_FRAME = 3;

// where point i of a frame goes: the number of the frame's ids below its own (the ids are distinct)
AIF_FN int aif_rank(const int64_t *ids, int n, int i) {
    const int64_t v = ids[i];
    int r = 0;
    for (int k = 0; k < n; ++k) r += ids[k] < v ? 1 : 0;
    return r;
}

// the index of header t_0 among the n_frames strictly increasing headers, or -1
AIF_FN int aif_find(const double *t, int n_frames, double t_0) {
    int k = -1;
    for (int j = 0; j < n_frames; ++j)
        if (t[j] == t_0) k = j;
    return k;
}

// processIMU: the status of a run of n samples for a slot that holds `held`; `open_exists`: the slot has had an image
AIF_FN int aif_imu_status(int open_exists, int held, int n) {
    return open_exists && held + n > AIF_MAX_SAMPLES ? AIF_STATUS_POOL_FULL : AIF_STATUS_OK;
}

// processImage: the status of a frame of n points for a slot of n_frames frames and `held` points; the frame count is asked first
AIF_FN int aif_image_status(int n_frames, int held, int n) {
    if (n_frames >= AIF_MAX_FRAMES) return AIF_STATUS_FRAMES_FULL;
    return held + n > AIF_MAX_POINTS ? AIF_STATUS_POOL_FULL : AIF_STATUS_OK;
}

// the erase of frames 0 .. k: entry j of the new offsets from the old ones (`last`: the index of the old end entry, which every
// entry behind the data repeats), relative to the pool's start
AIF_FN int64_t aif_slid_off(const int64_t *off, int last, int k, int j) {
    const int s = j + k + 1 < last ? j + k + 1 : last;
    return off[s] - off[k + 1] + off[0];
}

// ---- initialStructure's frame work (estimator.cpp:243-270, :308-374) ----
constexpr int AIF_STATUS_WALK = 4;                  // VIO_AIF_STATUS_WALK
constexpr int AIF_MAX_KEY = 32;                     // VIO_AIF_MAX_KEY
constexpr int AIF_MAX_TRACKS = 4096;                // VIO_AIF_MAX_TRACKS

// Eigen's Quaterniond::toRotationMatrix on (w, x, y, z), not normalised, row-major
AIF_FN void aif_quat_to_rot(const double *q, double *R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// C = A ric^T, every element (A_i0 ric_j0 + A_i1 ric_j1) + A_i2 ric_j2; C may not alias A or ric
AIF_FN void aif_mul_rict(const double *A, const double *ric, double *C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double p0 = A[3 * i] * ric[3 * j], p1 = A[3 * i + 1] * ric[3 * j + 1], p2 = A[3 * i + 2] * ric[3 * j + 2];
            C[3 * i + j] = (p0 + p1) + p2;
        }
}

// The excitation check (:243-270) over the n = F - 1 records of frames 1 .. F - 1 in time order (rec: the records, `stride` doubles
// apart, sum_dt at [0] and delta_v at [8..10]): sum_g from zero (the reference leaves it uninitialised), tmp_g = delta_v / sum_dt,
// aver_g = (sum_g * 1.0) / n, var += (x x + y y) + z z of tmp_g - aver_g, sqrt(var / n).  n = 0 gives NaN, as the lines do.
AIF_FN double aif_excitation(const double *rec, int stride, int n) {
    double sum_g[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < n; ++j) {
        const double *r = rec + (int64_t)stride * j;
        for (int c = 0; c < 3; ++c) sum_g[c] = sum_g[c] + r[8 + c] / r[0];
    }
    const double dn = (double)n;
    double aver_g[3];
    for (int c = 0; c < 3; ++c) aver_g[c] = (sum_g[c] * 1.0) / dn;
    double var = 0.0;
    for (int j = 0; j < n; ++j) {
        const double *r = rec + (int64_t)stride * j;
        const double x = r[8] / r[0] - aver_g[0], y = r[9] / r[0] - aver_g[1], z = r[10] / r[0] - aver_g[2];
        var = var + ((x * x + y * y) + z * z);
    }
    return std::sqrt(var / dn);
}

// The key walk (:309-327) as written.  is_key[j] and guess[j] (the keyframe whose pose is frame j's guess, or, for a keyframe, its
// own index) for the F frames; 0, or AIF_STATUS_WALK where i runs past n_key or a header of `headers` is found in no frame.
AIF_FN int aif_walk(const double *t, int F, const double *headers, int n_key, int32_t *is_key, int32_t *guess) {
    int i = 0, found = 0;
    for (int j = 0; j < F; ++j) {
        if (i >= n_key) return AIF_STATUS_WALK;
        if (t[j] == headers[i]) {
            is_key[j] = 1; guess[j] = i;
            ++i; ++found;
            continue;
        }
        if (t[j] > headers[i]) ++i;
        if (i >= n_key) return AIF_STATUS_WALK;
        is_key[j] = 0; guess[j] = i;
    }
    return found == n_key ? AIF_STATUS_OK : AIF_STATUS_WALK;
}

// the index of `id` in the ascending ids, or -1
AIF_FN int aif_bisect(const int64_t *ids, int n, int64_t id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && ids[lo] == id ? lo : -1;
}
