// vio_front_guess_math.h — the rule of a read's prediction (include/vio_frame_predict.h): how a slot's listed
// ids and pixels are laid out for the device, how a point's id is looked up among them, and when a slot is tracked again without a
// guess.  It is frontend.FeatureTracker._take_guess's rule: a stable sort of the listed ids, a lower bound per point, a hit where the
// id found is the point's and the point's id is not negative.  Device code of csrc/vio_front_guess_body.inc; plain C++ otherwise, so
// that tests/cpp/front_guess_main.cpp can run it on the host and tests/test_front_guess_cpu.py can hold it to a numpy restatement.
// Integers and comparisons only; pixels are copied.
#pragma once

#include <algorithm>
#include <cstdint>

#include "vio_front_math.h"

// The rows of a prediction as they go up: ids ascending, of a repeated id the first listed row alone, the pixels in the same order.
// out_ids: [n], out_px: [n][2]; returns the rows written (at most n).  Host code: a stable sort of at most FRONT_CAP indices.
inline int32_t front_guess_normalise(const long long *ids, const float *pixels, int32_t n, long long *out_ids, float *out_px) {
    int32_t order[FRONT_CAP];
    n = front_clamp(n, 0, FRONT_CAP);
    for (int32_t k = 0; k < n; ++k) order[k] = k;
    std::stable_sort(order, order + n, [ids](int32_t a, int32_t b) { return ids[a] < ids[b]; });
    int32_t m = 0;
    for (int32_t k = 0; k < n; ++k) {
        const int32_t r = order[k];
        if (m > 0 && out_ids[m - 1] == ids[r]) continue;    // (a later listing of the id before)
        out_ids[m] = ids[r];
        out_px[2 * m] = pixels[2 * r]; out_px[2 * m + 1] = pixels[2 * r + 1];
        ++m;
    }
    return m;
}

// the row of `id` among m ids in ascending order, or -1: the lower bound and the equality test; an id below 0 is no track's
FRONT_FN int32_t front_guess_find(const long long *sorted_ids, int32_t m, long long id) {
    if (id < 0) return -1;
    int32_t lo = 0, hi = m;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (sorted_ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < m && sorted_ids[lo] == id ? lo : -1;
}

// VINS-Fusion's fallback: a guessed slot with fewer than min_tracked points of status 0 is tracked again; min_tracked 0 is no fallback
FRONT_FN bool front_guess_falls_back(int32_t guessed, int32_t n_ok, int32_t min_tracked) {
    return guessed != 0 && min_tracked > 0 && n_ok < min_tracked;
}
