// vio_fm_outlier_math.h — what vio_fm_remove_batch (include/vio_fm_outlier.h) does with its id lists, where a host
// compiler can build it too: the bisection k_fm_remove (csrc/vio_fm_outlier_body.inc) runs per row on the sorted ids, and the host's
// sort with its permutation and duplicate check.  Integers only.  tests/cpp/fm_outlier_main.cpp runs this text on the host and
// tests/test_fm_outlier_cpu.py holds it to numpy's searchsorted.
#pragma once

#include <algorithm>
#include <cstdint>

#include "vio_fm_math.h"

// the first index in sorted[0 .. n) (ascending) whose id is not below key: n if every id is below it
FM_FN int32_t fm_id_lower_bound(const int64_t *sorted, int32_t n, int64_t key) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// where key is in sorted[0 .. n), or -1
FM_FN int32_t fm_id_find(const int64_t *sorted, int32_t n, int64_t key) {
    const int32_t k = fm_id_lower_bound(sorted, n, key);
    return k < n && sorted[k] == key ? k : -1;
}

// sorted[k] = ids[perm[k]], ascending.  False if an id is listed twice (sorted and perm are then still a sorted copy).
inline bool fm_sort_ids(const int64_t *ids, int32_t n, int64_t *sorted, int32_t *perm) {
    for (int32_t i = 0; i < n; ++i) perm[i] = i;
    std::sort(perm, perm + n, [ids](int32_t a, int32_t b) { return ids[a] < ids[b] || (ids[a] == ids[b] && a < b); });
    for (int32_t k = 0; k < n; ++k) sorted[k] = ids[perm[k]];
    for (int32_t k = 1; k < n; ++k)
        if (sorted[k] == sorted[k - 1]) return false;
    return true;
}

// the hit bytes of the sorted ids back in the caller's order
inline void fm_unpermute_hits(const uint8_t *hit_sorted, const int32_t *perm, int32_t n, uint8_t *erased) {
    for (int32_t k = 0; k < n; ++k) erased[perm[k]] = hit_sorted[k] ? 1 : 0;
}
