// vio_obs_csr.h — the observation list grouped by landmark (host only), shared by the companion libraries (vio_covariance.hip,
// vio_residuals.hip).
//
// off[n + 1] are the landmarks' first slots; the edges of landmark l take the slots off[l] .. off[l + 1] - 1 in the caller's order
// (the grouping is stable).  place(e, l, q) is called once per edge e, in order, with its landmark l and slot q; returning false stops
// the build, and obs_csr returns false.  The caller has checked every lm[e] to lie in [0, n).
#ifndef VIO_OBS_CSR_H
#define VIO_OBS_CSR_H

#include <cstdint>
#include <vector>

template <class Place>
static bool obs_csr(int64_t m, const int32_t *lm, int64_t n, int *off, Place &&place) {
    for (int64_t l = 0; l <= n; ++l) off[l] = 0;
    for (int64_t e = 0; e < m; ++e) ++off[lm[e] + 1];
    for (int64_t l = 0; l < n; ++l) off[l + 1] += off[l];
    std::vector<int> fill(off, off + n);
    for (int64_t e = 0; e < m; ++e) {
        const int l = lm[e], q = fill[l]++;
        if (!place(e, l, q)) return false;
    }
    return true;
}

#endif
