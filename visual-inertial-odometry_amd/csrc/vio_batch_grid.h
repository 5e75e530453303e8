// vio_batch_grid.h — the window of a workgroup in the batch grids of the companion libraries (vio_covariance.hip, vio_residuals.hip).
//
// A batch grid gives window w the workgroups [blk0[w], blk0[w + 1]) (blk0 ascending, blk0[0] = 0; a window without work has
// blk0[w] = blk0[w + 1]).  Each window's workgroups restart at its own element 0, so a workgroup does exactly what the single-window
// kernel does on that window alone.
#ifndef VIO_BATCH_GRID_H
#define VIO_BATCH_GRID_H

#include <hip/hip_runtime.h>

// the last w with blk0[w] <= b: the window that owns workgroup b (uniform over the workgroup)
__device__ __forceinline__ int batch_window(const int *__restrict__ blk0, int count, unsigned b) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((unsigned)blk0[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

#endif
