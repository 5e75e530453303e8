/*
 * vio_fm_stream.h — the two pieces of FeatureManager traffic a stream driver needs beside include/vio_fm.h, in the same library
 * (libvio_fm_hip.so) and on the same handle, so that a driver can keep its track list in a slot:
 *   vio_fm_init_depth_batch   visualInitialAlign's depth hand-over (estimator.cpp:406-417, :436-442): clearDepth(-1), triangulate on
 *                             the un-scaled SfM poses, estimated_depth *= s                                     (k_fm_init_depth)
 *   vio_fm_tracks_batch       the list of every listed slot as arrays in one launch with one wait: sfm_f (estimator.cpp:275-289),
 *                             what vio_fm_tracks_get returns one slot at a time                                 (k_fm_tracks)
 * Both follow vio_fm.h's rules (argument errors launch nothing; a rule only the device can check leaves the slot as it was and names
 * a VIO_FM_STATUS_* in its result; repeated calls are bitwise identical; a slot's result depends neither on the batch nor on the
 * slot index; no floating-point atomics; the caller's HIP device is restored) and return vio_fm_result unchanged.  vio_fm_timing
 * reports them as it reports the other batched calls.
 */
#ifndef VIO_FM_STREAM_H
#define VIO_FM_STREAM_H

#include "vio_fm.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FM_HAS_STREAM 1
#define VIO_FM_STATUS_CAPACITY 4                    /* tracks_batch: the item's arrays are too small for the slot */

/* For every usable row (n_obs >= 2 && start_frame < WINDOW_SIZE - 2): estimated_depth = -1, then the depth vio_fm_export_batch
 * (triangulate = 1) would write for it on `poses` / `ext` (a depth below 0.1 becomes init_depth), then that depth times s: one IEEE
 * product, init_depth fallbacks included (estimator.cpp:441).  Rows that are not usable keep their depth; no solve_flag changes.
 * visualInitialAlign passes the SfM poses and tic = 0 in ext; the call does not force it.  result.n_triangulated is the number of
 * usable rows.  Argument errors: those of vio_fm_export_batch, and an s that is not finite or not > 0. */
typedef struct vio_fm_init_depth_item {
    int32_t slot;
    int32_t reserved;
    double s;                       /* finite and > 0 */
    const double *poses;            /* [11][7]: P (3), Q (x, y, z, w) */
    const double *ext;              /* [7] */
} vio_fm_init_depth_item;
vio_status vio_fm_init_depth_batch(vio_fm *h, int32_t count, const vio_fm_init_depth_item *items, vio_fm_result *results);

/* Every listed slot's list as vio_fm_tracks_get returns it, byte for byte: track i has observations pts[off[i] .. off[i + 1]).
 * result.n_tracks is the number of tracks, result.n_rows the total number of observations.  cap_tracks below the slot's n_tracks or
 * cap_obs below that total gives VIO_FM_STATUS_CAPACITY: nothing is written for that slot, n_rows is the total it needs, the other
 * slots are served.  Argument errors: a negative capacity, a NULL array where the capacity is not 0 (off is always required). */
typedef struct vio_fm_tracks_item {
    int32_t slot;
    int32_t cap_tracks;
    int64_t cap_obs;
    int64_t *ids;                   /* [cap_tracks] */
    int32_t *start;                 /* [cap_tracks] */
    double *depth;                  /* [cap_tracks] */
    int32_t *flag;                  /* [cap_tracks] */
    int64_t *off;                   /* [cap_tracks + 1] */
    double *pts;                    /* [cap_obs][2] */
} vio_fm_tracks_item;
vio_status vio_fm_tracks_batch(vio_fm *h, int32_t count, const vio_fm_tracks_item *items, vio_fm_result *results);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
