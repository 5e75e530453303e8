/*
 * vio_fm_outlier.h — erasing tracks by feature id from a slot of include/vio_fm.h's handle, in the same library (libvio_fm_hip.so)
 * (DESIGN.md section 34):
 *   vio_fm_remove_batch       removeOutlier (feature_manager.cpp:259-275, without the `return;` it starts with) for the rows whose ids
 *                             are listed, as if is_outlier were set on them; with the ids of the solve_flag == 2 rows it is
 *                             removeFailures (:161-171)                                                          (k_fm_remove)
 * The ids are the ones vio_fm_export_batch returned (feature_ids), which stay valid whatever rows a vio_fm_set_depth_batch with
 * remove_failures has erased since; the landmark index of the exported window does not.  The residual query (include/vio_residuals.h,
 * lm_flags) gives the landmarks to erase; the call sits behind vio_res_compute_batch and the marginalisation and in front of
 * vio_fm_slide_batch.
 * It follows vio_fm.h's rules (argument errors launch nothing and write nothing; repeated calls are bitwise identical; a slot's result
 * depends neither on the batch nor on the slot index; no floating-point operations at all; the caller's HIP device is restored; one
 * launch and one wait per call) and returns vio_fm_result unchanged.  There is no rule only the device can check: every result's
 * status is VIO_FM_STATUS_OK.  vio_fm_timing reports it as it reports the other batched calls.
 */
#ifndef VIO_FM_OUTLIER_H
#define VIO_FM_OUTLIER_H

#include "vio_fm.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FM_HAS_REMOVE 1

/* Every row of the slot's table whose feature_id is among ids[0 .. n) is erased, whatever its n_obs, start_frame, depth or flag.  The
 * rows that stay keep their order and every byte.  An id no row has is not an error: erased[i] (if given) says which ids named a
 * row.  A slot never used has no rows and nothing is erased.  The result holds the slot's three counts after the call, and n_rows,
 * the field vio_fm_corresponding_batch and vio_fm_tracks_batch use for their row totals, is reused here for the number of rows
 * erased; every other field is 0.  The handle's counts (vio_fm_counts) follow.  Argument errors: count outside [0, VIO_FM_MAX_SLOTS],
 * NULL items or results, a slot out of range or listed twice, n outside [0, VIO_FM_MAX_TRACKS], ids == NULL with n > 0, an id listed
 * twice within one item. */
typedef struct vio_fm_remove_item {
    int32_t slot;
    int32_t n;                      /* in [0, VIO_FM_MAX_TRACKS] */
    const int64_t *ids;             /* [n] feature ids, distinct, any order, any int64 value; may be NULL when n == 0 */
    uint8_t *erased;                /* [n] or NULL: 1 where ids[i] named a row (now gone), 0 where no row had that id */
} vio_fm_remove_item;
vio_status vio_fm_remove_batch(vio_fm *h, int32_t count, const vio_fm_remove_item *items, vio_fm_result *results);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
