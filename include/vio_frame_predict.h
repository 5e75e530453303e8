/*
 * vio_frame_predict.h — predicted pixels for the tracking step of vio_frame_read_batch (libvio_frame_hip.so; include/vio_frame.h
 * includes this header behind vio_frame_back.h, and VIO_FRAME_HAS_PREDICT says so).  DESIGN.md section 39 has the kernels and the
 * measurements.
 *
 * VINS-Fusion's setPrediction on resident points: a slot's pending prediction lists track ids with the pixels they are expected at in
 * the next image (vio_fm_predict_batch, then vio_camera_project_batch).  The next vio_frame_read_batch that lists the slot starts the
 * Lucas-Kanade search of a point whose id is listed from its predicted pixel and of every other point of the slot from its own pixel,
 * which is what frontend.FeatureTracker.set_prediction does through vio_frame_track_batch's guess; every published array equals that
 * path's byte for byte.  With vio_frame_set_prediction_fallback(h, k), k > 0, a slot whose guessed pass leaves fewer than k points
 * with status VIO_OK (after the forward-backward check where that is on) is tracked again without a guess, and the second pass is
 * the slot's result: VINS-Fusion's fallback.  The ids are joined, the statuses counted and the fallback decided on the device
 * (k_front_guess, k_front_fallback, k_front_take in csrc/vio_front_guess_body.inc); the read still waits once.
 *
 * A pending prediction is used by one read.  A vio_frame_read_batch that lists the slot and is not refused consumes it, whatever the
 * read does with it: a slot that holds one frame or no points has nothing to guess and drops it.  A refused read (VIO_ERR_BAD_ARG)
 * leaves it pending.  vio_frame_reset, a vio_frame_push_batch on the slot and a change of flow->levels drop it, as they drop the
 * slot's points.
 *
 * One rule differs from the per-stream path on purpose: a pixel that is not finite is refused here (VIO_ERR_BAD_ARG), where
 * vio_frame_track_batch takes such a guess and reports VIO_ERR_NOT_FINITE for the keypoint.
 *
 * A read whose listed slots have no pending prediction enqueues exactly what it enqueued before this header existed.
 */
#ifndef VIO_FRAME_PREDICT_H
#define VIO_FRAME_PREDICT_H

#include "vio_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct vio_frame_prediction_item {
    int32_t slot;                   /* in [0, VIO_FRAME_MAX_SLOTS) */
    int32_t n;                      /* in [0, VIO_FRAME_MAX_TRACK_POINTS]; 0: a prediction without rows, every point starts at its own pixel */
    const int64_t *ids;             /* [n]; an id below 0 never matches; of a repeated id the first listed row counts */
    const float *pixels;            /* [n][2] (x, y) in the next image, finite */
} vio_frame_prediction_item;

/* Stores each listed slot's prediction in host memory of the handle, in place of the one it had; touches no GPU and does not wait.
 * VIO_ERR_BAD_ARG, with nothing stored for any item: count < 0 or above VIO_FRAME_MAX_SLOTS, a NULL array, a slot out of range or
 * listed twice, n out of range, a NULL ids or pixels with n > 0, a pixel that is not finite. */
vio_status vio_frame_set_prediction_batch(vio_frame *h, int32_t count, const vio_frame_prediction_item *items);

/* Drops the slot's pending prediction; VIO_OK where there is none. */
vio_status vio_frame_clear_prediction(vio_frame *h, int32_t slot);

/* min_tracked in [0, VIO_FRAME_MAX_TRACK_POINTS]; 0 (the default): no fallback.  A handle setting, like vio_frame_set_tracker. */
vio_status vio_frame_set_prediction_fallback(vio_frame *h, int32_t min_tracked);

/* Of the tracking step of the slot's last vio_frame_read_batch: *n_listed, the rows of the prediction it consumed; *n_guessed, the
 * slot's points whose id was listed; *n_ok_guessed, the points with status VIO_OK after the guessed pass; *fell_back, 1 if the slot
 * was tracked again without a guess.  All are 0 without a prediction, before the first read and after vio_frame_reset; the last three
 * are 0 where the slot had no points to track.  Each may be NULL. */
vio_status vio_frame_read_predict_info(const vio_frame *h, int32_t slot, int32_t *n_listed, int32_t *n_guessed, int32_t *n_ok_guessed,
                                       int32_t *fell_back);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
