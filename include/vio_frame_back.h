/*
 * vio_frame_back.h — the forward-backward check of the tracker on resident frames, and a published read without rejectWithF
 * (libvio_frame_hip.so; include/vio_frame.h includes this header behind vio_frame_camera.h, and VIO_FRAME_HAS_BACK says so).
 * DESIGN.md section 36 has the kernel and the measurements.
 *
 * The check is include/vio_flow_back.h's, by the same kernel text: with it enabled, vio_frame_track_batch and the tracking step of
 * vio_frame_read_batch follow every point that tracked back into the slot's prev frame, and a point that is lost on the way or ends
 * farther than max_dist from where it started gets VIO_FLOW_FAIL_BACK_LOST or VIO_FLOW_FAIL_BACK_FAR.  vio_frame_read_batch keeps the
 * rows whose status is VIO_OK, as it always did, so such a point leaves the slot with those the tracker lost.
 *
 * VINS-Fusion, where the check comes from, does not run rejectWithF behind it.  vio_frame_set_reject_with_f(h, 0) gives that front
 * end: a published read marks every pair inactive, which is the branch pairs of fewer than VIO_REJECT_MIN_POINTS points always took:
 * k_reject_ransac is not launched, reject_status is VIO_OK, reject_hyp is -1 and n_after_reject = n_after_track.  setMask, the
 * detection and undistortedPoints run as always.  Either setting works without the other.
 *
 * With the check off and rejectWithF on (the defaults) every call does exactly what it did before this header existed.
 */
#ifndef VIO_FRAME_BACK_H
#define VIO_FRAME_BACK_H

#include "vio_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* vio_flow_set_back for the handle's tracker: cfg NULL is off, the default.  cfg->levels above the handle's flow levels is
 * VIO_ERR_BAD_ARG, and so is a vio_frame_set_config that would bring the flow levels below the levels of an enabled check; a refused
 * call leaves the handle's settings and its slots as they were. */
vio_status vio_frame_set_flow_back(vio_frame *h, const vio_flow_back_config *cfg);

/* vio_frame_track_batch with the check, laid out as vio_flow_track_back_batch's (back: [sum of n_pts] or NULL).  VIO_ERR_BAD_ARG on a
 * handle with the check off.  With the check enabled vio_frame_track_batch is this call with back = NULL. */
vio_status vio_frame_track_back_batch(vio_frame *h, int32_t count, const vio_frame_track_item *items, float *next_pts, vio_flow_pt_info *info,
                                      vio_flow_back_info *back);

/* enabled 1 (the default): a published vio_frame_read_batch runs rejectWithF.  0: it does not (see above). */
vio_status vio_frame_set_reject_with_f(vio_frame *h, int32_t enabled);

/* Of the tracking step of the slot's last vio_frame_read_batch: *n_checked, the points whose backward pass ran (those that tracked
 * forwards and were inside the tracker's border); *n_back_lost and *n_back_far, those of them that failed the check either way.  All
 * are 0 with the check off, before the first read and after vio_frame_reset.  Each may be NULL. */
vio_status vio_frame_read_back_info(const vio_frame *h, int32_t slot, int32_t *n_checked, int32_t *n_back_lost, int32_t *n_back_far);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
