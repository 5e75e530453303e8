/*
 * vio_frame_camera.h — a camera of its own for every resident slot, of any of the four models (libvio_frame_hip.so; include/vio_frame.h
 * includes this header behind vio_frame_read.h, and VIO_FRAME_HAS_SLOT_CAMERAS says so).  DESIGN.md section 29 has the layout, the
 * dispatch and the measurements.
 *
 * vio_frame_set_camera (include/vio_frame_read.h) gives a handle one PINHOLE camera, through which every slot lifts.  Streams from
 * different devices have different intrinsics, and a fisheye rig is no PINHOLE: vio_frame_set_slot_camera gives one slot the camera
 * include/vio_camera.h describes (PINHOLE, KANNALA_BRANDT, MEI, SCARAMUZZA), and vio_frame_read_batch then runs that slot's
 * rejectWithF and undistortedPoints through it.  The arithmetic is include/vio_camera.h's, the kernels are the same text
 * (csrc/vio_reject_body.inc against csrc/vio_camera_math.h), so every array of a slot equals, byte for byte, what
 * frontend.FeatureTracker(frames=, slot=s, rejecter=CameraHandle.bind(s)) followed by update_ids gives with the same camera.
 *
 * Read rules, added to those of include/vio_frame_read.h:
 *   - a listed slot needs a camera: its own, or the handle's (vio_frame_set_camera, PINHOLE as before).  A listed slot with neither is
 *     VIO_ERR_BAD_ARG for the whole call: nothing is written, launched or rolled;
 *   - the camera's width and height enter rejectWithF's virtual pixel only; they are not compared with the image;
 *   - a call in which no listed slot has a camera of its own runs exactly what it ran before this header existed.  Otherwise the
 *     whole call runs the general kernels, every descriptor naming its slot; a slot without its own camera takes the handle's as a
 *     PINHOLE camera of include/vio_camera.h, whose results are the same in every byte, so a slot's result does not depend on which of
 *     the two the call ran;
 *   - a lift the tracker cannot use (include/vio_camera.h: P0 / P2 or P1 / P2 not finite, P2 == 0 on a fisheye).  In
 *     undistortedPoints: every un_pts and velocity of the slot is NaN, in the rows returned and in the slot's prev_un (the velocities
 *     of the next frame are NaN with them), as vio_camera_undistort_batch leaves the item.  In rejectWithF (the RANSAC of a pair of 8
 *     points or more lifts both frames' points): the mask is all zeros, so every tracked point is dropped and the detector refills;
 *     reject_status is VIO_ERR_NOT_FINITE and reject_hyp -1.  Either way the slot's result.status is VIO_ERR_NOT_FINITE, the other
 *     slots are computed and get VIO_OK, the call returns VIO_ERR_NOT_FINITE, and the slot's frames and points have rolled.
 * The RANSAC settings stay one per handle.
 */
#ifndef VIO_FRAME_CAMERA_H
#define VIO_FRAME_CAMERA_H

#include "vio_frame.h"
#include "vio_camera.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FRAME_HAS_SLOT_CAMERAS 1

/* The slot's own camera, under the rules of vio_camera_set (the KANNALA_BRANDT monotonicity check among them); cam NULL clears it, and
 * the slot lifts through the handle's camera again.  A refused camera leaves the slot as it was.  The slot's frames, points, prev_un,
 * id counter and time are not touched.  The camera goes to the device ahead of the next read that needs it, on the handle's stream. */
vio_status vio_frame_set_slot_camera(vio_frame *h, int32_t slot, const vio_camera_model *cam);

/* *is_set: 1 if the slot has a camera of its own, and then *cam is that camera as it was given (reserved 0).  Either may be NULL. */
vio_status vio_frame_get_slot_camera(const vio_frame *h, int32_t slot, int32_t *is_set, vio_camera_model *cam);

/* The RANSAC settings of vio_frame_set_camera without a handle-wide camera (whose cam must not be NULL): for a handle whose slots all
 * have cameras of their own. */
vio_status vio_frame_set_reject_config(vio_frame *h, const vio_reject_config *cfg);

/* Of the slot's last vio_frame_read_batch, from its undistortedPoints stage as vio_camera_undistort_batch counts them: *n_clamped, the
 * KANNALA_BRANDT points beyond r(theta_max) (0 where a lift is bad, as there), and *n_bad, the points whose lift is not finite.  Both
 * are 0 before the first read and after vio_frame_reset.  Either may be NULL. */
vio_status vio_frame_read_lift_info(const vio_frame *h, int32_t slot, int32_t *n_clamped, int32_t *n_bad);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
