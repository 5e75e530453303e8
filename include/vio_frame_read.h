/*
 * vio_frame_read.h — readImage for many streams on the device, the points kept there (libvio_frame_hip.so; include/vio_frame.h includes
 * this header, and VIO_FRAME_HAS_READ says so).  DESIGN.md section 24 has the layout, the rules and the measurements.
 *
 * Besides its frames and its mask a slot owns a point table on the device of
 * VIO_FRAME_MAX_TRACK_POINTS rows: cur_pts (float x, y), ids (int64, -1 for a point without one) and track_cnt (int32), which belong to
 * the slot's next frame; prev_un_ids / prev_un_pts, the ids and the normalised points of the frame before as they were when they were
 * undistorted, that is before updateID (the quirk include/vio_reject.h documents: a new point's velocity is zero in its first two
 * frames); and the slot's next free id.  The host keeps the two row counts, which it learns from each call's read-back, the count of
 * frames read (rejectWithF's `pair`) and the last time stamp.
 *   vio_frame_read_batch      FeatureTracker::readImage (feature_tracker.cpp:87-164, :258-306) and updateID (:204-214) for one new image
 *                             of each listed slot, in one call that waits once: the push above; the slot's points tracked from prev
 *                             into next (k_flow_track); those the tracker lost and those that round (ties to even) outside the border
 *                             dropped, track_cnt + 1; with `publish` rejectWithF (k_reject_ransac, pair = the frames the slot has read;
 *                             fewer than 8 points or VIO_REJECT_FAIL_NO_MODEL keep every point), setMask and the detection up to
 *                             max_cnt points (the four detect kernels, the slot's mask), the new points appended with id -1 and count
 *                             1; undistortedPoints against prev_un (k_reject_lift, dt = time - the slot's last time); prev_un
 *                             replaced; updateID in point order from the slot's counter; the points rolled.  Only the images go up
 *                             and only the published rows come down: what joins the kernels are five kernels of integer and copy
 *                             work (csrc/vio_front_body.inc).  Every array equals, byte for byte, what frontend.FeatureTracker over
 *                             vio_frame_push_batch / _track_batch / _detect_batch and vio_reject_batch / _undistort_batch gives,
 *                             followed by its update_ids.
 * Rules, besides those above:
 *   - a camera is required (vio_frame_set_camera, or for a slot its own: include/vio_frame_camera.h, any of the four models); a time that is not finite, or that does not increase while the slot's prev_un holds
 *     rows, is VIO_ERR_BAD_ARG, as are a slot listed twice, a geometry change and, with publish, a mask of another geometry: nothing is
 *     written, launched or rolled, and the slot's frames and points are as they were;
 *   - vio_frame_reset also drops the slot's points, its prev_un rows, its count of frames read and its time stamp; it keeps the slot's
 *     id counter.  A change of flow->levels does the same to every slot;
 *   - a direct vio_frame_push_batch on a slot drops that slot's points (they belong to the frame that has rolled away); prev_un, the
 *     counter, the count of frames read and the time stamp stay.
 */
#ifndef VIO_FRAME_READ_H
#define VIO_FRAME_READ_H

#include "vio_frame.h"
#include "vio_reject.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FRAME_MAX_TRACK_POINTS 1024             /* rows of a slot's point table: one workgroup scans it */
#define VIO_FRAME_DEFAULT_MAX_CNT 150               /* MAX_CNT */
#define VIO_FRAME_DEFAULT_BORDER 1                  /* inBorder's BORDER_SIZE */

/* The camera and the RANSAC settings of the slots' rejectWithF and undistortedPoints, under the validity rules of
 * include/vio_reject.h (PINHOLE only); cfg NULL: its defaults.  A read needs a camera: this one, or the slot's own
 * (vio_frame_set_slot_camera of include/vio_frame_camera.h, any model of include/vio_camera.h). */
vio_status vio_frame_set_camera(vio_frame *h, const vio_reject_camera *cam, const vio_reject_config *cfg);

/* max_cnt: the reference's MAX_CNT, in [0, VIO_FRAME_MAX_TRACK_POINTS]; border: inBorder's margin, >= 0.  A new handle has
 * VIO_FRAME_DEFAULT_MAX_CNT and VIO_FRAME_DEFAULT_BORDER. */
vio_status vio_frame_set_tracker(vio_frame *h, int32_t max_cnt, int32_t border);

typedef struct vio_frame_read_item {
    int32_t slot;                   /* in [0, VIO_FRAME_MAX_SLOTS) */
    int32_t width, height;
    int32_t stride;                 /* bytes between rows, >= width */
    const uint8_t *img;             /* [height][stride], the raw image */
    double time;                    /* the image's time stamp, finite */
    /* out: `rows` rows each, of which the first n are written; rows = max(max_cnt, the points the slot holds when the call begins),
     * and VIO_FRAME_MAX_TRACK_POINTS is always enough */
    float *pts;                     /* [rows][2] pixels */
    int64_t *ids;                   /* [rows], after updateID: none is -1 */
    int32_t *track_cnt;             /* [rows] */
    float *un_pts;                  /* [rows][2] normalised */
    float *velocity;                /* [rows][2] */
} vio_frame_read_item;

typedef struct vio_frame_read_result {
    int32_t status;                 /* VIO_OK; VIO_ERR_NOT_FINITE: the slot's own camera could not lift a point (vio_frame_camera.h) */
    int32_t n;                      /* the slot's points after the call: the rows written */
    int32_t n_new;                  /* of those, detected in this image (the last n_new rows; their ids are the counter's) */
    int32_t n_tracked_in;           /* the points the slot held */
    int32_t n_after_track;          /* ... still there after the tracker and the border */
    int32_t n_after_reject;         /* ... and after rejectWithF */
    int32_t reject_status;          /* VIO_OK or VIO_REJECT_FAIL_NO_MODEL (VIO_OK where nothing ran); VIO_ERR_NOT_FINITE as for status */
    int32_t reject_hyp;             /* the winning hypothesis, -1 where nothing ran */
    int32_t n_candidates;           /* the detector's */
    int32_t reserved;
} vio_frame_read_result;

/* publish: the reference's PUB_THIS_FRAME for the whole call, 0 or 1; with 0 neither rejectWithF nor the detection runs. */
vio_status vio_frame_read_batch(vio_frame *h, int32_t count, const vio_frame_read_item *items, int32_t publish, vio_frame_read_result *results);

/* Seeds the slot's points, which lie in its next frame (it needs one): n in [0, VIO_FRAME_MAX_TRACK_POINTS] rows pts [n][2],
 * ids [n] (-1: none yet), track_cnt [n].  Every point must be finite and round inside the frame; otherwise VIO_ERR_BAD_ARG and
 * nothing is written.  prev_un and the counter stay.  It waits. */
vio_status vio_frame_points_set(vio_frame *h, int32_t slot, int32_t n, const float *pts, const int64_t *ids, const int32_t *track_cnt);

/* The slot's points: *n and the first *n rows of pts, ids, track_cnt; *m and the first *m rows of prev_un_ids, prev_un_pts; the
 * slot's next free id.  Arrays of VIO_FRAME_MAX_TRACK_POINTS rows; any pointer may be NULL.  It waits. */
vio_status vio_frame_points_get(vio_frame *h, int32_t slot, int32_t *n, float *pts, int64_t *ids, int32_t *track_cnt, int32_t *m,
                                int64_t *prev_un_ids, float *prev_un_pts, int64_t *next_id);

/* ms of the last vio_frame_read_batch (NaN before the first): host checks, packing and enqueueing up to the first kernel of the join;
 * then by HIP events: the push (upload, CLAHE, pyramid), k_front_begin + k_flow_track + k_front_filter, k_reject_ransac +
 * k_front_after_reject, the four detect kernels, k_front_merge + k_reject_lift + k_front_finish, the read-back copy; last the whole
 * call. */
vio_status vio_frame_read_timing(const vio_frame *h, double *out8);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
