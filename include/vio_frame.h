/*
 * vio_frame.h — frames that stay on the GPU across equalisation, tracking and detection (companion library libvio_frame_hip.so).
 *
 * The image steps of FeatureTracker::readImage (VM/src/feature_tracker.cpp:87-149) for many image streams, with the images kept where
 * the kernels are: what vio_clahe_apply_batch, vio_flow_track_batch and vio_detect_batch compute from host arrays, computed from frames
 * that were uploaded once.  The kernels are the very ones of those three libraries (one copy of their source, compiled into both:
 * csrc/vio_clahe_body.inc, vio_flow_body.inc, vio_detect_body.inc), so every result equals theirs byte for byte.  DESIGN.md section 23
 * has the layout and the measurements.
 *
 * A handle owns VIO_FRAME_MAX_SLOTS slots, one per image stream.  A slot holds at most two resident frames, `prev` and `next` (the
 * reference's cur_img and forw_img), and at most one mask.  A frame is level 0, the image as the tracker and the detector see it
 * (equalised if the handle is configured so), and the pyramid levels 1 .. levels - 1 of include/vio_flow.h above it.
 *   vio_frame_push_batch      uploads each raw image once, equalises it on the device into level 0 (k_clahe_lut, k_clahe_apply) or
 *                             takes it as level 0, builds the pyramid once (k_flow_pyr_down), and makes the result the slot's next:
 *                             the former next becomes prev, the former prev is dropped.  It does not wait for the device: not for
 *                             its own work.  It does wait for the push before it (whose timing events it reads), and a buffer
 *                             that a later, larger call regrows is released by hipFree, which waits: calls back to back are safe
 *                             through those two waits, not through the stream's order alone.
 *   vio_frame_track_batch     vio_flow_track_batch's contract word for word, from the slot's prev into its next     (k_flow_track)
 *   vio_frame_set_mask        the slot's mask (the reference's fisheye mask): uploaded once, resident until replaced or cleared
 *   vio_frame_detect_batch    vio_detect_batch's contract word for word, on level 0 of the slot's next with the slot's mask
 *                             (k_detect_setmask, k_detect_response, k_detect_candidates, k_detect_select)
 *   vio_frame_download        one level of prev or next, tightly packed
 *   vio_frame_reset           drops the slot's frames (its mask stays), after which a push may bring another geometry
 *   vio_frame_read_batch      all of readImage for one new image per slot, the points kept on the device (vio_frame_read.h)
 * All work of a handle is enqueued on its one stream, in call order; that order is what keeps a frame from being overwritten while an
 * earlier call still reads it.  The handle owns the pinned memory uploads are staged in, and does not touch it again before the copy
 * that reads it has finished (an event).  Device storage grows by whole blocks and never moves or frees a frame.
 *
 * Rules:
 *   - argument errors write nothing, launch nothing and leave every slot as it was: VIO_ERR_BAD_ARG, vio_frame_last_error names the
 *     item.  They are: count < 0 or above VIO_FRAME_MAX_SLOTS, a NULL array, a slot outside [0, VIO_FRAME_MAX_SLOTS), a slot listed
 *     twice in one call, width or height below 1 or above VIO_FRAME_MAX_DIM, stride < width, a pyramid level smaller than 2 x 2, a
 *     geometry that differs from the slot's resident frames (until vio_frame_reset), tracking a slot with fewer than two frames,
 *     detecting on a slot without a frame or with a mask of another geometry, and those of the library whose contract the call follows;
 *   - a non-finite keypoint or tracked point behaves as in vio_flow_track_batch and vio_detect_batch: VIO_ERR_NOT_FINITE for the
 *     keypoint or the item, the others are computed as if it were not there;
 *   - repeated calls are bitwise identical, and an item's result depends neither on the batch nor on the slot it is in;
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 *
 * Resident points (VIO_FRAME_HAS_READ): include/vio_frame_read.h, which this header includes, declares vio_frame_read_batch and what
 * goes with it: all of readImage for one new image per slot, the points kept on the device.  include/vio_frame_camera.h, included behind
 * it (VIO_FRAME_HAS_SLOT_CAMERAS), gives every slot a camera of its own, of any model of include/vio_camera.h.  include/vio_frame_back.h
 * (VIO_FRAME_HAS_BACK) adds the tracker's forward-backward check, include/vio_frame_predict.h (VIO_FRAME_HAS_PREDICT) predicted pixels
 * for the tracking step of a read.
 */
#ifndef VIO_FRAME_H
#define VIO_FRAME_H

#include "vio_backend.h"
#include "vio_clahe.h"
#include "vio_detect.h"
#include "vio_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FRAME_VERSION 1
#define VIO_FRAME_MAX_SLOTS 256                     /* image streams of a handle; also the most items of one call */
#define VIO_FRAME_MAX_DIM 16384                     /* width and height, as VIO_FLOW_MAX_DIM */
#define VIO_FRAME_PREV 0                            /* `which` of vio_frame_download */
#define VIO_FRAME_NEXT 1
#define VIO_FRAME_HAS_READ 1                        /* include/vio_frame_read.h is there */
#define VIO_FRAME_HAS_BACK 1                        /* include/vio_frame_back.h is there: the forward-backward check */
#define VIO_FRAME_HAS_PREDICT 1                     /* include/vio_frame_predict.h is there: predicted pixels for a read's tracking step */

typedef struct vio_frame vio_frame;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_frame_create(int32_t device, void *stream, vio_frame **out);
void vio_frame_destroy(vio_frame *h);
const char *vio_frame_last_error(const vio_frame *h);      /* valid until the next call on h */
int32_t vio_frame_version(void);

/* equalize: 0 (level 0 is the image) or 1 (level 0 is its CLAHE).  clahe, flow, detect: the settings of those libraries under their
 * validity rules, or NULL for their defaults.  A new handle has equalize = 0 and the defaults.  A change of flow->levels drops every
 * resident frame (the masks stay). */
vio_status vio_frame_set_config(vio_frame *h, int32_t equalize, const vio_clahe_config *clahe, const vio_flow_config *flow,
                                const vio_detect_config *detect);

typedef struct vio_frame_push_item {
    int32_t slot;                   /* in [0, VIO_FRAME_MAX_SLOTS) */
    int32_t width, height;
    int32_t stride;                 /* bytes between rows, >= width */
    const uint8_t *img;             /* [height][stride], the raw image; free to change once the call has returned */
} vio_frame_push_item;
vio_status vio_frame_push_batch(vio_frame *h, int32_t count, const vio_frame_push_item *items);

typedef struct vio_frame_track_item {
    int32_t slot;
    int32_t n_pts;                  /* in [0, VIO_FLOW_MAX_POINTS] */
    const float *prev_pts;          /* [n_pts][2] (x, y) in the slot's prev */
    const float *guess;             /* [n_pts][2] start positions in the slot's next, or NULL: start at prev_pts */
} vio_frame_track_item;
/* next_pts: [sum of n_pts][2], info: [sum of n_pts] or NULL, laid out as vio_flow_track_batch's. */
vio_status vio_frame_track_batch(vio_frame *h, int32_t count, const vio_frame_track_item *items, float *next_pts, vio_flow_pt_info *info);

/* mask: [height][stride], zero where nothing may be detected, or NULL: the slot has no mask (the other arguments are ignored). */
vio_status vio_frame_set_mask(vio_frame *h, int32_t slot, const uint8_t *mask, int32_t width, int32_t height, int32_t stride);

typedef struct vio_frame_detect_item {
    int32_t slot;
    int32_t n_tracked;              /* in [0, VIO_DETECT_MAX_POINTS] */
    int32_t max_total;              /* in [0, VIO_DETECT_MAX_POINTS] */
    int32_t reserved;               /* 0 */
    const float *tracked;           /* [n_tracked][2] (x, y); may be NULL with n_tracked == 0 */
    const int32_t *track_cnt;       /* [n_tracked] */
    int32_t *keep_order;            /* out [n_tracked] */
    float *new_pts;                 /* out [max_total][2]; may be NULL with max_total == 0 */
} vio_frame_detect_item;
vio_status vio_frame_detect_batch(vio_frame *h, int32_t count, const vio_frame_detect_item *items, vio_detect_result *results);

/* Level `level` of the slot's prev (VIO_FRAME_PREV) or next (VIO_FRAME_NEXT): out[h_level][w_level], tightly packed.  It waits. */
vio_status vio_frame_download(vio_frame *h, int32_t slot, int32_t which, int32_t level, uint8_t *out);

vio_status vio_frame_reset(vio_frame *h, int32_t slot);

/* Bytes moved since creation: image bytes host to device, image bytes device to host, other bytes host to device, other bytes device
 * to host.  Image bytes are level-0 pixels and masks, width * height each whatever the device pitch; the other bytes are descriptor
 * tables, keypoints, results, and the levels above 0 of a download. */
vio_status vio_frame_counters(const vio_frame *h, uint64_t *out4);

/* ms of the last call of each kind (NaN before the first): push: host packing and enqueueing, upload, CLAHE kernels, pyramid kernels
 * (HIP events; this call waits for them); track: k_flow_track (HIP events), the whole call; detect: the four kernels, the whole call. */
vio_status vio_frame_timing(vio_frame *h, double *out8);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#include "vio_frame_read.h"
#include "vio_frame_camera.h"
#include "vio_frame_back.h"
#include "vio_frame_predict.h"

#endif
