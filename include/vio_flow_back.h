/*
 * vio_flow_back.h — the forward-backward check of the batched Lucas-Kanade tracker (libvio_flow_hip.so; include/vio_flow.h includes
 * this header at its end, and VIO_FLOW_HAS_BACK says so).  DESIGN.md section 36 has the kernel, its resources and the measurements.
 *
 * The successor of the reference's front end (VINS-Fusion, FLOW_BACK) gates its tracks by following every point back from the new
 * image into the old one, starting at the point's old position, and keeping it only if it comes back to within half a pixel.  Here
 * that is a second run of the tracker of include/vio_flow.h inside k_flow_track, on the wavefront that holds the keypoint's state.
 *
 * For a keypoint p (float, in prev) whose forward result f has the status VIO_OK (tracked and inside the border):
 *   - The backward pass is the same tracker with the images exchanged: the template is the next pyramid at f, the moving image is the
 *     prev pyramid, the start is p under the guess rule of include/vio_flow.h.  It runs over the levels back_levels - 1 .. 0 of the
 *     same pyramids (vio_flow_back_config.levels in [1, the handle's levels]; 0 means the handle's levels), with the handle's own
 *     half_patch, max_iter, inverse and early_stop, the same lane-strided sums and butterfly in the same order.  No border test is
 *     applied to its result b.  In tests/flow_reference.py's words it is multi_level(img_next, img_prev, f, guess=p, levels=back_levels,
 *     border=0, order="wave64"), whose statuses OK and FAIL_BORDER both read as tracked (tests/flow_back_reference.py restates the whole).
 *   - The verdict.  A backward pass that is lost (success = false at level 0) gives VIO_FLOW_FAIL_BACK_LOST.  Otherwise
 *     dx = (double)bx - (double)px, dy likewise, d2 = dx * dx + dy * dy, every product and sum rounded on its own, and the point is
 *     kept (VIO_OK) iff d2 <= max_dist * max_dist (that product is formed once, on the host).  A comparison that is false, NaN
 *     included, gives VIO_FLOW_FAIL_BACK_FAR.  No square root is taken.  max_dist is finite and >= 0.
 * A keypoint whose forward status is VIO_FLOW_FAIL_LOST, VIO_FLOW_FAIL_BORDER or VIO_ERR_NOT_FINITE keeps that status, and its
 * backward pass does not run: backward status -1, NaN position, 0 iterations, NaN cost and d2.  next_pts is what the forward pass left,
 * in every case.  The determinism rules of include/vio_flow.h hold unchanged, and with the check off (the default) every byte of every
 * call is what it was before this header existed.
 */
#ifndef VIO_FLOW_BACK_H
#define VIO_FLOW_BACK_H

#include "vio_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FLOW_BACK_DEFAULT_MAX_DIST 0.5

/* Per-keypoint outcomes of the check, in vio_flow_pt_info.status beside those of include/vio_flow.h. */
#define VIO_FLOW_FAIL_BACK_LOST 3       /* tracked forwards and inside the border, lost on the way back */
#define VIO_FLOW_FAIL_BACK_FAR 4        /* came back, farther than max_dist from where it started */
#define VIO_FLOW_BACK_NOT_RUN (-1)      /* vio_flow_back_info.status of a keypoint that was not VIO_OK forwards */

typedef struct vio_flow_back_config {
    int32_t enabled;                /* 0 or 1 */
    int32_t levels;                 /* in [1, the handle's levels], or 0 for the handle's levels */
    double max_dist;                /* finite, >= 0 */
} vio_flow_back_config;

/* cfg NULL: off, the default.  A cfg whose levels exceed the handle's flow levels is VIO_ERR_BAD_ARG; so is a vio_flow_set_config
 * that would bring the flow levels below the levels of an enabled check.  A refused call leaves the handle as it was. */
vio_status vio_flow_set_back(vio_flow *h, const vio_flow_back_config *cfg);

typedef struct vio_flow_back_info {
    float x, y;                     /* where the backward pass ended in img_prev (NaN if it did not run) */
    int32_t status;                 /* VIO_OK: tracked, VIO_FLOW_FAIL_LOST: lost, VIO_FLOW_BACK_NOT_RUN */
    int32_t iterations;             /* of level 0 of the backward pass */
    double cost;                    /* as vio_flow_pt_info.cost, of the backward pass */
    double d2;                      /* the squared distance from prev_pts, formed whenever the backward pass ran; else NaN */
} vio_flow_back_info;

/* vio_flow_track_batch with the check, on a handle that has it enabled (otherwise VIO_ERR_BAD_ARG: nothing written, nothing
 * launched).  back: [sum of n_pts] or NULL.  With the check enabled vio_flow_track_batch is this call with back = NULL. */
vio_status vio_flow_track_back_batch(vio_flow *h, int32_t count, const vio_flow_item *items, float *next_pts, vio_flow_pt_info *info,
                                     vio_flow_back_info *back);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
