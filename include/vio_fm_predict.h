/*
 * vio_fm_predict.h — the tracks of a slot of include/vio_fm.h's handle as 3-D points in the camera of the next frame, in the same
 * library (libvio_fm_hip.so):
 *   vio_fm_predict_batch      VINS-Fusion's Estimator::predictPtsInNextFrame: every track that has a depth and ends at frame_count,
 *                             moved into the camera of the next pose                                             (k_fm_predict)
 * The points go to vio_camera_project_batch (include/vio_camera_project.h) for the pixels a Lucas-Kanade track starts from.
 *
 * The rule.  A row is predicted iff estimated_depth > 0 && n_obs >= 2 && start_frame + n_obs - 1 == frame_count.  The rows that qualify
 * come out in list order, compacted: ids[k] and pts_cam[k] of the k-th of them.  frame_count < 2 predicts nothing.
 *   The next pose is next_pose (P, then Q as x, y, z, w) when given; with next_pose NULL it is the constant-velocity one,
 * T_next = T_cur (T_prev^-1 T_cur) with cur = frame_count and prev = frame_count - 1:
 *       R_rel = R_prev^T R_cur      t_rel = R_prev^T (P_cur - P_prev)      R_next = R_cur R_rel      P_next = R_cur t_rel + P_cur
 *   Per row, with (x, y) the first observation and d the depth:
 *       p_c = (d x, d y, d)     p_i = ric p_c + tic     p_w = R_start p_i + P_start     p_l = R_next^T (p_w - P_next)
 *       p_cam = ric^T (p_l - tic)
 * Every entry of a matrix product is a dot product summed left to right, (a0 b0 + a1 b1) + a2 b2, every product and sum rounded on its
 * own (no contraction); the translation is added to (subtracted from) the finished dot product.  The rotation matrix of a quaternion
 * is evaluated as d_quat_to_R of the triangulation evaluates it (2x, 2y, 2z first; csrc/vio_fm_predict_math.h restates the
 * expressions under contraction off).  tests/fm_predict_reference.py is the same arithmetic in numpy; the device agrees with it in
 * every bit.
 *
 * It follows vio_fm.h's rules (argument errors launch nothing and write nothing; repeated calls are bitwise identical; a slot's result
 * depends neither on the batch nor on the slot index; no floating-point atomics; the caller's HIP device is restored; one launch and
 * one wait per call) and returns vio_fm_result unchanged: the slot's three counts, n_rows reused for the rows written, every other
 * field 0.  The table is read and never written.  There is no rule only the device can check: every status is VIO_FM_STATUS_OK.  A
 * slot never used has no rows and predicts none.  Argument errors: count outside [0, VIO_FM_MAX_SLOTS], NULL items or results, a slot
 * out of range or listed twice, frame_count outside [0, 10], cap_rows below the slot's n_tracks, poses or ext NULL, ids or pts_cam
 * NULL where the slot has rows, a pose that is not finite.
 */
#ifndef VIO_FM_PREDICT_H
#define VIO_FM_PREDICT_H

#include "vio_fm.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FM_HAS_PREDICT 1

typedef struct vio_fm_predict_item {
    int32_t slot;
    int32_t frame_count;            /* in [0, 10] */
    int32_t cap_rows;               /* rows of ids and pts_cam: at least the slot's n_tracks */
    int32_t reserved;               /* 0 */
    const double *poses;            /* [11][7]: P (3), Q (x, y, z, w), as vio_fm_export_item has them */
    const double *ext;              /* [7] */
    const double *next_pose;        /* [7], or NULL: the constant-velocity pose */
    int64_t *ids;                   /* out [cap_rows] */
    double *pts_cam;                /* out [cap_rows][3] */
} vio_fm_predict_item;
vio_status vio_fm_predict_batch(vio_fm *h, int32_t count, const vio_fm_predict_item *items, vio_fm_result *results);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
