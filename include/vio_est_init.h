/*
 * vio_est_init.h — the two things the reference's Estimator does to its own window state beside include/vio_est.h, in the same
 * library (libvio_est_hip.so) and on the same handle, so that a stream can live in its slot from its first IMU sample (DESIGN.md
 * section 33):
 *   vio_est_init_apply_batch    visualInitialAlign's writes into the slot (estimator.cpp:397-404, :419-425, :433, :444-455) from the rows
 *                               vio_init_align_batch wrote for the window                      (k_est_init_apply, frame i on lane i)
 *   vio_est_relinearize_batch   IntegrationBase::repropagate (integration_base.h:38-52) for the intervals whose start frame's bias
 *                               moved past a threshold                                         (k_est_relinearize, interval j on lane j)
 * A slot keeps an interval as its samples and its constructor arguments, and vio_est_window_batch recomputes every record from them.
 * A re-propagation is therefore a write of lin_bias[j]; there is no second copy of the propagation kernel.  vio_est.h says of an
 * interval that "its constructor arguments never change": with this header that holds between these two calls only.  The
 * linearisation biases of an interval that exists change here and nowhere else; its (acc_0, gyr_0) and its samples still never do.
 *
 * Both calls follow vio_est.h's rules: argument errors write nothing and launch nothing for the whole call (VIO_ERR_BAD_ARG,
 * vio_est_last_error names the item): count outside [0, VIO_EST_MAX_SLOTS], a NULL array, a slot out of range or listed twice, a
 * non-finite input, a negative threshold.  A rule only the device can check leaves that slot exactly as it was, names a
 * VIO_EST_STATUS_* in the slot's result and does not touch the other slots of the call.  Repeated calls are bitwise identical and a
 * slot's result depends neither on the batch nor on the slot index.  The products have vio_est.h's written orders and there is no
 * atan2 / sin / cos in either call, so both agree with a host restatement (csrc/vio_est_init_math.h) bit for bit.  vio_est_timing
 * reports them as it reports the other batched calls.
 */
#ifndef VIO_EST_INIT_H
#define VIO_EST_INIT_H

#include "vio_est.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_EST_HAS_INIT 1
#define VIO_EST_STATUS_NOT_READY 2                  /* init_apply: frame_count != WINDOW_SIZE, or one of intervals 0 .. 10 does not exist */

/* visualInitialAlign's state change.  poses / speed_bias are the K = 11 rows vio_init_align_batch wrote for this window ((p, q xyzw)
 * and (V, ba, bg)), g and rot are vio_init_result.g and .rot as they are.  In this order:
 *   Ps[i] = p_i;  q_i / sqrt(((x x + y y) + z z) + w w) (double2vector's normalisation);  Rs[i] = toRotationMatrix(q_i);
 *   Vs[i] = V_i, Bas[i] = ba_i, Bgs[i] = bg_i;  the slot's g = rot g (M v in vio_est.h's order);
 *   lin_bias[j] = (0, 0, 0, Bgs[j]) for every interval j in 0 .. 10: repropagate(Vector3d::Zero(), Bgs[i]) taken literally.
 * Nothing else changes: Headers, frame_count, the samples and their offsets, first, acc_0 / gyr_0, tic / ric,
 * last_R / last_P / last_R0 / last_P0, first_imu and failure_occur stay.  The reference would dereference a null pre_integrations[i]
 * where an interval is missing; here such a slot, and one whose window is not full, gets VIO_EST_STATUS_NOT_READY.  The rows of a
 * window whose alignment failed are NaN, which is an argument error: a caller lists its successes only.  The result is a
 * vio_est_result with status and frame_count.
 *
 * commit_last != 0 also writes last_R / last_P / last_R0 / last_P0 = Rs[10] / Ps[10] / Rs[0] / Ps[0] of the window just written.  The
 * reference's INITIAL branch (estimator.cpp:192-201) runs no failureDetection behind its first solve and sets the four afterwards;
 * vio_est_update_batch always runs it, against the last_P the slot holds, which is zero in a fresh slot and an earlier stream's in a
 * reused one, so a window whose newest frame lies more than 5 m from there (1 m in z) would be reported as a failure by the first
 * update.  With commit_last that first verdict measures against the initialisation's own newest frame. */
typedef struct vio_est_init_item {
    int32_t slot;
    int32_t commit_last;
    double poses[11][7];
    double speed_bias[11][9];
    double g[3];
    double rot[9];                  /* row-major */
} vio_est_init_item;
vio_status vio_est_init_apply_batch(vio_est *h, int32_t count, const vio_est_init_item *items, vio_est_result *results);

/* repropagate for the intervals whose bias moved.  For j in 1 .. 10 where interval j exists (it starts at frame j - 1): if
 * max_c |Bas[j - 1][c] - lin_bias[j][c]| > ba_thresh or max_c |Bgs[j - 1][c] - lin_bias[j][3 + c]| > bg_thresh (strict), then
 * lin_bias[j] = (Bas[j - 1], Bgs[j - 1]), and the next vio_est_window_batch returns that interval's record at the new biases.
 * Interval 0 is never touched.  Thresholds are finite and >= 0. */
typedef struct vio_est_relin_item {
    int32_t slot;
    int32_t reserved;
    double ba_thresh;
    double bg_thresh;
} vio_est_relin_item;
typedef struct vio_est_relin_result {
    int32_t status;                 /* VIO_EST_STATUS_OK */
    int32_t frame_count;
    int32_t n_relinearized;         /* intervals re-propagated */
    int32_t mask;                   /* bit j: interval j was re-propagated */
} vio_est_relin_result;
vio_status vio_est_relinearize_batch(vio_est *h, int32_t count, const vio_est_relin_item *items, vio_est_relin_result *results);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
