/*
 * vio_est.h — the Estimator's window state and IMU buffers of many streams on the GPU (companion library libvio_est_hip.so).
 *
 * The reference's Estimator (vins-mono/src/estimator.cpp) joins the stages: it owns Ps / Rs / Vs / Bas / Bgs / Headers, the raw IMU
 * samples of every interval of the window, acc_0 / gyr_0, last_R / last_P / last_R0 / last_P0 and frame_count.  Here a handle keeps up
 * to VIO_EST_MAX_SLOTS such states resident on the device, one per stream ("slot"), and every method runs for `count` slots in one
 * call with one wait:
 *   vio_est_imu_batch      processIMU (:105-139) for a run of samples per slot                  (k_est_imu, one wavefront per slot)
 *   vio_est_image_batch    Headers[frame_count] = header, frame_count++ (:154, :206-207)        (k_est_image)
 *   vio_est_window_batch   vector2double (:505-547) and the window's ten pre-integrations       (k_est_export, k_imu_propagate)
 *   vio_est_update_batch   double2vector (:549-619), then failureDetection (:645-691)           (k_est_update, frame i on lane i)
 *   vio_est_slide_batch    slideWindow, both branches (:1144-1264)                              (k_est_slide, one workgroup per slot)
 *   vio_est_reset          clearState + setParameter of one slot (:46-103)
 *   vio_est_state_set / _get   seed and download one slot's whole state                         (copies)
 * It works from host arrays and needs nothing from libvio_hip but the vio_status / vio_preint types.  DESIGN.md section 30 has the
 * layout, the kernels and the measurements.
 *
 * A slot holds what vio_est_state lists, and the samples (dt, acc, gyr) of its 11 intervals, contiguous in interval order in one
 * region of VIO_EST_MAX_SAMPLES samples, with 12 offsets; interval j holds the samples between frame j - 1 and frame j.  td,
 * relocalisation (relo_*, drift_correct_*), all_image_frame and tmp_pre_integration are not carried: nothing in this project reads
 * them, td is not estimated, and the initialisation has its own libraries.  An IntegrationBase is kept as its constructor arguments
 * (acc_0, gyr_0, linearised Ba, Bg) and its samples; vio_est_window_batch recomputes the record from them with the kernel of
 * libvio_imu_hip (the same text, csrc/vio_imu_body.inc), which equals the reference's incremental push_back, also after a
 * slideWindowNew merge, because an interval's samples never change order and its constructor arguments never change.  Samples are
 * appended to interval frame_count only, so the intervals behind it are empty; vio_est_state_set refuses a state where they are not,
 * and one where an interval that does not exist holds samples.
 *
 * The order of every product and sum is part of this contract (csrc/vio_est_math.h is its one text; no contraction anywhere).
 * 3 x 3 matrices are row-major, quaternions (x, y, z, w).
 *   M v                 (M_i0 v_0 + M_i1 v_1) + M_i2 v_2                       A B: (A_i0 B_0j + A_i1 B_1j) + A_i2 B_2j
 *   toRotationMatrix    Eigen's, not normalised: tx = 2x, ty = 2y, tz = 2z, twx = tx w, twy = ty w, twz = tz w, txx = tx x,
 *                       txy = ty x, txz = tz x, tyy = ty y, tyz = tz y, tzz = tz z;
 *                       [1 - (tyy + tzz), txy - twz, txz + twy; txy + twz, 1 - (txx + tzz), tyz - twx; txz - twy, tyz + twx, 1 - (txx + tyy)]
 *   processIMU          un_acc_0 = Rs (acc_0 - Ba) - g;  un_gyr = 0.5 (gyr_0 + gyr) - Bg;  q = ((un_gyr dt) / 2.0, 1), not
 *                       normalised;  Rs = Rs toRotationMatrix(q) (Rs is never re-orthonormalised, as in the reference);
 *                       un_acc_1 = Rs (acc - Ba) - g;  un_acc = 0.5 (un_acc_0 + un_acc_1);
 *                       Ps = Ps + (dt Vs + ((0.5 dt) dt) un_acc);  Vs = Vs + dt un_acc
 *   matrix -> quaternion  Eigen's Quaterniond(Matrix3d): t = (m00 + m11) + m22; if t > 0: t = sqrt(t + 1), w = 0.5 t, t = 0.5 / t,
 *                       x = (m21 - m12) t, y = (m02 - m20) t, z = (m10 - m01) t; else i = the largest diagonal (i = 0; if m11 > m00
 *                       i = 1; if m22 > m_ii i = 2), j = (i + 1) % 3, k = (j + 1) % 3, t = sqrt(m_ii - m_jj - m_kk + 1), q_i = 0.5 t,
 *                       t = 0.5 / t, w = (m_kj - m_jk) t, q_j = (m_ji + m_ij) t, q_k = (m_ki + m_ik) t.  Not normalised.
 *   R2ypr               y = atan2(R10, R00), p = atan2(-R20, R00 cos y + R10 sin y), r = atan2(R02 sin y - R12 cos y,
 *                       -R01 sin y + R11 cos y); each / pi * 180
 *   double2vector       origin = R2ypr(Rs[0]) and Ps[0] (last_R0 and last_P0 where failure_occur is set, which is cleared);
 *                       R00 = toRotationMatrix(q of pose 0); y_diff = origin.y - R2ypr(R00).y; rot_diff = [c, -s, 0; s, c, 0; 0, 0, 1]
 *                       with c, s = cos, sin(y_diff / 180 * pi); in the singular branch (| |pitch| - 90 | < 1.0 of either)
 *                       rot_diff = Rs[0] R00^T.  Per frame: q / sqrt(((x x + y y) + z z) + w w), Rs = rot_diff toRotationMatrix(q),
 *                       Ps = rot_diff (p_i - p_0) + origin_P0, Vs = rot_diff v, Bas, Bgs and tic copied, ric = toRotationMatrix(q_ext).
 *   failureDetection    norms as sqrt((x x + y y) + z z); gates in source order: |Bas[10]| > 2.5, |Bgs[10]| > 1.0, |Ps[10] - last_P| > 5,
 *                       |Ps[10].z - last_P.z| > 1.  The commented-out gates stay out.
 *   slideWindowOld      marg_R = back_R0 ric, new_R = Rs[0] ric, marg_P = back_P0 + back_R0 tic, new_P = Ps[0] + Rs[0] tic
 * The device's atan2 / sin / cos are not the host's to the last bit; everything else is, so vio_est_update_batch agrees with a host
 * restatement to rounding and the other calls bit for bit.
 *
 * Rules:
 *   - argument errors write nothing and launch nothing for the whole call (VIO_ERR_BAD_ARG, vio_est_last_error names the item): count
 *     outside [0, VIO_EST_MAX_SLOTS], a NULL array, a slot outside [0, VIO_EST_MAX_SLOTS) or listed twice, n < 0 or above
 *     VIO_EST_MAX_SAMPLES, a kind that is neither, a non-finite sample, header, pose, speed-bias or extrinsic;
 *   - rules only the device can check leave that slot exactly as it was, give the slot's result a VIO_EST_STATUS_* and do not touch
 *     the other slots of the call (the call returns VIO_OK): the slot's region would exceed VIO_EST_MAX_SAMPLES;
 *   - repeated calls are bitwise identical, and a slot's result depends neither on the batch nor on the slot index (no atomics, the
 *     orders above);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_EST_H
#define VIO_EST_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_EST_VERSION 1
#define VIO_EST_MAX_SLOTS 256
#define VIO_EST_MAX_SAMPLES 4096                    /* raw samples a slot can hold over its 11 intervals */
#define VIO_EST_WINDOW_SIZE 10                      /* WINDOW_SIZE */
#define VIO_EST_FRAMES 11                           /* WINDOW_SIZE + 1 */

/* A slot's status in a result: a rule only the device can check; the slot is as it was. */
#define VIO_EST_STATUS_OK 0
#define VIO_EST_STATUS_POOL_FULL 1                  /* the run would not fit into VIO_EST_MAX_SAMPLES samples */

#define VIO_EST_MARG_OLD 0                          /* MARGIN_OLD */
#define VIO_EST_MARG_SECOND_NEW 1                   /* MARGIN_SECOND_NEW */

#define VIO_EST_GATE_NONE 0                         /* failureDetection's verdict: the first gate that fires, in source order */
#define VIO_EST_GATE_BA 1                           /* |Bas[10]| > 2.5 */
#define VIO_EST_GATE_BG 2                           /* |Bgs[10]| > 1.0 */
#define VIO_EST_GATE_TRANSLATION 3                  /* |Ps[10] - last_P| > 5 */
#define VIO_EST_GATE_Z 4                            /* |Ps[10].z - last_P.z| > 1 */

typedef struct vio_est vio_est;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own.  Every slot starts as
 * vio_est_reset leaves it under the default config. */
vio_status vio_est_create(int32_t device, void *stream, vio_est **out);
void vio_est_destroy(vio_est *h);
const char *vio_est_last_error(const vio_est *h);          /* valid until the next call on h */
int32_t vio_est_version(void);

/* setParameter's inputs and the IMU noise of the pre-integrations.  Default: tic = 0, ric = identity, g = (0, 0, 9.81), noise
 * (0.2687, 0.2121, 7.07e-6, 7.07e-7), the project's synthetic defaults.  Everything finite. */
typedef struct vio_est_config {
    double tic[3];
    double ric[4];                  /* quaternion (x, y, z, w); the slot's ric is its toRotationMatrix, not normalised */
    double g[3];
    double noise[4];                /* acc_n, gyr_n, acc_w, gyr_w, as vio_imu_noise */
} vio_est_config;
vio_status vio_est_set_config(vio_est *h, const vio_est_config *cfg);

/* One slot's state without its samples.  An IntegrationBase (interval j, the samples between frames j - 1 and j) is its existence,
 * the (acc_0, gyr_0) and the linearisation biases it was constructed with. */
typedef struct vio_est_state {
    int32_t frame_count;            /* in [0, 10] */
    int32_t first_imu;              /* 0 / 1 */
    int32_t failure_occur;          /* 0 / 1 */
    int32_t reserved;
    int32_t exists[12];             /* [j] for j in [0, 10]: pre_integrations[j] != nullptr; [11] is 0 */
    double Ps[11][3];
    double Rs[11][9];
    double Vs[11][3];
    double Bas[11][3];
    double Bgs[11][3];
    double Headers[11];
    double tic[3];
    double ric[9];
    double g[3];
    double acc_0[3];
    double gyr_0[3];
    double first[11][6];            /* acc_0 | gyr_0 interval j was constructed with */
    double lin_bias[11][6];         /* Ba | Bg interval j was constructed with */
    double last_R[9];
    double last_P[3];
    double last_R0[9];
    double last_P0[3];
} vio_est_state;

/* clearState + setParameter of one slot: Rs identity, Ps / Vs / Bas / Bgs zero, no interval and no sample, first_imu, frame_count and
 * failure_occur 0, tic / ric / g from the config.  What clearState leaves alone stays: Headers, acc_0 / gyr_0 and
 * last_R / last_P / last_R0 / last_P0.  (clearState does clear failure_occur, at :98; a caller that reboots after a failure and wants
 * double2vector's last_R0 branch sets the flag again through vio_est_state_set.)  Waits. */
vio_status vio_est_reset(vio_est *h, int32_t slot);

/* One slot's whole state as plain arrays.  off: 12 entries, off[0] = 0, non-decreasing, off[11] <= VIO_EST_MAX_SAMPLES; interval j has
 * samples [off[j], off[j + 1]) of dt / acc (x 3) / gyr (x 3).  _set refuses (VIO_ERR_BAD_ARG, nothing written) frame_count outside
 * [0, 10], flags other than 0 / 1, samples in an interval behind frame_count or in one that does not exist, and anything non-finite.
 * _get needs room for cap_samples >= off[11] samples, else VIO_ERR_BAD_ARG with off written (so the caller can size the arrays);
 * dt / acc / gyr may be NULL when the slot has no samples.  Both wait. */
vio_status vio_est_state_set(vio_est *h, int32_t slot, const vio_est_state *state, const int64_t *off, const double *dt,
                             const double *acc, const double *gyr);
vio_status vio_est_state_get(vio_est *h, int32_t slot, vio_est_state *state, int64_t cap_samples, int64_t *off, double *dt, double *acc,
                             double *gyr);

/* What every batched call returns per item.  The fields after frame_count belong to one call each and are 0 in the others. */
typedef struct vio_est_result {
    int32_t status;                 /* VIO_EST_STATUS_* */
    int32_t frame_count;            /* the slot's frame_count after the call */
    int32_t n_samples;              /* imu, slide: samples the slot holds after the call */
    int32_t failure;                /* update: failureDetection's return */
    int32_t gate;                   /* update: VIO_EST_GATE_* */
    int32_t singular;               /* update: double2vector took the singular branch */
    int32_t slid;                   /* slide: 1 where frame_count == WINDOW_SIZE, 0 where nothing happened */
    int32_t shift_depth;            /* slide, MARG_OLD: the item's nonlinear flag (slideWindowOld's shift_depth) */
    double marg_R[9];               /* slide, MARG_OLD: the four arrays vio_fm_slide_item takes */
    double marg_P[3];
    double new_R[9];
    double new_P[3];
} vio_est_result;

/* processIMU for samples 0 .. n - 1 in order.  n = 0 does nothing. */
typedef struct vio_est_imu_item {
    int32_t slot;
    int32_t n;                      /* in [0, VIO_EST_MAX_SAMPLES] */
    const double *dt;               /* [n] */
    const double *acc;              /* [n][3] linear_acceleration */
    const double *gyr;              /* [n][3] angular_velocity */
} vio_est_imu_item;
vio_status vio_est_imu_batch(vio_est *h, int32_t count, const vio_est_imu_item *items, vio_est_result *results);

/* The state part of processImage: Headers[frame_count] = header; then frame_count++ if `advance` and frame_count < WINDOW_SIZE. */
typedef struct vio_est_image_item {
    int32_t slot;
    int32_t advance;
    double header;
} vio_est_image_item;
vio_status vio_est_image_batch(vio_est *h, int32_t count, const vio_est_image_item *items, vio_est_result *results);

/* vector2double and the pre-integrations of intervals 1 .. 10 (preint[j - 1] is interval j: frame j - 1 to frame j), each recomputed
 * from its resident samples at its own construction biases and (acc_0, gyr_0).  An interval that does not exist or has no samples
 * gives the empty record of vio_imu.h: sum_dt = 0, delta_q identity, jacobian I, covariance 0 (linearised biases as constructed, 0
 * where the interval does not exist).  poses / speed_bias / ext are what vio_set_window takes, preint what vio_set_imu_all takes. */
typedef struct vio_est_window_item {
    int32_t slot;
    int32_t reserved;
    double *poses;                  /* [11][7] */
    double *speed_bias;             /* [11][9] */
    double *ext;                    /* [7] */
    vio_preint *preint;             /* [10] */
} vio_est_window_item;
vio_status vio_est_window_batch(vio_est *h, int32_t count, const vio_est_window_item *items, vio_est_result *results);

/* double2vector from the solved arrays, then failureDetection.  failure == 0 and commit_last: last_R / last_P / last_R0 / last_P0 =
 * Rs[10] / Ps[10] / Rs[0] / Ps[0] (:234-237).  failure == 1: the slot is left updated with failure_occur = 1; the caller decides to
 * vio_est_reset.  The three outputs (each may be NULL) are vector2double of the updated state, the re-anchored arrays the
 * marginalisation takes (estimator.cpp:1086-1102), so that a frame needs no second vio_est_window_batch. */
typedef struct vio_est_update_item {
    int32_t slot;
    int32_t commit_last;
    const double *poses;            /* [11][7] */
    const double *speed_bias;       /* [11][9] */
    const double *ext;              /* [7] */
    double *poses_out;              /* [11][7] or NULL */
    double *speed_bias_out;         /* [11][9] or NULL */
    double *ext_out;                /* [7] or NULL */
} vio_est_update_item;
vio_status vio_est_update_batch(vio_est *h, int32_t count, const vio_est_update_item *items, vio_est_result *results);

/* slideWindow.  Nothing happens unless frame_count == WINDOW_SIZE (result.slid says).  VIO_EST_MARG_OLD: states and intervals shift
 * down by one, state 10 stays (a copy of the old frame 10), interval 10 is constructed anew from acc_0, gyr_0, Bas[10], Bgs[10], the
 * dropped interval's samples leave the region; the result carries slideWindowOld's four arrays.  VIO_EST_MARG_SECOND_NEW: interval
 * 10's samples are appended to interval 9, state 9 becomes state 10, interval 10 is constructed anew. */
typedef struct vio_est_slide_item {
    int32_t slot;
    int32_t kind;                   /* VIO_EST_MARG_OLD / VIO_EST_MARG_SECOND_NEW */
    int32_t nonlinear;              /* solver_flag == NON_LINEAR: returned as shift_depth */
    int32_t reserved;
} vio_est_slide_item;
vio_status vio_est_slide_batch(vio_est *h, int32_t count, const vio_est_slide_item *items, vio_est_result *results);

/* ms of the last batched call that launched: host checks, packing and upload (host clock); the kernels (HIP events); the read-back
 * (HIP events); the whole call (host clock). */
vio_status vio_est_timing(const vio_est *h, double *out4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
