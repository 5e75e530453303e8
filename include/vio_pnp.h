/*
 * vio_pnp.h — batched PnP of the non-keyframes for the initialisation on the GPU (companion library libvio_pnp_hip.so).
 *
 * The step of Estimator::initialStructure between the global SfM and the visual-inertial alignment (VM/src/estimator.cpp:308-374): the
 * cv::solvePnP of every frame of all_image_frame that is not a keyframe, from the points the SfM triangulated (sfm_tracked_points)
 * and the pose of the next keyframe as the guess, for `count` independent windows in one call:
 *   vio_pnp_frames_batch          every non-keyframe of every window, one wavefront per frame                  (k_pnp_frames)
 * Its inputs are what vio_sfm_batch (include/vio_sfm.h) gives, its outputs are what vio_init_item (include/vio_init.h) takes for the
 * frames with is_key = 0.  It works from host arrays and needs nothing from libvio_hip but the vio_status type.  DESIGN.md section 18
 * has the math, the layout and the measurements.
 *
 * Flat problems are the same call: a caller that only wants many independent PnPs passes valid = NULL, obs_point = 0, 1, 2, ... and
 * one keyframe pose per frame as its guess.
 *
 * The reference does the solve with OpenCV.  What replaces it, so that the work is fixed and repeatable (not compared against
 * OpenCV, which is not a dependency; tests/pnp_reference.py restates it in numpy and the device is held to that):
 *   - cv::solvePnP(pts_3_vector, pts_2_vector, K = I, D, rvec, t, useExtrinsicGuess = 1): the Levenberg-Marquardt solve of
 *     include/vio_sfm.h on (a left-multiplied rotation-vector increment, t) from the guess, with Ceres' trust-region rule: step
 *     (J^T J + D / radius) d = -g with D = diag(J^T J) clamped to [1e-6, 1e32], initial radius VIO_SFM_LM_INITIAL_RADIUS;
 *     rho = cost change / model change; a step with rho > 1e-3 is taken and radius = min(radius / max(1/3, 1 - (2 rho - 1)^3), 1e16);
 *     otherwise radius /= v, v *= 2 (v = 2 after a step taken).  At most VIO_SFM_PNP_MAX_ITER iterations, every one counts, taken or
 *     not; it stops when |step| <= VIO_SFM_PNP_STEP_TOL, when the gradient's largest entry is at most VIO_SFM_BA_GRADIENT_TOL, or
 *     when the radius falls below 1e-32.  The constants are those of include/vio_sfm.h, which this header includes.
 *   - the guess: R = Q[g]^-1 (the transposed rotation matrix of the quaternion as given), t = -R T[g] with g = guess_key[frame]
 *     (estimator.cpp:328-329).  The result: Q = Quaternion(R^T), T = -R^T t, which are R_pnp and T_pnp of estimator.cpp:365-371
 *     before the RIC[0]^T factor, in the convention of vio_sfm_result.
 *   - double throughout, where the reference rounds the points to cv::Point3f / cv::Point2f.
 *   - fewer than min_points usable points fail the frame (estimator.cpp:355: 6).
 *
 * The order of the sums is part of this contract.  A frame's usable points are its observations whose point is valid, in the order
 * of the observations (an observation whose point is not valid is skipped, as a key missing from sfm_tracked_points is).  They are
 * listed inside the kernel by a wave prefix count: the observations are taken 64 at a time, a ballot of the valid ones and the count
 * of set bits below each lane give every usable point its rank.  Usable point m belongs to lane m mod 64.  Each lane sums its
 * points' terms (the 21 entries of the upper triangle of J^T J, the 6 of J^T r, and r^2) in ascending order from 0.0 into 28 private
 * accumulators; the 28 values are then reduced across the 64 lanes by the butterfly v[i] += v[i ^ s] for s = 1, 2, 4, 8, 16, 32.
 * IEEE addition is commutative, so every lane ends with the same bits, and every lane runs the 6 x 6 solve and the LM decision on
 * them.  The order depends neither on how many wavefronts share a workgroup nor on which frames share one.
 *
 * Rules (those of include/vio_sfm.h):
 *   - argument errors (count < 0, a NULL array, n_frames outside [0, VIO_PNP_MAX_FRAMES], a negative n_points or n_key, a
 *     guess_key outside [0, n_key), an obs_offset that does not start at 0 or decreases, a frame with more than VIO_PNP_MAX_POINTS
 *     observations, an obs_point outside [0, n_points)) write nothing and launch nothing: VIO_ERR_BAD_ARG, vio_pnp_last_error names
 *     the window.  count == 0 does nothing and returns VIO_OK;
 *   - a window whose inputs or results are not finite gets VIO_ERR_NOT_FINITE (all of its frames' outputs NaN); the others are
 *     computed as if it were not there, and the call returns VIO_ERR_NOT_FINITE.  The inputs that count are those a frame reads: its
 *     observations' image points, the coordinates of its usable points, and its guess pose.  (The coordinates of a point that is not
 *     valid are not read: vio_sfm_batch leaves them NaN.)  A frame that fails one of the reference's tests gets one of the
 *     VIO_PNP_FAIL_* codes below; that is an outcome, not an error (the call returns VIO_OK).  The frames after a failing one are
 *     still computed and reported;
 *   - repeated calls are bitwise identical, and a frame's result depends neither on the batch nor on the window it is in (no
 *     floating-point atomics, the summation order above);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_PNP_H
#define VIO_PNP_H

#include "vio_backend.h"
#include "vio_sfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_PNP_VERSION 1
#define VIO_PNP_MAX_FRAMES 32                       /* non-keyframes per window: VIO_INIT_MAX_FRAMES bounds all_image_frame */
#define VIO_PNP_MAX_POINTS 4096                     /* observations per frame, as VIO_SFM_MAX_TRACKS */
#define VIO_PNP_DEFAULT_MIN_POINTS 6                /* estimator.cpp:355 */

/* Per-frame and per-window outcomes besides VIO_OK and VIO_ERR_NOT_FINITE. */
#define VIO_PNP_FAIL_FEW_POINTS 1       /* fewer than min_points usable points ("Not enough points for solve pnp !") */
#define VIO_PNP_FAIL_NO_POSE 2          /* solvePnP's false: the cost at the guess is not finite (a point in the guess camera's
                                           z = 0 plane, or an overflow), so the solve cannot start */

typedef struct vio_pnp vio_pnp;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_pnp_create(int32_t device, void *stream, vio_pnp **out);
void vio_pnp_destroy(vio_pnp *h);
const char *vio_pnp_last_error(const vio_pnp *h);          /* valid until the next call on h */
int32_t vio_pnp_version(void);

typedef struct vio_pnp_config {
    int32_t min_points;             /* in [3, VIO_PNP_MAX_POINTS]; default VIO_PNP_DEFAULT_MIN_POINTS */
    int32_t reserved;
} vio_pnp_config;
vio_status vio_pnp_set_config(vio_pnp *h, const vio_pnp_config *cfg);

/* One window: the SfM's points and keyframe poses, and the observations of its non-keyframes. */
typedef struct vio_pnp_item {
    int32_t n_points;               /* sfm_tracked_points: vio_sfm_batch's points / state of the window */
    int32_t n_key;
    int32_t n_frames;               /* the non-keyframes to solve, in [0, VIO_PNP_MAX_FRAMES] */
    int32_t reserved;
    const double *points;           /* [n_points][3], in frame l */
    const uint8_t *valid;           /* [n_points], or NULL: every point is valid */
    const double *key_Q;            /* [n_key][4] (w, x, y, z): the keyframes' camera poses in frame l, as vio_sfm_result's Q */
    const double *key_T;            /* [n_key][3] */
    const int32_t *guess_key;       /* [n_frames]: the keyframe whose pose is the frame's guess (the next keyframe in time) */
    const int64_t *obs_offset;      /* [n_frames + 1]: frame k's observations are obs_point / obs_pts [obs_offset[k] ..
                                       obs_offset[k + 1]), at most VIO_PNP_MAX_POINTS of them */
    const int32_t *obs_point;       /* [obs_offset[n_frames]]: an index into points */
    const double *obs_pts;          /* [obs_offset[n_frames]][2] normalised image points */
} vio_pnp_item;

typedef struct vio_pnp_result {
    int32_t status;                 /* VIO_OK, the first failing frame's VIO_PNP_FAIL_*, or VIO_ERR_NOT_FINITE */
    int32_t fail_frame;             /* the first failing frame in the item's order (the reference returns false there), else -1 */
} vio_pnp_result;

typedef struct vio_pnp_frame_info {
    int32_t status;                 /* VIO_OK, VIO_PNP_FAIL_*, VIO_ERR_NOT_FINITE (then for every frame of the window) */
    int32_t iterations;             /* of the LM, taken or not */
    int32_t n_used;                 /* usable points */
    int32_t reserved;
    double cost;                    /* half the sum of squared residuals at the result (NaN unless VIO_OK) */
} vio_pnp_frame_info;

/* res: [count].  Q: [sum of n_frames][4] (w, x, y, z), T: [sum of n_frames][3] (NaN unless the frame's status is VIO_OK),
 * frame_info: [sum of n_frames] or NULL; window i's part starts at the sum of the n_frames before it. */
vio_status vio_pnp_frames_batch(vio_pnp *h, int32_t count, const vio_pnp_item *items, vio_pnp_result *res, double *Q, double *T,
                                vio_pnp_frame_info *frame_info);

/* ms of the last call that launched: host packing + upload, k_pnp_frames (HIP events), the whole call. */
vio_status vio_pnp_timing(const vio_pnp *h, double *out3);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
