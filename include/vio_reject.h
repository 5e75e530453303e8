/*
 * vio_reject.h — batched rejectWithF and undistortedPoints on the GPU (companion library libvio_reject_hip.so).
 *
 * The camera-model half of FeatureTracker::readImage (VM/src/feature_tracker.cpp), for `count` independent streams in one call:
 *   vio_reject_batch             rejectWithF (feature_tracker.cpp:169-202): both point sets lifted, RANSAC on the fundamental matrix,
 *                                the mask of the pairs to keep                                              (k_reject_ransac)
 *   vio_reject_undistort_batch   undistortedPoints (feature_tracker.cpp:258-306): the normalised points and their velocities against
 *                                the previous frame's, matched by id                                        (k_reject_lift)
 *   vio_reject_lift              the bare lift of one point set, in double                                  (k_reject_lift)
 * It works from host arrays and needs nothing from libvio_hip but the vio_status type.  DESIGN.md section 21 has the layout and the
 * measurements.  tests/reject_reference.py restates all of it in numpy.
 *
 * Camera.  The reference's PINHOLE model (VM/src/camera_models/camera_models/PinholeCamera.cc), the one both of its configurations
 * use (VM/config/euroc_config.yaml:9, VM/config/vio_simulation.yaml:9): fx, fy, cx, cy, the radial k1, k2 and the tangential p1, p2.
 * The other camodocal models (KANNALA_BRANDT, MEI, SCARAMUZZA) are refused with VIO_ERR_BAD_ARG: include/vio_camera.h
 * (libvio_camera_hip.so) is the same two stages through all four.
 *
 * Lift.  PinholeCamera::liftProjective (PinholeCamera.cc:461-521) with PinholeCamera::distortion (:657-673), in double:
 *       mx_d = (1 / fx) u + (-cx / fx),  my_d = (1 / fy) v + (-cy / fy)                       (m_inv_K11 .. m_inv_K23, divided once)
 *   if k1 = k2 = p1 = p2 = 0 (m_noDistortion) that is the result.  Otherwise the "recursive distortion model":
 *       m_u = m_d - d(m_d), then VIO_REJECT_LIFT_EVALUATIONS - 1 = 7 more rounds of m_u = m_d - d(m_u)   (n = 8: eight evaluations of d)
 *       d(x, y): x2 = x x, y2 = y y, xy = x y, r2 = x2 + y2, rad = k1 r2 + (k2 r2) r2,
 *                dx = (x rad + (2 p1) xy) + p2 (r2 + 2 x2),  dy = (y rad + (2 p2) xy) + p1 (r2 + 2 y2)
 *   in the reference's operation order, every product and sum rounded on its own (contraction off).  The device, the host build of
 *   csrc/vio_reject_math.h and the restatement agree in every bit.  z is 1, so x / z and y / z are x and y.
 *
 * vio_reject_batch.  For one pair: n matched points cur_pts, forw_pts (pixels, float) and `pair`, which enters the sampling hash where
 * the structure-from-motion passes its candidate frame (the tracker passes the count of frames read).
 *   - n < 8: nothing runs (the reference's size gate, feature_tracker.cpp:171): the mask is all ones, VIO_OK, hyp = -1, F is NaN.
 *   - Both sets are lifted and mapped to focal_length x + width / 2.0, focal_length y + height / 2.0 (:180-187), then rounded to
 *     float: the reference stores them as cv::Point2f, and that is kept.  The fit and the scores are in double on those values.
 *   - cv::findFundamentalMat(FM_RANSAC, F_THRESHOLD, 0.99) is replaced by the RANSAC of include/vio_sfm.h, word for word:
 *     ransac_hypotheses fixed hypotheses; draw k of hypothesis h by hash(seed, pair, h, k) % (n - k) (sample8); the normalised 8-point
 *     model with rank 2 enforced; score: the larger of the two squared point-to-epipolar-line distances <= f_threshold^2; winner: most
 *     inliers, ties to the lowest h; one refit on the winner's inliers if there are at least 8; then the final mask.  Every symmetric
 *     eigenproblem is the cyclic Jacobi iteration of VIO_SFM_JACOBI_SWEEPS sweeps.
 *   - No hypothesis reaches 8 inliers, or the refit is not finite: VIO_REJECT_FAIL_NO_MODEL, the mask is all ones, F is NaN, hyp is the
 *     winner.  Deviation: OpenCV returns an empty matrix there and leaves `status` in a state reduceVector then reads out of bounds
 *     (feature_tracker.cpp:193-198).  A tracker must not lose every track to one degenerate pair, so every pair is kept.
 *   - A point that is not finite: VIO_ERR_NOT_FINITE for that pair alone (mask all zeros, hyp = -1, F NaN); the others are computed
 *     as if it were not there, and the call returns VIO_ERR_NOT_FINITE.
 *   n_inliers is the number of ones in the mask.  Other deviations from OpenCV: a fixed hypothesis count instead of the adaptive
 *   one, counter-based sampling instead of cv::RNG, the 8-point instead of the 7-point minimal model, no degeneracy test of a sample.
 *
 * k_reject_ransac's LDS.  A hypothesis is fitted out of its 9 x 9 normal matrix and the 9 x 9 eigenvectors: 162 doubles.  They live in
 * LDS, entry-major and lane-minor (entry e of lane l at double e * VIO_REJECT_ROUND + l), so consecutive lanes touch consecutive
 * doubles: an 8-byte access of 32 lanes covers all 64 banks once.  162 * 8 * ROUND bytes: 41 472 at ROUND = 32, 82 944 at 64,
 * 165 888 at 128, which is beyond the CU's 163 840.  ROUND = 64 is one full wavefront per round and the largest that fits; with the
 * round's F (4 608 B), the counters and the refit's statistics a workgroup declares 88 048 B, and the compiler adds 18 432 B (a
 * 9-double array per thread that it keeps in LDS instead of scratch): 106 480 B, so one workgroup runs per CU.  Three of ROUND = 32
 * would fit a CU, but a half-filled wavefront fits no faster than a full one and the kernel's registers allow one wavefront per SIMD.
 * The workgroup has VIO_REJECT_THREADS = 256 threads: one wavefront fits, all four score (hypothesis, correspondence) pairs, lift
 * and write the masks.
 *
 * vio_reject_undistort_batch.  For one item: n points pts with ids (-1: a new point), the previous frame's m ids prev_ids with their
 * normalised points prev_un_pts, and dt = cur_time - prev_time.  un_pts[i] = the lift's (x / z, y / z) rounded to float
 * (feature_tracker.cpp:268).  velocity[i] = (un_pts[i] - prev_un_pts[j]) / dt, computed in double from the float values and rounded to
 * float, where j is the first entry of prev_ids equal to ids[i], if ids[i] != -1 and there is one (:279-288); (0, 0) otherwise, and
 * for every point when m == 0 (:298-303).  With m > 0, dt must be finite and > 0.  (Deviation: the reference subtracts the two
 * cv::Point2f coordinates in float before the division; here the difference is exact.)
 * Kept quirk: undistortedPoints runs before updateID, so a point detected in frame t still carries id -1 when its first normalised
 * point is stored; in frame t + 1 it has its id, but the previous frame's list holds it under -1 and nothing matches.  Its velocity
 * is zero in its first two frames.  The caller passes prev_ids as they were at that moment.
 * An item with a point that is not finite gets VIO_ERR_NOT_FINITE, un_pts and velocity NaN.
 *
 * Rules (those of include/vio_detect.h):
 *   - argument errors (count outside [0, VIO_REJECT_MAX_ITEMS], a NULL array, n or m outside [0, VIO_REJECT_MAX_POINTS], no camera set, dt not finite or <= 0 with
 *     m > 0) write nothing and launch nothing: VIO_ERR_BAD_ARG, vio_reject_last_error names the item.  count == 0 returns VIO_OK;
 *   - repeated calls are bitwise identical, and an item's result does not depend on the batch it is in (no floating-point atomics,
 *     fixed summation orders, sampling by counter);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_REJECT_H
#define VIO_REJECT_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_REJECT_VERSION 1
#define VIO_REJECT_MAX_POINTS 4096                  /* per pair / per item; VIO_DETECT_MAX_POINTS */
#define VIO_REJECT_MAX_ITEMS 4096                   /* pairs or items per call */
#define VIO_REJECT_MAX_HYPOTHESES 4096              /* VIO_SFM_MAX_HYPOTHESES */
#define VIO_REJECT_DEFAULT_HYPOTHESES 128           /* VIO_SFM_DEFAULT_HYPOTHESES */
#define VIO_REJECT_DEFAULT_F_THRESHOLD 1.0          /* F_THRESHOLD, in virtual pixels */
#define VIO_REJECT_DEFAULT_FOCAL_LENGTH 460.0       /* FOCAL_LENGTH */
#define VIO_REJECT_LIFT_EVALUATIONS 8               /* of the distortion, PinholeCamera.cc:503 */
#define VIO_REJECT_MIN_POINTS 8                     /* the size gate, and the inliers a model needs */
#define VIO_REJECT_ROUND 64                         /* hypotheses fitted at once by k_reject_ransac (for the tests' shapes) */
#define VIO_REJECT_THREADS 256                      /* the workgroup of k_reject_ransac and of k_reject_lift */
#define VIO_REJECT_ID_CHUNK 1024                    /* prev_ids staged through LDS by k_reject_lift */

#define VIO_REJECT_MODEL_PINHOLE 0
#define VIO_REJECT_MODEL_KANNALA_BRANDT 1           /* refused here: include/vio_camera.h */
#define VIO_REJECT_MODEL_MEI 2                      /* refused here: include/vio_camera.h */
#define VIO_REJECT_MODEL_SCARAMUZZA 3               /* refused here: include/vio_camera.h */

/* Per-pair outcome besides VIO_OK and VIO_ERR_NOT_FINITE. */
#define VIO_REJECT_FAIL_NO_MODEL 1

typedef struct vio_reject vio_reject;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_reject_create(int32_t device, void *stream, vio_reject **out);
void vio_reject_destroy(vio_reject *h);
const char *vio_reject_last_error(const vio_reject *h);    /* valid until the next call on h */
int32_t vio_reject_version(void);

typedef struct vio_reject_camera {
    double fx, fy, cx, cy;          /* fx, fy finite and not 0 */
    double k1, k2, p1, p2;          /* all 0: no distortion */
    int32_t width, height;          /* COL, ROW: >= 1 */
    int32_t model;                  /* VIO_REJECT_MODEL_PINHOLE */
    int32_t reserved;               /* 0 */
} vio_reject_camera;
vio_status vio_reject_set_camera(vio_reject *h, const vio_reject_camera *cam);

typedef struct vio_reject_config {
    uint32_t seed;                  /* of the sampling hash; default 0 */
    int32_t ransac_hypotheses;      /* in [1, VIO_REJECT_MAX_HYPOTHESES] */
    double f_threshold;             /* > 0, virtual pixels */
    double focal_length;            /* > 0 */
} vio_reject_config;
vio_status vio_reject_set_config(vio_reject *h, const vio_reject_config *cfg);

typedef struct vio_reject_item {
    int32_t n;                      /* in [0, VIO_REJECT_MAX_POINTS] */
    uint32_t pair;                  /* enters the sampling hash */
    const float *cur_pts;           /* [n][2] pixels; may be NULL with n == 0 */
    const float *forw_pts;          /* [n][2] */
} vio_reject_item;

typedef struct vio_reject_result {
    int32_t status;                 /* VIO_OK, VIO_REJECT_FAIL_NO_MODEL, VIO_ERR_NOT_FINITE */
    int32_t hyp;                    /* the winning hypothesis, -1 if none ran */
    int32_t n_inliers;              /* the ones of the mask */
    int32_t reserved;
    double F[9];                    /* row-major, x_forw^T F x_cur = 0 in virtual pixels (NaN unless VIO_OK with n >= 8) */
} vio_reject_result;

/* mask: [sum of n]; pair i's part starts at the sum of the n before it; 1: keep. */
vio_status vio_reject_batch(vio_reject *h, int32_t count, const vio_reject_item *items, vio_reject_result *results, uint8_t *mask);

typedef struct vio_reject_undistort_item {
    int32_t n, m;                   /* in [0, VIO_REJECT_MAX_POINTS] */
    const float *pts;               /* [n][2] pixels */
    const int64_t *ids;             /* [n], -1: a new point */
    const int64_t *prev_ids;        /* [m] */
    const float *prev_un_pts;       /* [m][2] */
    double dt;                      /* finite and > 0 when m > 0 */
    float *un_pts;                  /* out [n][2] */
    float *velocity;                /* out [n][2] */
} vio_reject_undistort_item;

/* status: [count], VIO_OK or VIO_ERR_NOT_FINITE per item. */
vio_status vio_reject_undistort_batch(vio_reject *h, int32_t count, const vio_reject_undistort_item *items, int32_t *status);

/* The lift alone: out[n][2] doubles (x, y) of n points pts[n][2]; n in [0, VIO_REJECT_MAX_POINTS].  Points that are not finite
 * give what the arithmetic gives. */
vio_status vio_reject_lift(vio_reject *h, int32_t n, const float *pts, double *out);

/* ms of the last call that launched: host packing + upload, the kernel (HIP events), the whole call. */
vio_status vio_reject_timing(const vio_reject *h, double *out3);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
