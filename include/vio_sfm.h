/*
 * vio_sfm.h — batched structure-from-motion for the initialisation on the GPU (companion library libvio_sfm_hip.so).
 *
 * The vision half of the reference's initialisation (Estimator::initialStructure, VM/src/estimator.cpp:224-382) for `count`
 * independent windows in one call; its output feeds the alignment half (include/vio_init.h):
 *   vio_sfm_relative_pose_batch   Estimator::relativePose (estimator.cpp:462-491) with MotionEstimator::solveRelativeRT
 *                                 (VM/src/initial/solve_5pts.cpp:193-226)                                   (k_sfm_relpose)
 *   vio_sfm_construct_batch       GlobalSFM::construct (VM/src/initial/initial_sfm.cpp:121-313): the PnP / triangulation chains in
 *                                 its order, then the full bundle adjustment                               (k_sfm_construct)
 *   vio_sfm_batch                 both, without a host round trip in between
 * The PnP of the non-keyframes of all_image_frame (estimator.cpp:320-373) is include/vio_pnp.h's, not this library's.  It works from host arrays
 * and needs nothing from libvio_hip but the vio_status type.  DESIGN.md section 16 has the math, the layout and the measurements.
 *
 * The reference does this part with OpenCV and Ceres.  What replaces them, so that the work is fixed and repeatable:
 *   - cv::findFundamentalMat(FM_RANSAC, 0.3 / 460, 0.99): RANSAC with a fixed number of hypotheses (vio_sfm_config) over the
 *     normalised 8-point model (Hartley scaling of each point set to mean distance sqrt 2, the smallest eigenvector of the 9 x 9
 *     normal matrix, rank 2 enforced by removing the smallest singular direction).  Score: the larger of the two squared
 *     point-to-epipolar-line distances against (0.3 / 460)^2; winner: most inliers, ties to the lowest hypothesis; one refit on the
 *     winner's inliers (at least 8), then the final mask.  Sampling is counter-based.  With
 *         mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16            (uint32 arithmetic)
 *         hash(seed, i, h, k) = mix(mix(mix(mix(seed + 0x9e3779b9) + i) + h) + k)
 *     draw k = 0 .. 7 of hypothesis h of candidate frame i over n correspondences takes r = hash(seed, i, h, k) % (n - k) and picks
 *     the r-th index (from 0, ascending) that draws 0 .. k-1 have not taken.  Correspondences are in track order.
 *   - cv::recoverPose: the SVD of E, the four (R, t) candidates in the order (R1, t), (R2, t), (R1, -t), (R2, -t), each scored by
 *     triangulating the inliers (depth in (0, 50) in both views); the first candidate with the most points wins; success iff that
 *     count > 12.  relative_R = R^T, relative_T = -R^T t (solve_5pts.cpp:218-219).
 *   - cv::solvePnP(useExtrinsicGuess): Levenberg-Marquardt on (a left-multiplied rotation-vector increment, t) from the guess, at
 *     most VIO_SFM_PNP_MAX_ITER iterations, stopping when |step| <= VIO_SFM_PNP_STEP_TOL or the gradient's largest entry is at
 *     most VIO_SFM_BA_GRADIENT_TOL.  Fewer than 10 points fail, as in the reference.
 *   - the Ceres solve (DENSE_SCHUR, no loss function): Levenberg-Marquardt over every frame's rotation (3-dof increment,
 *     left-multiplied) and translation and every triangulated point; constant: the rotation of frame l, the translations of l and of
 *     F-1.  Points are eliminated by a Schur complement; the 6F x 6F reduced system (constant parameters as identity rows) is
 *     factorised by Cholesky in LDS.  Both LMs use Ceres' trust-region rule: step (J^T J + D / radius) d = -g with
 *     D = diag(J^T J) clamped to [1e-6, 1e32]; rho = cost change / model change; a step with rho > 1e-3 is taken and
 *     radius = min(radius / max(1/3, 1 - (2 rho - 1)^3), 1e16); otherwise radius /= v, v *= 2 (v = 2 after a step taken).  Every
 *     iteration counts, taken or not.  Convergence: Ceres' three tests with the constants below.  Success iff converged or the final
 *     cost (half the sum of squares) < 5e-3, as initial_sfm.cpp:283.  The reference's 0.2 s wall-clock limit has no counterpart.
 *   - every symmetric eigenproblem (9 x 9, 4 x 4 triangulation, 3 x 3) is a cyclic Jacobi iteration of VIO_SFM_JACOBI_SWEEPS sweeps.
 *
 * Rules:
 *   - argument errors (count < 0, a NULL array, n_frames outside [3, VIO_SFM_MAX_FRAMES], n_tracks outside [0, VIO_SFM_MAX_TRACKS],
 *     a track that leaves the window, a stage-1 result with l outside the window) write nothing and launch nothing:
 *     VIO_ERR_BAD_ARG, vio_sfm_last_error names the window.  count == 0 does nothing and returns VIO_OK;
 *   - a window whose inputs or results are not finite gets VIO_ERR_NOT_FINITE (its outputs NaN); the others are computed as if it
 *     were not there, and the call returns VIO_ERR_NOT_FINITE.  A window that fails one of the reference's tests gets one of the
 *     VIO_SFM_FAIL_* codes below; that is an outcome, not an error (the call returns VIO_OK);
 *   - repeated calls are bitwise identical, and a window's result does not depend on the batch it is in (no floating-point atomics,
 *     fixed summation orders, sampling by counter);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_SFM_H
#define VIO_SFM_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_SFM_VERSION 1
/* F: k_sfm_construct keeps the packed lower triangle of the 6F x 6F reduced BA system and its vectors in LDS, 8 (18 F^2 + 87 F)
 * bytes: 25 KB at F = 11 (WINDOW_SIZE + 1), 48 KB at F = 16, 170 KB at F = 32, which is beyond the CU's 160 KB.  At 16 three
 * workgroups' LDS fits a CU, so the kernel's registers (two workgroups per CU), not LDS, bound the occupancy.  The LDS of a launch
 * is sized by the largest F of the batch: that changes how many windows share a CU, never a window's result. */
#define VIO_SFM_MAX_FRAMES 16
#define VIO_SFM_MAX_TRACKS 4096                     /* per window (the reference's NUM_OF_F is 1000) */
#define VIO_SFM_MAX_HYPOTHESES 4096
#define VIO_SFM_DEFAULT_HYPOTHESES 128

#define VIO_SFM_JACOBI_SWEEPS 10
#define VIO_SFM_PNP_MAX_ITER 20
#define VIO_SFM_PNP_STEP_TOL 1.1920929e-07          /* FLT_EPSILON, OpenCV's criterion */
#define VIO_SFM_BA_MAX_ITER 50                      /* Ceres' defaults */
#define VIO_SFM_BA_FUNCTION_TOL 1e-6
#define VIO_SFM_BA_GRADIENT_TOL 1e-10
#define VIO_SFM_BA_PARAMETER_TOL 1e-8
#define VIO_SFM_LM_INITIAL_RADIUS 1e4

/* Per-window outcomes besides VIO_OK and VIO_ERR_NOT_FINITE, in the order the reference meets them. */
#define VIO_SFM_FAIL_RELATIVE_POSE 1    /* relativePose: no frame with enough correspondences, parallax and points in front */
#define VIO_SFM_FAIL_PNP 2              /* solveFrameByPnP of frame fail_frame: fewer than 10 points, or no finite pose */
#define VIO_SFM_FAIL_BA 3               /* the bundle adjustment neither converged nor ended below 5e-3 */

typedef struct vio_sfm vio_sfm;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_sfm_create(int32_t device, void *stream, vio_sfm **out);
void vio_sfm_destroy(vio_sfm *h);
const char *vio_sfm_last_error(const vio_sfm *h);          /* valid until the next call on h */
int32_t vio_sfm_version(void);

typedef struct vio_sfm_config {
    uint32_t seed;                  /* of the sampling hash; default 0 */
    int32_t ransac_hypotheses;      /* in [1, VIO_SFM_MAX_HYPOTHESES]; default VIO_SFM_DEFAULT_HYPOTHESES */
} vio_sfm_config;
vio_status vio_sfm_set_config(vio_sfm *h, const vio_sfm_config *cfg);

typedef struct vio_sfm_item {
    int32_t n_frames;               /* F in [3, VIO_SFM_MAX_FRAMES] */
    int32_t n_tracks;               /* sfm_f (estimator.cpp:275-289), in f_manager.feature's order */
    const int32_t *start_frame;     /* [n_tracks] */
    const int64_t *obs_offset;      /* [n_tracks + 1]: track j is seen in frames start_frame[j] .. with pts[obs_offset[j] ..] */
    const double *pts;              /* [obs_offset[n_tracks]][2] normalised image points */
} vio_sfm_item;

typedef struct vio_sfm_rel_result {
    int32_t status;                 /* VIO_OK, VIO_SFM_FAIL_RELATIVE_POSE, VIO_ERR_NOT_FINITE */
    int32_t l;                      /* the frame chosen, -1 if none */
    int32_t hyp;                    /* the winning hypothesis of frame l */
    int32_t n_corres;               /* correspondences of frame l: the length of its mask */
    int32_t n_inliers;              /* of the final mask */
    int32_t n_front;                /* recoverPose's count */
    double R[9];                    /* relative_R, row-major (NaN unless VIO_OK) */
    double T[3];                    /* relative_T, |T| = 1 */
    int32_t corres[VIO_SFM_MAX_FRAMES];     /* [i < F-1]: correspondences between frame i and frame F-1 */
    double parallax[VIO_SFM_MAX_FRAMES];    /* ... and their mean parallax * 460 */
} vio_sfm_rel_result;

typedef struct vio_sfm_result {
    int32_t status;                 /* VIO_OK, VIO_SFM_FAIL_*, VIO_ERR_NOT_FINITE */
    int32_t fail_frame;             /* the frame whose PnP failed, else -1 */
    int32_t ba_iterations;
    int32_t ba_converged;
    int32_t n_triangulated;
    int32_t pnp_iterations[VIO_SFM_MAX_FRAMES];
    double initial_cost, final_cost;            /* of the bundle adjustment */
    double Q[4 * VIO_SFM_MAX_FRAMES];           /* [F] (w, x, y, z): camera poses in frame l (NaN unless VIO_OK) */
    double T[3 * VIO_SFM_MAX_FRAMES];           /* [F] */
} vio_sfm_result;

/* mask: [sum of n_tracks] or NULL; window i's part starts at the sum of the n_tracks before it, and its first n_corres bytes are
 * the final RANSAC mask over frame l's correspondences (in track order). */
vio_status vio_sfm_relative_pose_batch(vio_sfm *h, int32_t count, const vio_sfm_item *items, vio_sfm_rel_result *rel, uint8_t *mask);

/* rel: [count] stage-1 results (status, l, R, T are read); a window whose rel status is not VIO_OK passes that status through.
 * points: [sum of n_tracks][3] or NULL, state: [sum of n_tracks] or NULL, laid out as mask: sfm_f[j].position (NaN where
 * state is 0 or the window did not succeed) and sfm_f[j].state. */
vio_status vio_sfm_construct_batch(vio_sfm *h, int32_t count, const vio_sfm_item *items, const vio_sfm_rel_result *rel,
                                   vio_sfm_result *res, double *points, uint8_t *state);

/* Both stages; rel_out: [count] or NULL, mask: as above or NULL. */
vio_status vio_sfm_batch(vio_sfm *h, int32_t count, const vio_sfm_item *items, vio_sfm_rel_result *rel_out, uint8_t *mask,
                         vio_sfm_result *res, double *points, uint8_t *state);

/* ms of the last call that launched: host packing + upload, k_sfm_relpose, k_sfm_construct (HIP events; NaN for a stage that did
 * not run), the whole call. */
vio_status vio_sfm_timing(const vio_sfm *h, double *out4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
