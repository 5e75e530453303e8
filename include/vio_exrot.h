/*
 * vio_exrot.h — batched camera-IMU extrinsic rotation calibration on the GPU (companion library libvio_exrot_hip.so).
 *
 * InitialEXRotation::CalibrationExRotation (VM/src/initial/initial_ex_rotation.cpp:11-141, driven from estimator.cpp:161-178, the
 * ESTIMATE_EXTRINSIC == 2 case) for `count` independent windows in one call.  The reference is called once per new frame and keeps a
 * growing history of rotation pairs; here a window of F frames is that history after F - 1 calls, and every call's outcome ("step"
 * k = 1 .. F - 1, the reference's frame_count) is reported:
 *   vio_exrot_relative_rotations_batch   solveRelativeR of every consecutive frame pair of every window            (k_exrot_pairs)
 *   vio_exrot_calibrate_batch            the recursion over the pairs from given Rc and delta_q: Rc_g with the ric of the step
 *                                        before, the Huber weights, the 4 x 4 problem, the gate                     (k_exrot_solve)
 *   vio_exrot_batch                      both, without a host round trip in between
 * It works from host arrays and needs nothing from libvio_hip but the vio_status type.  DESIGN.md section 17 has the math, the layout
 * and the measurements.
 *
 * The reference does step 1 with OpenCV.  What replaces it, so that the work is fixed and repeatable (this reading is not compared
 * against OpenCV, which is not a dependency; tests/exrot_reference.py restates it in numpy and the device is held to that):
 *   - cv::findFundamentalMat(ll, rr) with its defaults (FM_RANSAC, threshold 3.0, confidence 0.99): the points are normalised image
 *     coordinates, so a threshold of 3.0 makes every correspondence an inlier of every hypothesis, and OpenCV's final step is the
 *     normalised 8-point fit over all correspondences.  That fit is computed directly, over all correspondences in track order: no
 *     sampling, no seed, no hypothesis count.  It is the model of include/vio_sfm.h (Hartley scaling of each point set to mean
 *     distance sqrt 2, the smallest eigenvector of the 9 x 9 normal matrix, rank 2 enforced by removing the smallest singular
 *     direction).  Every sum over the correspondences (the centroids, the mean distances, the 45 entries of the normal matrix) runs
 *     in track order, one accumulator per sum.  The reference's conversion of the points to float (cv::Point2f) is not imitated.
 *   - decomposeE (cv::SVD): V and the singular values from the eigenvectors of E^T E in descending order, u0 = E v0 / s0,
 *     u1 = E v1 / s1 made orthonormal to u0, u2 = u0 x u1 (as cv::recoverPose is restated in vio_sfm.h, but with no sign fix of V:
 *     det V may be -1).  R1 = U W V^T, R2 = U W^T V^T, t = +-u2.  Where det R1 + 1 < 1e-9 the reference negates E and decomposes
 *     again; the SVD of -E is (-U, S, V), so R1 and R2 are negated and t1, t2 swap (det_flip reports it).
 *   - testTriangulation (cv::triangulatePoints): the two-view triangulation of vio_sfm.h for P = [I | 0], P1 = [R | t], in double;
 *     a point counts when its depth is positive in both views.  The four counts are reported in the order (R1, t1), (R1, t2),
 *     (R2, t1), (R2, t2) with t1 = u2, t2 = -u2.  All four ratios share the denominator n, so they are compared as integers:
 *     R1 is taken iff max(front[0], front[1]) > max(front[2], front[3]), else R2; the result is transposed.
 *   - fewer than 9 correspondences: the identity.
 * Steps 2-5 are the reference's own arithmetic:
 *   - Rc_g[k] = ric^T R(delta_q[k]) ric with the ric of step k - 1 (the identity before step 1), kept as stored;
 *   - pair k's Huber weight is huber_deg / angle where the angular distance between Quaternion(Rc[k]) and Quaternion(Rc_g[k])
 *     (2 atan2(|vec|, |w|) of q1 q2^-1, in degrees) exceeds huber_deg, else 1.  It is set when the pair arrives and never changes,
 *     so one weight per step is reported;
 *   - A stacks huber (L(q_c) - R(q_imu)) of pairs 1 .. k; x = the right singular vector of its smallest singular value, from the
 *     eigenvectors of A^T A (4 x 4, summed in pair order); ric = Quaternion(x).toRotationMatrix()^T;
 *   - the gate: k >= min_frames and the second-smallest singular value > min_sigma.
 *   - every symmetric eigenproblem (9 x 9, 4 x 4, 3 x 3) is a cyclic Jacobi iteration of VIO_SFM_JACOBI_SWEEPS sweeps.
 *
 * Rules (those of include/vio_sfm.h):
 *   - argument errors (count < 0, a NULL array, n_frames outside [2, VIO_EXROT_MAX_FRAMES], n_tracks outside
 *     [0, VIO_EXROT_MAX_TRACKS], a track that leaves the window) write nothing and launch nothing: VIO_ERR_BAD_ARG,
 *     vio_exrot_last_error names the window.  count == 0 does nothing and returns VIO_OK;
 *   - a window whose inputs or results are not finite gets VIO_ERR_NOT_FINITE (its outputs NaN); the others are computed as if it
 *     were not there, and the call returns VIO_ERR_NOT_FINITE.  A window that never passes the gate gets
 *     VIO_EXROT_FAIL_NOT_OBSERVABLE; that is an outcome, not an error (the call returns VIO_OK);
 *   - repeated calls are bitwise identical, and a window's result does not depend on the batch it is in (no floating-point atomics,
 *     fixed summation orders);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_EXROT_H
#define VIO_EXROT_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_EXROT_VERSION 1
/* F: the reference's history grows past the window (frame_count only ever increases), so the cap is above WINDOW_SIZE + 1.
 * k_exrot_solve prepares the pairs one per lane of its single wavefront (at most 63 pairs) and keeps 23 doubles per pair in LDS:
 * 5.7 KB at F = 32, so LDS never bounds how many windows share a CU (160 KB), and nothing is kept in per-lane scratch arrays
 * indexed by the pair.  32 is three windows' worth of pairs; the per-pair and per-step results are flat arrays sized by the call,
 * so the cap is not part of a struct's layout. */
#define VIO_EXROT_MAX_FRAMES 32
#define VIO_EXROT_MAX_TRACKS 4096                   /* per window, as VIO_SFM_MAX_TRACKS */
#define VIO_EXROT_MIN_CORRES 9                      /* solveRelativeR: fewer give the identity */

#define VIO_EXROT_DEFAULT_MIN_FRAMES 10             /* WINDOW_SIZE */
#define VIO_EXROT_DEFAULT_MIN_SIGMA 0.25
#define VIO_EXROT_DEFAULT_HUBER_DEG 5.0

/* Per-window outcome besides VIO_OK and VIO_ERR_NOT_FINITE. */
#define VIO_EXROT_FAIL_NOT_OBSERVABLE 1     /* no step passed the gate */

typedef struct vio_exrot vio_exrot;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_exrot_create(int32_t device, void *stream, vio_exrot **out);
void vio_exrot_destroy(vio_exrot *h);
const char *vio_exrot_last_error(const vio_exrot *h);      /* valid until the next call on h */
int32_t vio_exrot_version(void);

typedef struct vio_exrot_config {
    int32_t min_frames;             /* the gate's frame_count, >= 1; default VIO_EXROT_DEFAULT_MIN_FRAMES */
    int32_t reserved;
    double min_sigma;               /* the gate's second-smallest singular value (exceeded), finite, >= 0; default 0.25 */
    double huber_deg;               /* > 0; default 5 */
} vio_exrot_config;
vio_status vio_exrot_set_config(vio_exrot *h, const vio_exrot_config *cfg);

/* The CSR track form of vio_sfm_item plus the pre-integrated rotations. */
typedef struct vio_exrot_item {
    int32_t n_frames;               /* F in [2, VIO_EXROT_MAX_FRAMES] */
    int32_t n_tracks;               /* in f_manager.feature's order */
    const int32_t *start_frame;     /* [n_tracks] */
    const int64_t *obs_offset;      /* [n_tracks + 1]: track j is seen in frames start_frame[j] .. with pts[obs_offset[j] ..] */
    const double *pts;              /* [obs_offset[n_tracks]][2] normalised image points */
    const double *delta_q;          /* [F - 1][4] (w, x, y, z): the pre-integrated rotation from frame k to frame k + 1.
                                       vio_exrot_relative_rotations_batch does not read it (NULL allowed);
                                       vio_exrot_calibrate_batch reads only n_frames and delta_q */
} vio_exrot_item;

/* One consecutive frame pair (k, k + 1) of a window. */
typedef struct vio_exrot_pair {
    int32_t status;                 /* VIO_OK or VIO_ERR_NOT_FINITE */
    int32_t n_corres;               /* getCorresponding(k, k + 1) */
    int32_t front[4];               /* points in front of both cameras for (R1, t1), (R1, t2), (R2, t1), (R2, t2); the ratios are
                                       front / n_corres.  0 with fewer than VIO_EXROT_MIN_CORRES correspondences */
    int32_t choice;                 /* 1: R1, 2: R2, 0: the identity (too few correspondences) */
    int32_t det_flip;               /* 1: det R1 was -1 and E was negated */
    double Rc[9];                   /* row-major, the chosen rotation transposed (NaN unless VIO_OK) */
} vio_exrot_pair;

/* One step k = 1 .. F - 1 of a window: the state after pair k arrived. */
typedef struct vio_exrot_step {
    double q[4];                    /* ric (w, x, y, z), Eigen's Quaternion(Matrix3d) of R */
    double R[9];                    /* ric, row-major */
    double sigma[3];                /* the three smallest singular values of A, descending: sigma[1] is the gate's */
    double huber;                   /* the weight of pair k */
} vio_exrot_step;

typedef struct vio_exrot_result {
    int32_t status;                 /* VIO_OK, VIO_EXROT_FAIL_NOT_OBSERVABLE, VIO_ERR_NOT_FINITE */
    int32_t step;                   /* the first step that passed the gate (1-based, the reference's frame_count), else -1 */
    double q[4];                    /* ric at that step (NaN unless VIO_OK) */
    double R[9];
} vio_exrot_result;

/* pairs, steps: [sum of (n_frames - 1)]; window i's part starts at the sum of the (n_frames - 1) before it. */
vio_status vio_exrot_relative_rotations_batch(vio_exrot *h, int32_t count, const vio_exrot_item *items, vio_exrot_pair *pairs);

/* Rc: [sum of (n_frames - 1)][9] row-major, laid out as pairs.  steps: as above or NULL.  The steps after the first one that
 * passes the gate are still computed and reported (the reference goes on calibrating until the caller stops calling it). */
vio_status vio_exrot_calibrate_batch(vio_exrot *h, int32_t count, const vio_exrot_item *items, const double *Rc, vio_exrot_result *res,
                                     vio_exrot_step *steps);

/* Both stages; pairs and steps: as above or NULL. */
vio_status vio_exrot_batch(vio_exrot *h, int32_t count, const vio_exrot_item *items, vio_exrot_pair *pairs, vio_exrot_result *res,
                           vio_exrot_step *steps);

/* ms of the last call that launched: host packing + upload, k_exrot_pairs, k_exrot_solve (HIP events; NaN for a stage that did
 * not run), the whole call. */
vio_status vio_exrot_timing(const vio_exrot *h, double *out4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
