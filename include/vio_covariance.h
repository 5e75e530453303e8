/*
 * vio_covariance.h — marginal covariances of a solved window (companion library libvio_cov_hip.so).
 *
 * Not a reference entry point: the reference's Problem has no covariance query.  This library sits beside libvio_hip.so and calls
 * only its public C ABI (include/vio_backend.h); at build time it shares libvio_hip's device helpers (csrc/vio_device_math.h: the
 * loss functions, rotations, 3x3 products), so a change there changes both libraries.  It reads the states with vio_get_window / vio_get_landmarks(_xyz) and
 * H_pp_schur_ with vio_get_schur_system (calling vio_linearize first when the context holds no linearisation of its current
 * state), and enqueues its two kernels on the context's stream (vio_get_stream).  DESIGN.md section 10 has the math.
 *
 * Ordering of pose_cov: the one of vio_get_schur_system, [ext(6) | (pose 6, speed-bias 9) x 11], 171 x 171 row-major, both
 * triangles.  Variables held fixed come back as exact zero rows and columns:
 *   - the extrinsic when cfg.ext_fixed, and always in an XYZ window (EdgeReprojectionXYZ takes it as a constant);
 *   - frame 0's pose (6) under VIO_COV_GAUGE_FIX_OLDEST.
 * Landmarks:
 *   inverse depth  lm_var[l] = 1/h_l + w_l^T Sigma_cc w_l / h_l^2                       (n doubles)
 *   XYZ            lm_cov[l] = H_ll^-1 + H_ll^-1 W_l^T Sigma_cc W_l H_ll^-1            (n x 3 x 3 row-major)
 * with h_l / H_ll and w_l / W_l the landmark's information and its coupling to the 72 camera variables, recomputed from the
 * observations under the robust weighting of Edge::RobustInfo, and Sigma_cc the 72 x 72 camera block of pose_cov.
 *
 * Conditioning: VIO_OK says only that every pivot of the factorisation was positive and finite, not that the window determines its
 * states well.  A window with a direction it barely constrains (a null direction in exact arithmetic that rounding left slightly
 * positive) returns VIO_OK with covariances that mean nothing along it; vio_cov_pivot_ratio reports min_k d_k / S_kk, the smallest
 * pivot of S = L D L^T relative to its diagonal (1 for a diagonal S; of the order of 1 / kappa, or eps, when S is nearly singular).
 *
 * Errors: VIO_ERR_NOT_FINITE when a pivot of the pose factorisation, or a landmark's information, is not positive and finite
 * (vio_cov_last_error names the variable); nothing is written to the outputs then.  VIO_ERR_UNSUPPORTED for a sharded context.
 * One handle per context; the same threading rule as the context (one caller thread at a time).  The calling thread's current
 * HIP device is left as the caller had it.
 */
#ifndef VIO_COVARIANCE_H
#define VIO_COVARIANCE_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_COV_VERSION 2

typedef enum {
    VIO_COV_GAUGE_NONE = 0,         /* invert H_pp_schur as it is (a window without a prior has 4 unobservable directions) */
    VIO_COV_GAUGE_FIX_OLDEST = 1    /* frame 0's pose held fixed: covariances relative to it */
} vio_cov_gauge;

typedef struct vio_cov vio_cov;

/* cfg: the configuration the context currently runs with (vio_create / the last vio_set_config).  The handle keeps a copy (loss,
 * edge information, ext_fixed): after a vio_set_config on the context, call vio_cov_set_config with the same cfg before the next
 * compute, or the landmark weights and the fixed variables are those of the old configuration.  After a change that matters to the
 * system (loss, information, ext_fixed, gravity, item policy) the next compute re-linearises the context first: vio_set_config keeps
 * the linearisation the context held, which is of the old configuration. */
vio_status vio_cov_create(struct vio_ctx *ctx, const vio_config *cfg, vio_cov **out);
vio_status vio_cov_set_config(vio_cov *cv, const vio_config *cfg);
void vio_cov_destroy(vio_cov *cv);
const char *vio_cov_last_error(const vio_cov *cv);      /* valid until the next call on cv */
int32_t vio_cov_version(void);

/* Inverse-depth window.  m, lm, host, target, pts_i, pts_j: what vio_set_observations was given; n: the landmark count.
 * pose_cov: 171 x 171 or NULL; lm_var: n or NULL. */
vio_status vio_cov_compute(vio_cov *cv, int32_t gauge, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                           const double *pts_i, const double *pts_j, int64_t n, double *pose_cov, double *lm_var);
/* XYZ window.  m, lm, frame, pts: what vio_set_observations_xyz was given.  lm_cov: n x 3 x 3 or NULL. */
vio_status vio_cov_compute_xyz(vio_cov *cv, int32_t gauge, int64_t m, const int32_t *lm, const int32_t *frame, const double *pts,
                               int64_t n, double *pose_cov, double *lm_cov);

/* Many windows at once: what vio_cov_compute / vio_cov_compute_xyz give for each window, bitwise, with one
 * launch of each kernel for the whole batch and one synchronisation.  cvs[i]: one handle per window, no handle twice; their contexts
 * share one device and one stream (vio_config.stream) and all hold the kind of landmark `xyz` names (0: inverse depths, 1: XYZ).
 * items[i]: window i's arguments, those of the single call.  For an XYZ window `target` is the observing frame and `pts_j` the
 * observation (what vio_set_observations_xyz took as frame / pts); host and pts_i are ignored.
 * Errors of the batch, with nothing written and no kernel launched: VIO_ERR_BAD_ARG for a mismatch of device, stream or landmark kind,
 * a handle given twice, or a window whose arguments the single call refuses; VIO_ERR_UNSUPPORTED for a sharded context.  The message
 * is on cvs[0] (vio_cov_last_error) and names the window.  count = 0 is a no-op that returns VIO_OK.
 * Per window: window_status[i] (may be NULL) is VIO_OK or VIO_ERR_NOT_FINITE.  A window that fails has its outputs left untouched and
 * its handle's vio_cov_last_error naming the variable; the others are still computed and written, and the call then returns
 * VIO_ERR_NOT_FINITE.  Afterwards vio_cov_landmark_information / vio_cov_pivot_ratio of each successful window's handle are those of
 * its window, and vio_cov_timing of every handle of the batch gives the batch's times (host = every window's linearise + read-back +
 * upload, then the kernels over all windows, then the whole call).  No context's state changes. */
typedef struct vio_cov_batch_item {
    int64_t m;
    const int32_t *lm, *host, *target;
    const double *pts_i, *pts_j;
    int64_t n;
    double *pose_cov;               /* 171 x 171 or NULL */
    double *lm_out;                 /* lm_var (n) / lm_cov (n x 3 x 3) or NULL */
} vio_cov_batch_item;
vio_status vio_cov_compute_batch(vio_cov *const *cvs, int32_t count, int32_t gauge, int32_t xyz, const vio_cov_batch_item *items,
                                 vio_status *window_status);

/* h_l (n doubles) or H_ll (n x 3 x 3) as the last successful compute recomputed them. */
vio_status vio_cov_landmark_information(vio_cov *cv, int64_t n, double *info);
/* min_k d_k / S_kk of the last successful compute (see "Conditioning" above). */
vio_status vio_cov_pivot_ratio(vio_cov *cv, double *ratio);
/* Times of the last successful compute, ms: [0] linearise (when needed) + read-back of the system and states + upload, host wall
 * clock; [1] k_cov_pose, [2] k_cov_landmarks (HIP events on the context's stream); [3] the whole call, wall clock.  NaN when the
 * events could not be read. */
vio_status vio_cov_timing(vio_cov *cv, double *out4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
