/*
 * vio_residuals.h — per-edge residuals, the chi2 breakdown and landmark outlier flags of a window (companion library
 * libvio_res_hip.so).
 *
 * Not a reference entry point.  The reference keeps the hook for it and never uses it: FeatureManager::removeOutlier
 * (VM/src/feature_manager.cpp:259-275) erases the features marked is_outlier (VM/include/feature_manager.h:53), but its body starts
 * with `return;` and nothing sets the flag; removeFailures (:161-171) drops the features whose solve_flag is 2 (a negative depth,
 * setDepth :150-157).  This library answers "which measurements disagree with the estimate" after a solve, so that a caller can set
 * those flags.  It sits beside libvio_hip.so and calls only its public C ABI (include/vio_backend.h): the states through
 * vio_get_window / vio_get_landmarks(_xyz), err_prior through vio_get_prior, the stream through vio_get_stream.  Its kernels share
 * libvio_hip's device helpers (csrc/vio_device_math.h) and the IMU residual the solver evaluates (csrc/vio_imu_math.h).  DESIGN.md
 * section 11 has the kernels and the rules.
 *
 * Inputs: the observation arrays given to vio_set_observations / vio_set_observations_xyz, in the same order, and `pre`, the ten
 * pointers vio_set_imu_all took (a NULL entry: no edge).  With pre == NULL the IMU fields of the summary, and its chi2, are NaN.
 * Outputs (every one may be NULL; a NULL output is neither computed into host memory nor copied back):
 *   obs_out   m x 4, one row per edge in the caller's order: r_x, r_y (the 2-D residual, normalised-plane units),
 *             e2 = s^2 |r|^2 (Edge::Chi2, edge.cc:33-37) and rho0 (RobustChi2: the configured loss of e2; e2 itself without a loss)
 *   lm_out    n x 3, one row per landmark: mean and maximum of the pixel error focal * |r| over its edges, and the sum of their rho0;
 *             zeros for a landmark without an edge
 *   lm_flags  n bytes: VIO_RES_FLAG_* below
 *   summary   vio_res_summary below
 * Errors: VIO_ERR_BAD_ARG, with nothing written, for an index out of range, an n other than the context's landmark count, m < 0 or
 * focal <= 0.  (The public ABI has no getter of the context's edge count: m is the caller's to keep consistent with its last
 * vio_set_observations; the Python binding checks it.)  Non-finite states are not an error: NaN goes through to the outputs, as it
 * does through vio_chi2.  VIO_ERR_UNSUPPORTED for a sharded context (at create).
 * One handle per context; the same threading rule as the context.  Every call enqueues three kernels on the context's stream and
 * synchronises once, at the end; repeated calls on the same state give bitwise the same outputs (every sum has a fixed order).
 * The calling thread's current HIP device is left as the caller had it.
 */
#ifndef VIO_RESIDUALS_H
#define VIO_RESIDUALS_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_RES_VERSION 2

/* bits of lm_flags */
#define VIO_RES_FLAG_REPROJ 1u     /* the mean pixel error is above outlier_px (a NaN mean counts as above): FeaturePerId::is_outlier */
#define VIO_RES_FLAG_DEPTH 2u      /* some edge has its point at depth <= 0 in the observing camera */
#define VIO_RES_FLAG_STATE 4u      /* inverse depth <= 0 or not finite (solve_flag = 2, feature_manager.cpp:150-157); XYZ: a coordinate
                                      that is not finite */

typedef struct vio_res_summary {
    double chi2;                  /* 0.5 * (visual_robust + imu + prior): vio_chi2's value (problem.cc:549-556) */
    double visual_robust;         /* sum of rho0 over the reprojection edges */
    double visual_plain;          /* sum of e2 */
    double imu;                   /* sum of imu_edge */
    double prior;                 /* ||err_prior||, not squared, as problem.cc:549-556 adds it; 0 without a prior */
    double imu_edge[VIO_WINDOW_SIZE];     /* r^T Sigma^-1 r of the IMU edge k -> k + 1; 0 for a missing edge */
    double frame_robust[VIO_NUM_FRAMES];  /* sum of rho0 over the edges observed in frame f (target frame; XYZ: frame) */
    int64_t frame_edges[VIO_NUM_FRAMES];  /* their count */
    int64_t n_flagged[3];         /* landmarks with bit k of lm_flags set */
} vio_res_summary;

typedef struct vio_res vio_res;

/* cfg: the configuration the context currently runs with (loss, reproj_sqrt_info, gravity are read from the handle's copy).  After a
 * vio_set_config on the context, call vio_res_set_config with the same cfg before the next compute. */
vio_status vio_res_create(struct vio_ctx *ctx, const vio_config *cfg, vio_res **out);
vio_status vio_res_set_config(vio_res *rs, const vio_config *cfg);
void vio_res_destroy(vio_res *rs);
const char *vio_res_last_error(const vio_res *rs);      /* valid until the next call on rs */
int32_t vio_res_version(void);

/* Inverse-depth window.  m, lm, host, target, pts_i, pts_j: what vio_set_observations was given; n: the landmark count; focal: pixels
 * per normalised-plane unit (the pixel error is focal * |r|); outlier_px: the threshold of VIO_RES_FLAG_REPROJ. */
vio_status vio_res_compute(vio_res *rs, int64_t m, const int32_t *lm, const int32_t *host, const int32_t *target,
                           const double *pts_i, const double *pts_j, int64_t n, const vio_preint *const *pre, double focal,
                           double outlier_px, double *obs_out, double *lm_out, uint8_t *lm_flags, vio_res_summary *summary);
/* XYZ window.  m, lm, frame, pts: what vio_set_observations_xyz was given. */
vio_status vio_res_compute_xyz(vio_res *rs, int64_t m, const int32_t *lm, const int32_t *frame, const double *pts, int64_t n,
                               const vio_preint *const *pre, double focal, double outlier_px, double *obs_out, double *lm_out,
                               uint8_t *lm_flags, vio_res_summary *summary);

/* Many windows at once: what vio_res_compute / vio_res_compute_xyz give for each window, bitwise, with one
 * launch of each kernel for the whole batch (every window's edges and landmarks tiled from a workgroup boundary, one k_res_tail
 * workgroup per window) and one synchronisation.  rss[i]: one handle per window, no handle twice; their contexts share one device and
 * one stream (vio_config.stream) and all hold the kind of landmark `xyz` names (0: inverse depths, 1: XYZ).  items[i]: window i's
 * arguments and outputs, those of the single call (each output may be NULL); focal and outlier_px are the batch's.  For an XYZ window
 * `target` is the observing frame and `pts_j` the observation (vio_set_observations_xyz's frame / pts); host and pts_i are ignored.
 * Errors, with nothing written and no kernel launched: VIO_ERR_BAD_ARG for a mismatch of device, stream or landmark kind, a handle
 * given twice, or a window whose arguments the single call refuses; VIO_ERR_UNSUPPORTED for a sharded context.  The message is on
 * rss[0] (vio_res_last_error) and names the window.  count = 0 is a no-op that returns VIO_OK.  Afterwards vio_res_timing of every
 * handle of the batch gives the batch's times (host = every window's read-back + packing + upload). */
typedef struct vio_res_batch_item {
    int64_t m;
    const int32_t *lm, *host, *target;
    const double *pts_i, *pts_j;
    int64_t n;
    const vio_preint *const *pre;   /* the ten pointers of vio_set_imu_all, or NULL (IMU fields and chi2 NaN) */
    double *obs_out;                /* m x 4 or NULL */
    double *lm_out;                 /* n x 3 or NULL */
    uint8_t *lm_flags;              /* n or NULL */
    vio_res_summary *summary;       /* or NULL */
} vio_res_batch_item;
vio_status vio_res_compute_batch(vio_res *const *rss, int32_t count, int32_t xyz, const vio_res_batch_item *items, double focal,
                                 double outlier_px);

/* Times of the last successful compute, ms: [0] read-back of the states + packing + upload, host wall clock; [1] k_res_obs,
 * [2] k_res_lm, [3] k_res_tail (HIP events on the context's stream); [4] the whole call, wall clock.  NaN when the events could not
 * be read. */
vio_status vio_res_timing(vio_res *rs, double *out5);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
