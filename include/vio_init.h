/*
 * vio_init.h — batched visual-inertial alignment on the GPU (companion library libvio_init_hip.so).
 *
 * The alignment half of the reference's initialisation, Estimator::visualInitialAlign (VM/src/estimator.cpp:384-460) with
 * VisualIMUAlignment (VM/src/initial/initial_aligment.cpp), for `count` independent windows in one call:
 *   vio_init_gyro_bias_batch   solveGyroscopeBias (:3-37) without its repropagate                       (k_init_gyro)
 *   vio_init_align_batch       LinearAlignment + RefineGravity (:39-200) on re-propagated records, then visualInitialAlign's state
 *                              change (estimator.cpp:397-458): scale, gravity, velocities and the gravity-aligned, yaw-zeroed
 *                              keyframe states                                                          (k_init_align)
 * Between the two calls the caller re-propagates every interval at (ba = 0, bg_out), exactly as solveGyroscopeBias calls
 * repropagate(Vector3d::Zero(), Bgs[0]): vio_imu_propagate (include/vio_imu.h) does that for any number of intervals in one launch,
 * vio_preintegrate (include/vio_backend.h) one interval at a time.  The SfM that produces R / T (relativePose, GlobalSFM, solvePnP)
 * is not part of this library.  It works from host arrays and needs nothing from libvio_hip but the vio_preint / vio_status types.
 * DESIGN.md section 15 has the math, the layout and the measurements.
 *
 * Semantics are the reference's, line by line, its quirks included: A and b are multiplied by 1000 before every solve; the scale is
 * x(n-1) / 100; RefineGravity's A and b are zeroed once, before its four iterations, so every iteration adds to the previous,
 * already scaled, system; TangentBasis compares a == (0,0,1) exactly; g2R goes through Quaternion::FromTwoVectors with Eigen 3.3's
 * near-antiparallel branch; keyframe kv's velocity is read from x.segment<3>(kv * 3), an index over all frames; the accelerometer
 * biases stay zero.  Every ldlt().solve is Eigen's LDLT with diagonal pivoting, in the operation order of that routine.
 *
 * Rules:
 *   - argument errors (count < 0, a NULL array, n_frames outside [2, VIO_INIT_MAX_FRAMES], fewer than two keyframes) write nothing
 *     and launch nothing: VIO_ERR_BAD_ARG, vio_init_last_error names the window.  count == 0 does nothing and returns VIO_OK;
 *   - a window whose inputs or results are not finite gets VIO_ERR_NOT_FINITE (its outputs NaN); the others are computed as if it
 *     were not there, and the call returns VIO_ERR_NOT_FINITE.  A window that fails one of the reference's tests gets one of the
 *     VIO_INIT_FAIL_* codes below; that is an outcome, not an error (the call returns VIO_OK);
 *   - repeated calls are bitwise identical, and a window's result does not depend on the batch it is in (no atomics, fixed
 *     summation orders);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_INIT_H
#define VIO_INIT_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_INIT_VERSION 1
#define VIO_INIT_MAX_FRAMES 32                              /* F; the dense systems are at most 3F + 4 = 100 wide */
#define VIO_INIT_X_STRIDE (3 * VIO_INIT_MAX_FRAMES + 3)     /* doubles per window in vio_init_align_batch's x */
#define VIO_INIT_POSE_STRIDE (7 * VIO_INIT_MAX_FRAMES)      /* ... in its poses */
#define VIO_INIT_SB_STRIDE (9 * VIO_INIT_MAX_FRAMES)        /* ... in its speed_bias */

/* Per-window outcomes of vio_init_align_batch besides VIO_OK and VIO_ERR_NOT_FINITE: the three `return false` of LinearAlignment
 * (initial_aligment.cpp:178-200), in the order the reference tests them. */
#define VIO_INIT_FAIL_GRAVITY 1     /* linear stage: | |g| - G | > 1 */
#define VIO_INIT_FAIL_SCALE 2       /* linear stage: s < 0 (with |g| within 1 of G) */
#define VIO_INIT_FAIL_REFINED_SCALE 3   /* after RefineGravity: s < 0 */

typedef struct vio_init vio_init;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_init_create(int32_t device, void *stream, vio_init **out);
void vio_init_destroy(vio_init *h);
const char *vio_init_last_error(const vio_init *h);        /* valid until the next call on h */
int32_t vio_init_version(void);

typedef struct vio_init_item {
    int32_t n_frames;               /* F in [2, VIO_INIT_MAX_FRAMES]: all_image_frame in time order */
    const uint8_t *is_key;          /* [F], or NULL = every frame is a keyframe (Headers[]); at least two keyframes */
    const double *R;                /* [F][9] row-major: ImageFrame::R = Q_sfm * RIC^T */
    const double *T;                /* [F][3]: ImageFrame::T, up to scale */
    const vio_preint *pre;          /* [F-1]: pre[k] = interval k -> k+1 (frame k+1's pre_integration) */
} vio_init_item;

typedef struct vio_init_result {
    int32_t status;                 /* VIO_OK, VIO_INIT_FAIL_*, VIO_ERR_NOT_FINITE */
    int32_t n_key;                  /* K: keyframes, the rows of poses / speed_bias */
    double s;                       /* refined scale, x(n-1) / 100 after RefineGravity (NaN if the linear stage failed) */
    double g[3];                    /* refined gravity in the SfM frame (NaN if the linear stage failed) */
    double g_world[3];              /* R0 g (NaN unless status == VIO_OK) */
    double s_linear;                /* LinearAlignment's scale */
    double g_linear[3];             /* LinearAlignment's gravity, x.segment<3>(n-4) */
    double rot[9];                  /* R0 = rot_diff, row-major: SfM frame -> gravity-aligned, yaw-zeroed world (NaN unless VIO_OK) */
} vio_init_result;

/* solveGyroscopeBias (initial_aligment.cpp:3-37) without its repropagate: bg_out[i] = bg_in[i] + delta_bg of window i.
 * status: [count] per-window VIO_OK / VIO_ERR_NOT_FINITE, or NULL. */
vio_status vio_init_gyro_bias_batch(vio_init *h, int32_t count, const vio_init_item *items, const double *bg_in /*[count][3]*/,
                                    double *bg_out /*[count][3]*/, int32_t *status);

/* LinearAlignment + RefineGravity (:39-200) on re-propagated records, then visualInitialAlign's state change (estimator.cpp:397-458).
 * tic: [3] TIC[0]; g_norm: G.norm(); bg: [count][3] the gyro biases the records were propagated at (Bgs[]).
 * res: [count].  x: [count][VIO_INIT_X_STRIDE] or NULL: RefineGravity's x (3F + 3 values, the last one replaced by s), the rest of
 * the row not written.  poses: [count][VIO_INIT_POSE_STRIDE] or NULL: the K keyframes' (p, q xyzw) ready for vio_set_window;
 * speed_bias: [count][VIO_INIT_SB_STRIDE] or NULL: their (V, ba = 0, bg).  Rows of a window that did not succeed are NaN. */
vio_status vio_init_align_batch(vio_init *h, int32_t count, const vio_init_item *items, const double *tic, double g_norm,
                                const double *bg, vio_init_result *res, double *x, double *poses, double *speed_bias);

/* ms of the last call that launched: host packing + upload (wall clock + HIP events), the kernel (HIP events), the whole call. */
vio_status vio_init_timing(const vio_init *h, double *out3);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
