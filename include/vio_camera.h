/*
 * vio_camera.h — the reference's four camera models for the front end, batched on the GPU (companion library libvio_camera_hip.so).
 *
 * include/vio_reject.h is rejectWithF and undistortedPoints through the PINHOLE camera alone.  This library is the same two stages,
 * and the bare lift, through any camera CameraFactory builds (VM/src/camera_models/camera_models/CameraFactory.cc): PINHOLE,
 * KANNALA_BRANDT (the FISHEYE rigs), MEI and SCARAMUZZA, for `count` independent streams in one call, each naming its own camera:
 *   vio_camera_lift_batch        liftProjective of a point set: the rays, in double                         (k_reject_lift)
 *   vio_camera_undistort_batch   undistortedPoints (feature_tracker.cpp:258-306)                            (k_reject_lift)
 *   vio_camera_reject_batch      rejectWithF (feature_tracker.cpp:169-202)                                  (k_reject_ransac)
 * The kernels are the text of csrc/vio_reject_body.inc compiled against csrc/vio_camera_math.h: one RANSAC in the project, with
 * include/vio_reject.h's settings (vio_reject_config), results (vio_reject_result), sampling and deviations.  The library works from
 * host arrays and needs nothing of libvio_hip but the vio_status type.  DESIGN.md section 27 has the layout and the measurements;
 * tests/camera_reference.py restates the arithmetic in numpy.
 *
 * Camera slots.  A handle holds VIO_CAMERA_MAX_SLOTS cameras on the device; vio_camera_set fills one, every item names one.  An item
 * whose slot was never set is an argument error.  params[] of vio_camera_model, in the order the model's readFromYamlFile reads them
 * (and writeParameters writes them), unused entries 0:
 *   PINHOLE          k1 k2 p1 p2 fx fy cx cy                          (PinholeCamera.cc:170-180)      fx, fy not 0
 *   MEI              xi k1 k2 p1 p2 gamma1 gamma2 u0 v0               (CataCamera.cc:186-199)         gamma1, gamma2 not 0
 *   SCARAMUZZA       p0 p1 p2 p3 p4 ac ad ae cx cy                    (ScaramuzzaCamera.cc:89-103; the 20 inv_poly entries are
 *                                                                      spaceToPlane's: vio_camera_set_inv_poly)  ac - ad ae not 0
 *   KANNALA_BRANDT   k2 k3 k4 k5 mu mv u0 v0 theta_max                (EquidistantCamera.cc:171-179)  mu, mv not 0
 * theta_max is this library's (see the root solve): in (0, pi], 0 for the default VIO_CAMERA_KB_DEFAULT_THETA_MAX = pi.
 *
 * Lift.  liftProjective of each model in the reference's operation order, in double, every product and sum rounded on its own:
 *   PINHOLE      include/vio_reject.h's lift (the same function): the ray (x, y, 1).
 *   MEI          CataCamera.cc:556-626: m_inv_K* from gamma1, gamma2, u0, v0 (:320-323), the recursive distortion model with n = 8
 *                evaluations of the distortion (:766-781, PinholeCamera's formula), then with rho2 = mx mx + my my the ray
 *                (mx, my, 1 - xi (rho2 + 1) / (xi + sqrt(1 + (1 - xi xi) rho2))), and (mx, my, (1 - mx mx - my my) / 2) when xi == 1.0.
 *   SCARAMUZZA   ScaramuzzaCamera.cc:599-621: xc = p - (cx, cy); xc_a = inv_scale (xc0 - ad xc1, -ae xc0 + ac xc1) with
 *                inv_scale = 1 / (ac - ad ae) (:200); phi = |xc_a|; z = sum phi^i p_i accumulated as written (z += phi_i p_i;
 *                phi_i *= phi).  The ray is (xc0, xc1, -z): the reference uses xc there, not the affine-corrected xc_a, and so does
 *                this library.
 *   KANNALA_BRANDT   EquidistantCamera.cc:428-442 over backprojectSymmetric (:716-818): p_u = (u / mu - u0 / mu, v / mv - v0 / mv) as
 *                m_inv_K* has it, rho = |p_u|, phi = atan2(p_u1, p_u0) (0 when rho < 1e-10), npow = 9 less 2 for every zero
 *                coefficient (:731-747); npow == 1: theta = rho; otherwise theta is the root of the next paragraph.  The ray is
 *                (sin theta cos phi, sin theta sin phi, cos theta).
 *
 * The KANNALA_BRANDT root.  The reference takes the eigenvalues of the companion matrix of
 *       f(theta) = theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9 - rho
 * and returns the smallest real one above -1e-10 (rho if there is none).  Here the work per point is fixed and the domain is stated:
 * vio_camera_set refuses a polynomial whose derivative is not positive at the VIO_CAMERA_KB_GRID + 1 grid points of [0, theta_max],
 * so the smallest non-negative root is the only root in [0, theta_max] whenever rho <= r(theta_max) = r_max.  It is bracketed from
 * f(0) = -rho <= 0 by VIO_CAMERA_KB_BISECTIONS halvings, then VIO_CAMERA_KB_NEWTON Newton steps kept inside the shrinking bracket;
 * f is evaluated by the compensated Horner scheme (fma for the products' errors), f' by Horner in theta^2.  No trip count depends on
 * the point.  Deviation: a point with rho > r_max gets theta = theta_max and is counted in n_clamped (lift and undistort); the
 * reference would return a larger root there, or rho.
 *   sin, cos and atan2 are not a math library's: two libraries do not round alike, and a ray that depended on the one linked would
 * not be the same on the device, in the host build and in the restatement.  csrc/vio_camera_math.h computes them in + - * / and
 * floor (fdlibm's published kernels and coefficients, with its two-step reduction by pi/2), so all three agree in every bit; sin and
 * cos are within one ulp, atan2 within two.  The tests' absolute bound on a ray component, C 2^-53, is the figure measured against
 * 50-digit arithmetic at the tests' inputs (1.79), doubled and rounded up: VIO_CAMERA_KB_RAY_C.
 *
 * vio_camera_undistort_batch.  vio_reject_undistort_batch with un_pts[i] = ((float)(P0 / P2), (float)(P1 / P2)): the same item layout
 * with a slot, the same velocity by id against the previous frame (the difference exact, in double), the same kept quirk of id -1.
 *
 * vio_camera_reject_batch.  vio_reject_batch with the virtual pixels (double)(float)(focal_length P0 / P2 + width / 2.0) and
 * (double)(float)(focal_length P1 / P2 + height / 2.0) of the pair's camera: the n < 8 gate, the hypotheses drawn by
 * hash(seed, pair, h, k), VIO_REJECT_FAIL_NO_MODEL and every deviation listed in include/vio_reject.h.
 *
 * A lift the tracker cannot use.  If P0 / P2 or P1 / P2 of any point of an item is not finite (P2 == 0 on a fisheye, or a pixel that
 * is not finite), the item gets VIO_ERR_NOT_FINITE: its mask is all zeros (hyp -1, F NaN), its un_pts and velocity are NaN; the other
 * items are computed, and the call returns VIO_ERR_NOT_FINITE.  vio_camera_lift_batch returns rays, where P2 == 0 is a value like any
 * other: only a pixel that is not finite gives VIO_ERR_NOT_FINITE there (the rays hold what the arithmetic gives).
 *
 * Rules (those of include/vio_reject.h): argument errors (count outside [0, VIO_CAMERA_MAX_ITEMS], a NULL array, n or m outside
 * [0, VIO_CAMERA_MAX_POINTS], a slot outside [0, VIO_CAMERA_MAX_SLOTS) or never set, dt not finite or <= 0 with m > 0) write nothing
 * and launch nothing; count == 0 returns VIO_OK; one launch and one wait per call; repeated calls are bitwise identical and an item's
 * result depends neither on its batch nor on its slot's number; the calling thread's current HIP device is restored; one handle is
 * used by one caller thread at a time.
 *
 * spaceToPlane of the four models, with SCARAMUZZA's inv_poly, is include/vio_camera_project.h's, in this library and on these slots
 * (vio_camera_project_batch, vio_camera_set_inv_poly).  Not built: the fisheye circle mask, which is the mask
 * image the tracker already takes.  The resident read_batch path of include/vio_frame_read.h takes these cameras per slot through include/vio_frame_camera.h
 * (vio_frame_set_slot_camera; its handle-wide vio_frame_set_camera stays PINHOLE).
 */
#ifndef VIO_CAMERA_H
#define VIO_CAMERA_H

#include "vio_reject.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_CAMERA_VERSION 1
#define VIO_CAMERA_MAX_SLOTS 256
#define VIO_CAMERA_MAX_PARAMS 16
#define VIO_CAMERA_MAX_POINTS 4096                  /* per item; VIO_REJECT_MAX_POINTS */
#define VIO_CAMERA_MAX_ITEMS 4096                   /* items per call; VIO_REJECT_MAX_ITEMS */
#define VIO_CAMERA_KB_BISECTIONS 12                 /* of [0, theta_max], per point */
#define VIO_CAMERA_KB_NEWTON 8                      /* safeguarded Newton steps behind them */
#define VIO_CAMERA_KB_GRID 4096                     /* intervals of the monotonicity check of vio_camera_set */
#define VIO_CAMERA_KB_DEFAULT_THETA_MAX 3.14159265358979323846
#define VIO_CAMERA_KB_RAY_C 3.6                     /* the tests' bound on a ray component: C 2^-53, absolute */

/* The numbering of VIO_REJECT_MODEL_*. */
#define VIO_CAMERA_MODEL_PINHOLE 0
#define VIO_CAMERA_MODEL_KANNALA_BRANDT 1
#define VIO_CAMERA_MODEL_MEI 2
#define VIO_CAMERA_MODEL_SCARAMUZZA 3

typedef struct vio_camera vio_camera;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_camera_create(int32_t device, void *stream, vio_camera **out);
void vio_camera_destroy(vio_camera *h);
const char *vio_camera_last_error(const vio_camera *h);    /* valid until the next call on h */
int32_t vio_camera_version(void);

typedef struct vio_camera_model {
    int32_t model;                  /* VIO_CAMERA_MODEL_* */
    int32_t width, height;          /* image_width, image_height: >= 1 */
    int32_t reserved;               /* 0 */
    double params[VIO_CAMERA_MAX_PARAMS];   /* the model's layout above; all finite */
} vio_camera_model;

/* Sets camera slot `slot` in [0, VIO_CAMERA_MAX_SLOTS).  A refused camera leaves the slot as it was. */
vio_status vio_camera_set(vio_camera *h, int32_t slot, const vio_camera_model *cam);
/* The RANSAC's settings, include/vio_reject.h's: one per handle. */
vio_status vio_camera_set_config(vio_camera *h, const vio_reject_config *cfg);

typedef struct vio_camera_lift_item {
    int32_t n;                      /* in [0, VIO_CAMERA_MAX_POINTS] */
    int32_t slot;
    const float *pts;               /* [n][2] pixels */
    double *rays;                   /* out [n][3] */
    double *angles;                 /* out [n][2] (theta, phi), or NULL; 0 for the models that have none */
} vio_camera_lift_item;

typedef struct vio_camera_lift_result {
    int32_t status;                 /* VIO_OK or VIO_ERR_NOT_FINITE */
    int32_t n_clamped;              /* KANNALA_BRANDT points beyond r(theta_max) */
} vio_camera_lift_result;

vio_status vio_camera_lift_batch(vio_camera *h, int32_t count, const vio_camera_lift_item *items, vio_camera_lift_result *results);

typedef struct vio_camera_undistort_item {
    int32_t n, m;                   /* in [0, VIO_CAMERA_MAX_POINTS] */
    const float *pts;               /* [n][2] pixels */
    const int64_t *ids;             /* [n], -1: a new point */
    const int64_t *prev_ids;        /* [m] */
    const float *prev_un_pts;       /* [m][2] */
    double dt;                      /* finite and > 0 when m > 0 */
    float *un_pts;                  /* out [n][2] */
    float *velocity;                /* out [n][2] */
    int32_t slot;
    int32_t reserved;               /* 0 */
} vio_camera_undistort_item;

/* results: [count], VIO_OK or VIO_ERR_NOT_FINITE per item, and its clamped points. */
vio_status vio_camera_undistort_batch(vio_camera *h, int32_t count, const vio_camera_undistort_item *items, vio_camera_lift_result *results);

typedef struct vio_camera_reject_item {
    int32_t n;                      /* in [0, VIO_CAMERA_MAX_POINTS] */
    uint32_t pair;                  /* enters the sampling hash */
    const float *cur_pts;           /* [n][2] pixels; may be NULL with n == 0 */
    const float *forw_pts;          /* [n][2] */
    int32_t slot;
    int32_t reserved;               /* 0 */
} vio_camera_reject_item;

/* mask: [sum of n]; pair i's part starts at the sum of the n before it; 1: keep. */
vio_status vio_camera_reject_batch(vio_camera *h, int32_t count, const vio_camera_reject_item *items, vio_reject_result *results, uint8_t *mask);

/* ms of the last call that launched: host packing + upload, the kernel (HIP events), the whole call. */
vio_status vio_camera_timing(const vio_camera *h, double *out3);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
