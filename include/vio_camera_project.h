/*
 * vio_camera_project.h — spaceToPlane of the four camera models of include/vio_camera.h, batched, in the same library
 * (libvio_camera_hip.so) and on the same handle and camera slots:
 *   vio_camera_set_inv_poly      SCARAMUZZA's inv_poly_parameters of one slot
 *   vio_camera_project_batch     spaceToPlane of `count` point sets, each through its own slot's camera          (k_camera_project)
 * A point is (P0, P1, P2) in the camera frame, in double; the pixel is (u, v) in double.  The arithmetic is csrc/vio_camera_project_math.h
 * and follows the rules of csrc/vio_camera_math.h: the reference's operation order, every product and sum rounded on its own (no
 * contraction), no function of a math library but sqrt, floor and fma (atan2, sin and cos are vio_camera_math.h's own), so the device,
 * a host build and the numpy restatement (tests/camera_project_reference.py) agree in every bit.
 *
 * Per model (params[] named as include/vio_camera.h lists them):
 *   PINHOLE      PinholeCamera.cc:531-553.  p_u = (P0 / P2, P1 / P2); p_d = p_u + distortion(p_u) with the lift's distortion function,
 *                or p_u when the slot has no distortion (k1 = k2 = p1 = p2 = 0); the pixel is (fx p_d0 + cx, fy p_d1 + cy).
 *   MEI          CataCamera.cc:636-659.  z = P2 + xi |P| with |P| = sqrt((P0 P0 + P1 P1) + P2 P2); p_u = (P0 / z, P1 / z); the same
 *                distortion; the pixel is (gamma1 p_d0 + u0, gamma2 p_d1 + v0).
 *   SCARAMUZZA   ScaramuzzaCamera.cc:632-653.  norm = sqrt(P0 P0 + P1 P1); theta = atan2(-P2, norm); rho = sum theta^i inv_poly[i],
 *                accumulated as written (rho += theta_i c_i; theta_i *= theta) over the VIO_CAMERA_INV_POLY_MAX entries, those beyond
 *                the n that were set being 0; invNorm = 1 / norm; xn = (P0 invNorm rho, P1 invNorm rho); the pixel is
 *                (xn0 ac + xn1 ad + cx, xn0 ae + xn1 + cy).  A point on the axis has norm = 0 and, as in the reference, no finite pixel.
 *   KANNALA_BRANDT   EquidistantCamera.cc:451-461.  phi = atan2(P1, P0); p_u = r(theta) (cos phi, sin phi) with r the polynomial
 *                theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9 (Horner in theta^2, as the lift's root solve has it); the
 *                pixel is (mu p_u0 + u0, mv p_u1 + v0).
 *                Deviation: the reference takes theta = acos(P2 / |P|).  This library has no acos, and acos loses half its digits near
 *                the axis; theta = atan2(sqrt(P0 P0 + P1 P1), P2) here, the same angle.  theta is not clamped to the slot's theta_max.
 *
 * Flags.  flags[i] is 0 for a usable pixel, otherwise the OR of
 *   VIO_CAMERA_PROJECT_NOT_FINITE   a coordinate of the point or of the pixel is not finite; the pixel is then (NaN, NaN)
 *   VIO_CAMERA_PROJECT_BEHIND       the model's denominator is not positive (P2 <= 0 for PINHOLE, z <= 0 for MEI); the pixel is what the
 *                                   arithmetic gives (P2 == 0 sets both bits).  The other two models project every direction.
 * One flagged point does not touch the others.  An item with a VIO_CAMERA_PROJECT_NOT_FINITE point has status VIO_ERR_NOT_FINITE (its
 * other points are computed), and the call then returns VIO_ERR_NOT_FINITE, as vio_camera_lift_batch does for a pixel that is not
 * finite; VIO_CAMERA_PROJECT_BEHIND alone leaves VIO_OK.  n_flagged counts the points whose flag is not 0.
 *
 * Accuracy.  Against a 50-digit evaluation of the reference's formulas as written (acos and atan2 included) on the same double inputs,
 * over rays from the axis to theta_max of the tests' four cameras, the largest error of a pixel coordinate is
 * VIO_CAMERA_PROJECT_C_MEASURED pixels (tests/test_camera_project_accuracy.py); VIO_CAMERA_PROJECT_C is that figure doubled and rounded
 * up, the tests' absolute bound in pixels.
 *
 * Rules: those of include/vio_camera.h (argument errors write nothing and launch nothing; count == 0 returns VIO_OK; one launch and one
 * wait per call; repeated calls are bitwise identical and an item's result depends neither on its batch nor on its slot's number; the
 * caller's HIP device is restored).  Argument errors of vio_camera_project_batch: count outside [0, VIO_CAMERA_MAX_ITEMS], a NULL array,
 * n outside [0, VIO_CAMERA_MAX_POINTS], points or pixels NULL with n > 0, a slot out of range or never set, a SCARAMUZZA slot without
 * inv_poly.
 *
 * Not built: the Jacobians of spaceToPlane; device-to-device hand-over of the points.
 */
#ifndef VIO_CAMERA_PROJECT_H
#define VIO_CAMERA_PROJECT_H

#include "vio_camera.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_CAMERA_HAS_PROJECT 1
#define VIO_CAMERA_INV_POLY_MAX 20                  /* SCARAMUZZA_INV_POLY_SIZE */
#define VIO_CAMERA_PROJECT_NOT_FINITE 1
#define VIO_CAMERA_PROJECT_BEHIND 2
#define VIO_CAMERA_PROJECT_C_MEASURED 1.38e-13      /* pixels: the largest error the accuracy test measures (a pixel coordinate of 600) */
#define VIO_CAMERA_PROJECT_C 3e-13                  /* pixels: the tests' bound, the measured figure doubled and rounded up */

/* inv_poly_parameters of SCARAMUZZA slot `slot`: n in [1, VIO_CAMERA_INV_POLY_MAX] coefficients, all finite, lowest power first.  The
 * slot must hold a SCARAMUZZA camera (VIO_ERR_BAD_ARG otherwise, the slot as it was).  A later vio_camera_set on the slot clears them. */
vio_status vio_camera_set_inv_poly(vio_camera *h, int32_t slot, int32_t n, const double *inv_poly);

typedef struct vio_camera_project_item {
    int32_t n;                      /* in [0, VIO_CAMERA_MAX_POINTS] */
    int32_t slot;
    const double *points;           /* [n][3] in the camera frame */
    double *pixels;                 /* out [n][2] */
    uint8_t *flags;                 /* out [n], or NULL */
} vio_camera_project_item;

typedef struct vio_camera_project_result {
    int32_t status;                 /* VIO_OK or VIO_ERR_NOT_FINITE */
    int32_t n_flagged;              /* points whose flag is not 0 */
} vio_camera_project_result;

vio_status vio_camera_project_batch(vio_camera *h, int32_t count, const vio_camera_project_item *items, vio_camera_project_result *results);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
