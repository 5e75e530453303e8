/*
 * vio_flow.h — batched pyramidal Lucas-Kanade feature tracking on the GPU (companion library libvio_flow_hip.so).
 *
 * The step of FeatureTracker::readImage that makes the tracks (VM/src/feature_tracker.cpp:108-125: cv::calcOpticalFlowPyrLK and the
 * inBorder test), for `count` independent image pairs in one call:
 *   vio_flow_track_batch      the pyramids of every image of the call (k_flow_pyr_down, one launch per level), then every keypoint of
 *                             every pair, one wavefront per keypoint                                            (k_flow_track)
 *   vio_flow_pyramid          the pyramid levels of one image
 *   vio_flow_set_back         the forward-backward check inside k_flow_track, off by default        (include/vio_flow_back.h)
 * It works from host arrays and needs nothing from libvio_hip but the vio_status type.  DESIGN.md section 19 has the layout and the
 * measurements.
 *
 * The reference tracks with OpenCV.  What replaces it is the reference's own hand-written tracker, OpticalFlowSingleLevel and
 * OpticalFlowMultiLevel of A/06-frontend-direct-method/01-optical-flow/optical_flow.cpp, restated so that the work is fixed and
 * repeatable (tests/flow_reference.py restates it in numpy and the device is held to that):
 *   - Pyramid.  Level 0 is the 8-bit image, level k + 1 is cv::pyrDown of level k to (W / 2, H / 2) (integer division): the
 *     separable 5-tap [1 4 6 4 1] with BORDER_REFLECT_101 in integers, out = (sum + 128) >> 8.  Every level must be at least 2 x 2.
 *   - Gradients.  cv::Scharr(CV_64F): [-3 0 3; -10 0 10; -3 0 3] and its transpose with BORDER_REFLECT_101, integers, computed on the
 *     fly from the 8-bit level.  The bilinearly interpolated gradient is divided by VIO_FLOW_GRADIENT_DIVISOR = 26.0 as the reference
 *     does (the normalisation of these kernels is 32; the quirk is kept).
 *   - Bilinear interpolation at (x, y): x0 = int(x), x1 = x0 + 1, xx = x - x0 (the same in y),
 *     (1 - xx) (1 - yy) v(y0, x0) + xx (1 - yy) v(y0, x1) + (1 - xx) yy v(y1, x0) + xx yy v(y1, x1), left to right.  x1 and y1 are
 *     clamped to the image: x + du can round up to an integer, and then the reference reads one pixel past the patch with weight 0.
 *   - IsValidPatch(x, y): half_patch <= int(x), int(x) + 1 <= W - half_patch and the same in y.  Restated on the doubles as
 *     half_patch <= x < W - half_patch, which is the same test for every x an int can hold and is false for the others.
 *   - One level, per keypoint at (x0, y0) in the template T with the start (dx, dy) in the moving image I: nothing runs unless T's
 *     patch is valid.  Then at most max_iter iterations: x = x0 + dx, y = y0 + dy; an invalid patch in I sets success = false and
 *     ends the level (p kept).  Over the patch du, dv in [-h, h): error = T(x0 + du, y0 + dv) - I(x + du, y + dv),
 *     J = gradient of I at (x + du, y + dv) (forward mode) or of T at (x0 + du, y0 + dv) (inverse mode), H = sum J J^T (inverse mode:
 *     once per level, at the first iteration), b = sum error J, cost = sum (0.5 error) error.  dp = H^-1 b as below.  A NaN dp sets
 *     success = false and ends the level; cost_prev <= cost ends the level and leaves success as it was; otherwise p += dp and
 *     success = true.  The cost is that of the position before the step.  cost_prev starts at DBL_MAX, and the reference's
 *     State::Update never stores the new cost, so its early stop never fires: that is early_stop = 0, the default.  early_stop = 1
 *     stores the cost after every step taken, which is what the reference's comment intends.
 *   - dp = H.fullPivHouseholderQr().solve(b) of Eigen 3.3, restated for 2 x 2: the entry of largest magnitude (the first such in
 *     column-major order) is swapped to the corner; it being 0 is rank 0 and dp = 0.  One Householder reflection of the first
 *     column (tail^2 <= DBL_MIN: none; else beta = -sign(c0) sqrt(c0^2 + tail^2), v = tail / (c0 - beta), tau = (beta - c0) / beta)
 *     is applied to the second column and to b.  The second pivot is dropped if |m11| <= 2 eps times the first step's largest
 *     magnitude; the rank counts the kept pivots above 2 eps max|pivot|.  Rank 2: back substitution; rank 1: the basic solution
 *     (b0' / pivot in the pivot's column, 0 in the other).  The column swap is undone in dp.
 *   - Levels, coarse to fine.  Positions are float at every level boundary: target = (float)(prev * 0.5^l), source = target at the
 *     top level, or (float)(guess * 0.5^l) with a guess (the guess is given in level-0 pixels; the reference's non-empty kp2); (dx,
 *     dy) = source - target in double; the level's result is target + (float)(dx, dy) in float, and source = (float)(result / 0.5)
 *     for the next level.  A keypoint that failed at a coarse level carries its position on; its status is that of level 0 alone.
 *   - readImage's inBorder: a keypoint that tracked but whose position rounded to the nearest integer (ties to even, cvRound) is not in
 *     [border, W - border) x [border, H - border) gets VIO_FLOW_FAIL_BORDER.
 *
 * The order of the sums is part of this contract.  Patch pixel m = (du + h) 2h + (dv + h), the reference's loop order, belongs to
 * lane m mod 64.  Each lane adds its pixels' terms in ascending m from 0.0 into six private accumulators (H00, H01, H11, b0, b1,
 * cost); the six are reduced across the 64 lanes by the butterfly v[i] += v[i ^ s] for s = 1, 2, 4, 8, 16, 32.  IEEE addition is
 * commutative, so every lane ends with the same bits, and every lane runs the 2 x 2 solve and the decision on them.  Every product
 * and sum is rounded on its own (no contraction).  A keypoint's result depends on its own inputs alone.
 *
 * Rules (those of include/vio_pnp.h):
 *   - argument errors (count < 0, a NULL array, width or height below 1 or above VIO_FLOW_MAX_DIM, stride < width, a pyramid level
 *     smaller than 2 x 2, n_pts outside [0, VIO_FLOW_MAX_POINTS]) write nothing and launch nothing: VIO_ERR_BAD_ARG,
 *     vio_flow_last_error names the item.  count == 0 and n_pts == 0 do nothing and return VIO_OK;
 *   - a keypoint whose position or guess is not finite gets VIO_ERR_NOT_FINITE and NaN; the others are computed as if it were not
 *     there, and the call returns VIO_ERR_NOT_FINITE.  A keypoint that is lost is an outcome, not an error;
 *   - repeated calls are bitwise identical, and a keypoint's result depends neither on the batch nor on the item it is in (no
 *     floating-point atomics, the summation order above);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_FLOW_H
#define VIO_FLOW_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FLOW_VERSION 1
#define VIO_FLOW_MAX_LEVELS 8
#define VIO_FLOW_MAX_HALF_PATCH 16
#define VIO_FLOW_MAX_POINTS 4096                    /* keypoints per item */
#define VIO_FLOW_MAX_DIM 16384                      /* width and height */
#define VIO_FLOW_DEFAULT_LEVELS 4                   /* NUM_PYRAMIDS */
#define VIO_FLOW_DEFAULT_HALF_PATCH 4               /* HALF_PATCH_SIZE */
#define VIO_FLOW_DEFAULT_MAX_ITER 10                /* MAX_ITERATIONS */
#define VIO_FLOW_DEFAULT_BORDER 1                   /* BORDER_SIZE */
#define VIO_FLOW_GRADIENT_DIVISOR 26.0
#define VIO_FLOW_HAS_BACK 1                         /* include/vio_flow_back.h is there: the forward-backward check */

/* Per-keypoint outcomes besides VIO_OK and VIO_ERR_NOT_FINITE. */
#define VIO_FLOW_FAIL_LOST 1            /* the reference's success = false at level 0 */
#define VIO_FLOW_FAIL_BORDER 2          /* tracked, but the rounded position is outside the border (readImage's inBorder) */

typedef struct vio_flow vio_flow;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_flow_create(int32_t device, void *stream, vio_flow **out);
void vio_flow_destroy(vio_flow *h);
const char *vio_flow_last_error(const vio_flow *h);        /* valid until the next call on h */
int32_t vio_flow_version(void);

typedef struct vio_flow_config {
    int32_t levels;                 /* in [1, VIO_FLOW_MAX_LEVELS] */
    int32_t half_patch;             /* in [1, VIO_FLOW_MAX_HALF_PATCH]: the patch is 2 half_patch x 2 half_patch */
    int32_t max_iter;               /* in [1, 1000] */
    int32_t inverse;                /* 0: forward-additive, 1: inverse */
    int32_t border;                 /* >= 0 */
    int32_t early_stop;             /* 0: the reference as written (the cost is never stored), 1: stop when the cost rises */
} vio_flow_config;
vio_status vio_flow_set_config(vio_flow *h, const vio_flow_config *cfg);

/* One image pair and the keypoints to follow from img_prev into img_next. */
typedef struct vio_flow_item {
    int32_t width, height;
    int32_t stride;                 /* bytes between rows of both images, >= width */
    int32_t n_pts;                  /* in [0, VIO_FLOW_MAX_POINTS] */
    const uint8_t *img_prev;        /* [height][stride] */
    const uint8_t *img_next;
    const float *prev_pts;          /* [n_pts][2] (x, y) in img_prev */
    const float *guess;             /* [n_pts][2] start positions in img_next, or NULL: start at prev_pts */
} vio_flow_item;

typedef struct vio_flow_pt_info {
    int32_t status;                 /* VIO_OK, VIO_FLOW_FAIL_*, VIO_ERR_NOT_FINITE */
    int32_t iterations;             /* level 0's iterations whose sums were formed */
    double cost;                    /* the last of them's cost (NaN if there was none) */
} vio_flow_pt_info;

/* next_pts: [sum of n_pts][2], info: [sum of n_pts] or NULL; item i's part starts at the sum of the n_pts before it.  next_pts is
 * the position the reference leaves, tracked or not (NaN for VIO_ERR_NOT_FINITE). */
vio_status vio_flow_track_batch(vio_flow *h, int32_t count, const vio_flow_item *items, float *next_pts, vio_flow_pt_info *info);

/* The configured levels of one image, level 0 first, each tightly packed: out holds the sum over the levels of w_k * h_k bytes. */
vio_status vio_flow_pyramid(vio_flow *h, const uint8_t *img, int32_t width, int32_t height, int32_t stride, uint8_t *out);

/* ms of the last call that launched: host packing + upload, k_flow_pyr_down (all levels), k_flow_track (HIP events), the whole call. */
vio_status vio_flow_timing(const vio_flow *h, double *out4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#include "vio_flow_back.h"

#endif
