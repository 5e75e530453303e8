/*
 * vio_detect.h — batched Shi-Tomasi corner detection with setMask on the GPU (companion library libvio_detect_hip.so).
 *
 * The two steps of FeatureTracker::readImage that replace lost keypoints (VM/src/feature_tracker.cpp:36-69 setMask and :149
 * cv::goodFeaturesToTrack(forw_img, n_pts, MAX_CNT - forw_pts.size(), 0.01, MIN_DIST, mask)), for `count` independent images in one call:
 *   vio_detect_batch          setMask over the tracked points (k_detect_setmask), the response map and its masked maximum
 *                             (k_detect_response), the candidates (k_detect_candidates), the selection (k_detect_select)
 *   vio_detect_response       the response map of one image
 * It works from host arrays and needs nothing from libvio_hip but the vio_status type.  DESIGN.md section 20 has the layout and the
 * measurements.
 *
 * The reference detects with OpenCV, which is not part of this tree.  The contract is therefore written out here, restated in numpy
 * (tests/detect_reference.py), and the device is held to the restatement.  Every quantity is an integer up to one square root, so the
 * device agrees with the restatement in every bit and in every chosen corner: there is no tolerance anywhere.
 *
 * For one item: an 8-bit image [height][stride]; an optional 8-bit user mask of the same geometry (NULL: everything allowed, non-zero:
 * allowed; the reference's fisheye mask); n_tracked tracked points (x, y) as float with an int32 track_cnt each; max_total, the
 * reference's MAX_CNT.  The configuration holds quality (the reference's 0.01) and min_distance (MIN_DIST).  The block size
 * VIO_DETECT_BLOCK = 3 and the Sobel aperture VIO_DETECT_APERTURE = 3 are constants: the integer bounds below depend on them.
 *
 *   1. setMask.  The tracked points are ordered by (track_cnt descending, index ascending).  std::sort in the reference is unstable
 *      and leaves ties open; the index tie-break is this library's choice.  c = (cvRound(x), cvRound(y)), rounded ties-to-even.  A
 *      point is kept iff the user mask at c is non-zero and no point kept earlier has a centre c' with |c - c'|^2 <= min_distance^2.
 *      A kept point forbids the disc |p - c|^2 <= min_distance^2.  Deviation: cv::circle's filled rasterisation differs from this
 *      disc at a few boundary pixels.  Kept points leave in this order (the reference reorders forw_pts / ids / track_cnt the same
 *      way): keep_order holds their indices.
 *   2. Response.  gx, gy are the 3 x 3 Sobel ([-1 0 1; -2 0 2; -1 0 1] and its transpose) of the image with BORDER_REFLECT_101, as
 *      integers (|g| <= 1020).  a = sum gx^2, b = sum gx gy, c = sum gy^2 are the un-normalised 3 x 3 box sums of the product maps,
 *      the product maps again extended with BORDER_REFLECT_101, as cv::cornerMinEigenVal does; they are exact in int32
 *      (<= 9 363 600).  R = 0.5 * ((double)(a + c) - sqrt((double)((a - c)^2 + 4 b^2))).  The radicand is formed in int64
 *      (<= 4.4e14 < 2^53), so it is exact as a double; the square root is IEEE correctly rounded; the subtraction rounds once; the
 *      product with 0.5 is exact.  (a + c)^2 - radicand = 4 (a c - b^2) >= 0, so R >= 0 always, and R has one defined bit pattern
 *      per pixel.  Deviation: OpenCV scales the gradients by 1 / (255 * 4 * 3) and works in float32.  The scale cancels against the
 *      relative threshold; only float32 ties can choose differently.
 *   3. Candidates.  allowed(p) = the user mask is non-zero at p and p is in no kept point's disc.  maxR = the maximum of R over the
 *      allowed pixels of the whole image (minMaxLoc with the mask), 0 if none is allowed.  t = maxR * quality, one double product.  A
 *      pixel with 1 <= x <= W - 2, 1 <= y <= H - 2 is a candidate iff it is allowed, R > t and R > 0, and R >= each of its 8
 *      neighbours (threshold-to-zero, 3 x 3 dilate, equality: plateaus pass whole).  Images narrower or lower than 3 have none.
 *   4. Selection.  n_want = max_total - n_kept; n_want <= 0: no new corners.  Candidates are taken in the order (R descending, pixel
 *      index y W + x descending: OpenCV's greaterThanPtr).  One is accepted iff no corner accepted earlier in this call has
 *      dx^2 + dy^2 < min_distance^2 (OpenCV's strict <; the mask has dealt with the kept points; with min_distance < 1 every candidate
 *      is accepted in order).  Stop at n_want.  Accepted corners leave as float (x, y) in acceptance order.
 *
 * Every comparison above is on integers or on doubles that are exact or correctly rounded, and the only sum across threads is an
 * integer maximum of bit patterns, so neither contraction nor the order of arrival can change a bit.  The library is compiled with
 * contraction off all the same, as libvio_flow_hip is: there is no product followed by a sum in double for it to fuse.
 *
 * Rules (those of include/vio_flow.h):
 *   - argument errors (count < 0, a NULL array, width or height below 1 or above VIO_DETECT_MAX_DIM, stride < width, n_tracked or
 *     max_total outside [0, VIO_DETECT_MAX_POINTS], a finite tracked point whose rounded position is outside the image) write nothing
 *     and launch nothing: VIO_ERR_BAD_ARG, vio_detect_last_error names the item.  count == 0 does nothing and returns VIO_OK;
 *   - an item with a non-finite tracked point gets VIO_ERR_NOT_FINITE with n_kept = n_new = n_candidates = 0, max_response = 0 and
 *     keep_order all -1; the other items are computed as if it were not there, and the call returns VIO_ERR_NOT_FINITE;
 *   - repeated calls are bitwise identical, and an item's result does not depend on the batch it is in (no floating-point atomics;
 *     the candidates' order of arrival is arbitrary and nothing after it depends on it);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_DETECT_H
#define VIO_DETECT_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_DETECT_VERSION 1
#define VIO_DETECT_MAX_DIM 16384                    /* width and height, as VIO_FLOW_MAX_DIM */
#define VIO_DETECT_MAX_POINTS 4096                  /* bounds n_tracked and max_total */
#define VIO_DETECT_BLOCK 3                          /* the box of the products */
#define VIO_DETECT_APERTURE 3                       /* the Sobel kernel */
#define VIO_DETECT_DEFAULT_QUALITY 0.01
#define VIO_DETECT_DEFAULT_MIN_DISTANCE 30          /* MIN_DIST */
#define VIO_DETECT_DEFAULT_MAX_TOTAL 150            /* MAX_CNT */
#define VIO_DETECT_TILE_X 32                        /* the tile of k_detect_response and k_detect_candidates (for the tests' shapes) */
#define VIO_DETECT_TILE_Y 8

typedef struct vio_detect vio_detect;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_detect_create(int32_t device, void *stream, vio_detect **out);
void vio_detect_destroy(vio_detect *h);
const char *vio_detect_last_error(const vio_detect *h);    /* valid until the next call on h */
int32_t vio_detect_version(void);

typedef struct vio_detect_config {
    double quality;                 /* in (0, 1] */
    int32_t min_distance;           /* >= 0 */
    int32_t reserved;               /* 0 */
} vio_detect_config;
vio_status vio_detect_set_config(vio_detect *h, const vio_detect_config *cfg);

/* One image, its tracked points and the arrays its results go to. */
typedef struct vio_detect_item {
    int32_t width, height;
    int32_t stride;                 /* bytes between rows of the image and of the mask, >= width */
    int32_t n_tracked;              /* in [0, VIO_DETECT_MAX_POINTS] */
    int32_t max_total;              /* in [0, VIO_DETECT_MAX_POINTS] */
    int32_t reserved;               /* 0 */
    const uint8_t *img;             /* [height][stride] */
    const uint8_t *mask;            /* [height][stride], or NULL: everything allowed */
    const float *tracked;           /* [n_tracked][2] (x, y); may be NULL with n_tracked == 0 */
    const int32_t *track_cnt;       /* [n_tracked] */
    int32_t *keep_order;            /* out [n_tracked]: the indices of the kept points in output order, then -1 */
    float *new_pts;                 /* out [max_total][2]: the first n_new rows are written; may be NULL with max_total == 0 */
} vio_detect_item;

typedef struct vio_detect_result {
    int32_t status;                 /* VIO_OK or VIO_ERR_NOT_FINITE */
    int32_t n_kept;
    int32_t n_new;
    int32_t n_candidates;
    double max_response;            /* maxR of step 3 */
} vio_detect_result;

vio_status vio_detect_batch(vio_detect *h, int32_t count, const vio_detect_item *items, vio_detect_result *results);

/* Step 2 alone: the response map of one image, out[height][width] doubles. */
vio_status vio_detect_response(vio_detect *h, const uint8_t *img, int32_t width, int32_t height, int32_t stride, double *out);

/* ms of the last vio_detect_batch that launched: host packing + upload, k_detect_setmask, k_detect_response, k_detect_candidates,
 * k_detect_select (HIP events), the whole call. */
vio_status vio_detect_timing(const vio_detect *h, double *out6);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
