/*
 * vio_clahe.h — batched CLAHE image equalisation on the GPU (companion library libvio_clahe_hip.so).
 *
 * The first step of FeatureTracker::readImage with EQUALIZE set, as both of the reference's configurations have it
 * (VM/src/feature_tracker.cpp:87-95: cv::createCLAHE(3.0, cv::Size(8, 8))->apply(_img, img)), for `count` independent images in one call:
 *   vio_clahe_apply_batch     the tiles' look-up tables (k_clahe_lut), then the blended image (k_clahe_apply)
 * It works from host arrays and needs nothing from libvio_hip but the vio_status type.  DESIGN.md section 22 has the layout and the
 * measurements.
 *
 * The reference equalises with OpenCV, which is not part of this tree.  The contract is therefore written out here, restated in numpy
 * (tests/clahe_reference.py), and the device is held to the restatement in every byte: there is no tolerance anywhere.  Agreement with
 * OpenCV itself is unpinned: the steps below follow its CLAHE for 8-bit images, no OpenCV build has been compared with them.
 *
 * Images are 8-bit with one channel; there are VIO_CLAHE_BINS = 256 bins.  The configuration holds clip_limit (the reference's 3.0;
 * 0: no clipping) and the tile grid tiles_x x tiles_y (8 x 8), each in [1, VIO_CLAHE_MAX_TILES].  For one W x H image:
 *
 *   1. Tiling.  If W % tiles_x == 0 and H % tiles_y == 0 the histograms are taken of the image itself.  Otherwise they are taken of the
 *      image extended on the right by tiles_x - W % tiles_x columns and at the bottom by tiles_y - H % tiles_y rows with
 *      BORDER_REFLECT_101.  That is cv::copyMakeBorder as CLAHE calls it, kept as it is: a direction that divides still gets a whole
 *      extra tiles_x or tiles_y (16 x 13 with 8 x 8 tiles becomes 24 x 16).  The extension can exceed the image (1 x 1 gets 7), so the
 *      reflection has the period 2 (n - 1): position i reads m = i mod 2 (n - 1) if m < n, else 2 (n - 1) - m; for n = 1 it reads 0.
 *      tile_w = W_ext / tiles_x, tile_h = H_ext / tiles_y, area = tile_w tile_h.  W and H are at most VIO_CLAHE_MAX_DIM, so every
 *      count fits an int32.
 *   2. Clip limit.  clip = 0 if clip_limit == 0; otherwise clip = max((int)min(clip_limit area / 256, area), 1), formed in double and
 *      truncated (no bin exceeds area, so the bound changes no result; it keeps the conversion defined for every clip_limit).
 *      lut_scale = (float)255 / (float)area, one float32 division; inv_tile_w = 1.0f / (float)tile_w and inv_tile_h likewise.  The
 *      three are computed on the host and handed to the kernels: no device division enters the contract.
 *   3. Per tile.  hist[256] of the tile's source pixels.  If clip > 0: excess = sum max(hist[i] - clip, 0), hist[i] = min(hist[i], clip);
 *      batch = excess / 256, residual = excess - 256 batch; every bin gets + batch; if residual > 0, step = max(256 / residual, 1) and
 *      the bins 0, step, 2 step, ... get + 1 each while the index is below 256 and residual, decremented for each, is positive
 *      (OpenCV's loop; it may leave some residual undistributed).  In closed form bin b gets + 1 iff b % step == 0 and
 *      b / step < residual.
 *   4. LUT.  sum_i the inclusive prefix sum of the bins; lut[i] = saturate_u8(rint((float)sum_i * lut_scale)): one float32 product,
 *      rounded to nearest, ties to even.
 *   5. Blend, for the output pixel (x, y) of value v, in float32 with no contraction:
 *      txf = (float)x * inv_tile_w - 0.5f, tx1 = floor(txf), xa = txf - (float)tx1, xa1 = 1.0f - xa; then tx2 = min(tx1 + 1, tiles_x - 1)
 *      and tx1 = max(tx1, 0); the same in y.
 *      res = (lut[ty1][tx1][v] * xa1 + lut[ty1][tx2][v] * xa) * ya1 + (lut[ty2][tx1][v] * xa1 + lut[ty2][tx2][v] * xa) * ya, in exactly
 *      this association; out = saturate_u8(rint(res)).  A fused multiply-add changes bytes (res lies exactly on a half for thousands
 *      of pixels of an ordinary image), so the library is compiled with contraction off, as libvio_flow_hip and libvio_detect_hip are.
 *
 * Histograms, clip and redistribution are integers, the LUT is one rounded product per entry and the blend a fixed sequence of float32
 * operations per pixel: nothing depends on the order in which threads arrive.
 *
 * Rules (those of include/vio_detect.h):
 *   - argument errors (count < 0, a NULL array, width or height below 1 or above VIO_CLAHE_MAX_DIM, src_stride or dst_stride < width,
 *     a NULL src or dst, dst overlapping src) write nothing and launch nothing: VIO_ERR_BAD_ARG, vio_clahe_last_error names the
 *     item.  count == 0 does nothing and returns VIO_OK;
 *   - repeated calls are bitwise identical, and an item's result does not depend on the batch it is in (integer atomics only);
 *   - the items of one call may differ in size; they share the handle's configuration;
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_CLAHE_H
#define VIO_CLAHE_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_CLAHE_VERSION 1
#define VIO_CLAHE_MAX_DIM 16384                     /* width and height, as VIO_FLOW_MAX_DIM */
#define VIO_CLAHE_MAX_TILES 16                      /* bounds tiles_x and tiles_y */
#define VIO_CLAHE_BINS 256
#define VIO_CLAHE_DEFAULT_CLIP_LIMIT 3.0
#define VIO_CLAHE_DEFAULT_TILES 8
#define VIO_CLAHE_TILE_X 128                        /* the pixels a workgroup of k_clahe_apply covers (for the tests' shapes) */
#define VIO_CLAHE_TILE_Y 16

typedef struct vio_clahe vio_clahe;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_clahe_create(int32_t device, void *stream, vio_clahe **out);
void vio_clahe_destroy(vio_clahe *h);
const char *vio_clahe_last_error(const vio_clahe *h);      /* valid until the next call on h */
int32_t vio_clahe_version(void);

typedef struct vio_clahe_config {
    double clip_limit;              /* finite, >= 0; 0: no clipping */
    int32_t tiles_x, tiles_y;       /* in [1, VIO_CLAHE_MAX_TILES] */
} vio_clahe_config;
vio_status vio_clahe_set_config(vio_clahe *h, const vio_clahe_config *cfg);

/* One image and the arrays its results go to. */
typedef struct vio_clahe_item {
    int32_t width, height;
    int32_t src_stride, dst_stride; /* bytes between rows, >= width */
    const uint8_t *src;             /* [height][src_stride] */
    uint8_t *dst;                   /* out [height][dst_stride]: width bytes of every row are written; may not overlap src */
    uint8_t *luts;                  /* out [tiles_y][tiles_x][256], or NULL */
} vio_clahe_item;

typedef struct vio_clahe_result {
    int32_t status;                 /* VIO_OK */
    int32_t clip;                   /* step 2 */
    int32_t tile_w, tile_h;         /* step 1 */
} vio_clahe_result;

vio_status vio_clahe_apply_batch(vio_clahe *h, int32_t count, const vio_clahe_item *items, vio_clahe_result *results);

/* ms of the last vio_clahe_apply_batch that launched: host packing + upload, k_clahe_lut, k_clahe_apply (HIP events), the whole call. */
vio_status vio_clahe_timing(const vio_clahe *h, double *out4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
