/*
 * vio_fm.h — the FeatureManager of many streams on the GPU (companion library libvio_fm_hip.so).
 *
 * The reference's FeatureManager (VM/src/feature_manager.cpp) sits between the front end's (ids, normalised points) per image and the
 * window arrays the back end takes.  Here a handle keeps up to VIO_FM_MAX_SLOTS track lists resident on the device, one per stream
 * ("slot"), and every method runs for `count` slots in one launch, one workgroup per slot, with one wait:
 *   vio_fm_add_batch             addFeatureCheckParallax (:45-97), the keyframe decision included              (k_fm_add)
 *   vio_fm_export_batch          triangulate (:202-257), getDepthVector, the edge loop of estimator.cpp:975-1016:
 *                                the arrays vio_set_landmarks and vio_set_observations take                     (k_fm_export)
 *   vio_fm_set_depth_batch       setDepth / clearDepth, removeFailures (:141-182)                               (k_fm_set_depth)
 *   vio_fm_slide_batch           removeBackShiftDepth, removeBack, removeFront (:276-354)                       (k_fm_slide)
 *   vio_fm_corresponding_batch   getCorresponding (:120-139)                                                    (k_fm_corresponding)
 *   vio_fm_tracks_set / _get     seed and download one slot's list                                              (copies)
 * It works from host arrays and needs nothing from libvio_hip but the vio_status type.  DESIGN.md section 26 has the layout, the
 * kernels and the measurements.
 *
 * A row of a slot's table is one FeaturePerId: feature_id (int64, as the front end's ids are), start_frame, the number of
 * observations, estimated_depth (double; -1 when new), solve_flag, and the observations' normalised (x, y) as doubles with z = 1
 * implied.  uv, velocity and td of FeaturePerFrame are not carried: nothing in this project reads them downstream, and td is not
 * estimated.  Row order is the reference's list order, that is insertion order; every operation preserves it.  A slot's table
 * (VIO_FM_MAX_TRACKS rows of VIO_FM_MAX_OBS observations, about 420 KB) is allocated at the slot's first use.
 *
 * After every call the handle knows each slot's three counts from that call's read-back: n_tracks, n_landmarks (getFeatureCount():
 * rows with n_obs >= 2 && start_frame < WINDOW_SIZE - 2, "usable" below) and n_observations (the sum of n_obs - 1 over those).
 * vio_fm_counts returns them; they size the arrays of vio_fm_export_batch and vio_fm_set_depth_batch exactly.
 *
 * The order of the one floating-point sum is part of this contract.  parallax_sum of vio_fm_add_batch: the term of row r is
 * sqrt(du * du + dv * dv) with du = x_i / 1.0 - x_j, dv = y_i / 1.0 - y_j (compensatedParallax2 with its identity compensation; no
 * contraction), 0.0 for a row the reference's test skips.  Thread t of 1024 sums (0.0 + term[t]) + term[t + 1024]; the 1024 partial
 * sums are then reduced by the tree s[t] += s[t + w] for w = 512, 256, ..., 1.  The reference sums in list order; two orders over n
 * non-negative terms differ by at most 2 (n - 1) 2^-53 of the sum.  The depth shift of removeBackShiftDepth is evaluated as
 * csrc/vio_fm_math.h's fm_shift_depth writes it down (left to right, no contraction).
 *
 * Rules:
 *   - argument errors write nothing and launch nothing for the whole call (VIO_ERR_BAD_ARG, vio_fm_last_error names the item): count
 *     outside [0, VIO_FM_MAX_SLOTS], a NULL array, a slot outside [0, VIO_FM_MAX_SLOTS) or listed twice, a count out of range
 *     (frame_count outside [0, 10], n outside [0, VIO_FM_MAX_POINTS], l or r outside 0 <= l <= r <= 10, n != n_landmarks, an output
 *     capacity below the slot's counts), a non-finite point, pose or depth, duplicate ids within one item;
 *   - rules only the device can check leave that slot exactly as it was (a check phase, a barrier, then the write phase), give the
 *     slot's result a VIO_FM_STATUS_* and do not touch the other slots of the call (the call returns VIO_OK): the table would exceed
 *     VIO_FM_MAX_TRACKS rows, a matched track does not end at frame_count - 1, a track would get a twelfth observation (where
 *     several are broken the status names the first of: table full, twelfth observation, gap);
 *   - repeated calls are bitwise identical, and a slot's result depends neither on the batch nor on the slot index (no
 *     floating-point atomics, the summation order above);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_FM_H
#define VIO_FM_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_FM_VERSION 1
#define VIO_FM_MAX_SLOTS 256
#define VIO_FM_MAX_TRACKS 2048                      /* rows of a slot's table */
#define VIO_FM_MAX_POINTS 1024                      /* points of one image: VIO_FRAME_MAX_TRACK_POINTS */
#define VIO_FM_MAX_OBS 11                           /* observations of a track: WINDOW_SIZE + 1 */
#define VIO_FM_DEFAULT_INIT_DEPTH 5.0               /* INIT_DEPTH */
#define VIO_FM_DEFAULT_MIN_PARALLAX (10.0 / 460.0)  /* MIN_PARALLAX = 10 / FOCAL_LENGTH */

/* A slot's status in a result: a rule only the device can check; the slot is as it was. */
#define VIO_FM_STATUS_OK 0
#define VIO_FM_STATUS_TABLE_FULL 1                  /* the new tracks would not fit into VIO_FM_MAX_TRACKS rows */
#define VIO_FM_STATUS_GAP 2                         /* a matched track does not end at frame_count - 1 */
#define VIO_FM_STATUS_OBS_FULL 3                    /* a matched track has VIO_FM_MAX_OBS observations already */

#define VIO_FM_DEPTH_SET 0                          /* setDepth: solve_flag 1, or 2 for a negative depth */
#define VIO_FM_DEPTH_CLEAR 1                        /* clearDepth: the flags stay */

#define VIO_FM_BACK_SHIFT_DEPTH 0                   /* removeBackShiftDepth(marg_R, marg_P, new_R, new_P) */
#define VIO_FM_BACK 1                               /* removeBack */
#define VIO_FM_FRONT 2                              /* removeFront(frame_count) */

typedef struct vio_fm vio_fm;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
vio_status vio_fm_create(int32_t device, void *stream, vio_fm **out);
void vio_fm_destroy(vio_fm *h);
const char *vio_fm_last_error(const vio_fm *h);            /* valid until the next call on h */
int32_t vio_fm_version(void);

typedef struct vio_fm_config {
    double init_depth;              /* finite and > 0; default VIO_FM_DEFAULT_INIT_DEPTH */
    double min_parallax;            /* finite and >= 0; default VIO_FM_DEFAULT_MIN_PARALLAX */
} vio_fm_config;
vio_status vio_fm_set_config(vio_fm *h, const vio_fm_config *cfg);

/* clearState of one slot: its list is empty afterwards (the table stays allocated). */
vio_status vio_fm_reset(vio_fm *h, int32_t slot);
/* The slot's counts as the last call left them; any of the three may be NULL. */
vio_status vio_fm_counts(const vio_fm *h, int32_t slot, int32_t *n_tracks, int32_t *n_landmarks, int32_t *n_observations);

/* What every batched call returns per item.  The fields after the counts belong to one call each and are 0 in the others. */
typedef struct vio_fm_result {
    int32_t status;                 /* VIO_FM_STATUS_* */
    int32_t n_tracks;               /* the slot's counts after the call */
    int32_t n_landmarks;
    int32_t n_observations;
    int32_t keyframe;               /* add: addFeatureCheckParallax's return (1: marginalise the oldest) */
    int32_t last_track_num;         /* add */
    int32_t parallax_num;           /* add: 0 where a gate returned before the parallax loop */
    int32_t n_new;                  /* add: tracks appended */
    int32_t n_triangulated;         /* export: tracks whose depth was written */
    int32_t n_rows;                 /* corresponding: rows written */
    double parallax_sum;            /* add: in the order this header writes down */
} vio_fm_result;

/* addFeatureCheckParallax.  The ids may come in any order; they are taken in ascending order, as the reference's std::map iterates,
 * and new tracks are appended in that order.  frame_count < 2, last_track_num < 20 and parallax_num == 0 give keyframe = 1. */
typedef struct vio_fm_add_item {
    int32_t slot;
    int32_t frame_count;            /* in [0, 10] */
    int32_t n;                      /* in [0, VIO_FM_MAX_POINTS] */
    int32_t reserved;
    const int64_t *ids;             /* [n], distinct */
    const double *pts;              /* [n][2] normalised image points */
} vio_fm_add_item;
vio_status vio_fm_add_batch(vio_fm *h, int32_t count, const vio_fm_add_item *items, vio_fm_result *results);

/* triangulate (when `triangulate` is not 0), then getDepthVector and the edge loop.  Usable track k in list order gives
 * feature_ids[k], inv_depth[k] = 1.0 / estimated_depth, and for j = 1 .. n_obs - 1 one edge: lm = k, host = start_frame, target =
 * start_frame + j, pts_i = observation 0, pts_j = observation j.  Triangulation writes estimated_depth only for usable tracks whose
 * depth is not > 0; a depth below 0.1 becomes init_depth.  The arrays must hold the slot's n_landmarks and n_observations. */
typedef struct vio_fm_export_item {
    int32_t slot;
    int32_t triangulate;
    int32_t cap_landmarks;          /* rows of feature_ids and inv_depth: at least the slot's n_landmarks */
    int32_t cap_observations;       /* rows of the five edge arrays: at least the slot's n_observations */
    const double *poses;            /* [11][7]: P (3), Q (x, y, z, w) as vio_set_window takes them */
    const double *ext;              /* [7] */
    int64_t *feature_ids;           /* [cap_landmarks] */
    double *inv_depth;              /* [cap_landmarks] */
    int32_t *lm;                    /* [cap_observations] */
    int32_t *host;
    int32_t *target;
    double *pts_i;                  /* [cap_observations][2] */
    double *pts_j;
} vio_fm_export_item;
vio_status vio_fm_export_batch(vio_fm *h, int32_t count, const vio_fm_export_item *items, vio_fm_result *results);

/* setDepth (VIO_FM_DEPTH_SET) or clearDepth (VIO_FM_DEPTH_CLEAR) from x[n_landmarks]: estimated_depth = 1.0 / x[k] of usable track
 * k.  remove_failures != 0 then erases every row with solve_flag == 2 (removeFailures). */
typedef struct vio_fm_depth_item {
    int32_t slot;
    int32_t mode;
    int32_t remove_failures;
    int32_t n;                      /* must be the slot's n_landmarks */
    const double *x;                /* [n], finite */
} vio_fm_depth_item;
vio_status vio_fm_set_depth_batch(vio_fm *h, int32_t count, const vio_fm_depth_item *items, vio_fm_result *results);

/* The three slide rules.  VIO_FM_BACK_SHIFT_DEPTH reads the four matrices (row-major 3 x 3, 3); rows left with fewer than 2
 * observations are erased, dep_j <= 0 gives init_depth.  VIO_FM_FRONT reads frame_count; the observation it erases is the
 * reference's index WINDOW_SIZE - 1 - start_frame, and a row that does not have it is left alone. */
typedef struct vio_fm_slide_item {
    int32_t slot;
    int32_t kind;
    int32_t frame_count;            /* VIO_FM_FRONT: in [1, 10] */
    int32_t reserved;
    const double *marg_R;           /* [9]   VIO_FM_BACK_SHIFT_DEPTH only */
    const double *marg_P;           /* [3] */
    const double *new_R;            /* [9] */
    const double *new_P;            /* [3] */
} vio_fm_slide_item;
vio_status vio_fm_slide_batch(vio_fm *h, int32_t count, const vio_fm_slide_item *items, vio_fm_result *results);

/* getCorresponding(l, r): rows (x_l, y_l, x_r, y_r) of the tracks that span both frames, in list order; result.n_rows of them. */
typedef struct vio_fm_corr_item {
    int32_t slot;
    int32_t l;                      /* 0 <= l <= r <= 10 */
    int32_t r;
    int32_t cap_rows;               /* rows of `rows`: at least the slot's n_tracks */
    double *rows;                   /* [cap_rows][4] */
} vio_fm_corr_item;
vio_status vio_fm_corresponding_batch(vio_fm *h, int32_t count, const vio_fm_corr_item *items, vio_fm_result *results);

/* One slot's list as arrays (the layout of the golden files): track i has observations pts[off[i] .. off[i + 1]).  _set replaces the
 * list; it refuses (VIO_ERR_BAD_ARG, nothing written) more than VIO_FM_MAX_TRACKS rows, a track with fewer than 1 or more than
 * VIO_FM_MAX_OBS observations, start < 0, start + n_obs - 1 > 10, a duplicate id, and a non-finite point or depth.  _get
 * needs room for the slot's n_tracks rows and cap_pts observations.  Both wait. */
vio_status vio_fm_tracks_set(vio_fm *h, int32_t slot, int32_t n, const int64_t *ids, const int32_t *start, const double *depth,
                             const int32_t *flag, const int64_t *off, const double *pts);
vio_status vio_fm_tracks_get(vio_fm *h, int32_t slot, int32_t cap, int64_t cap_pts, int32_t *n, int64_t *ids, int32_t *start,
                             double *depth, int32_t *flag, int64_t *off, double *pts);

/* ms of the last batched call that launched: host checks, packing and upload (host clock, the upload by HIP events), the kernel
 * (HIP events), the read-back (HIP events), the whole call (host clock). */
vio_status vio_fm_timing(const vio_fm *h, double *out4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
