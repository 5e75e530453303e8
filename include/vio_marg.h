/*
 * vio_marg.h — batched marginalisation of many windows on the GPU (companion library libvio_marg_hip.so).
 *
 * What vio_marginalize (include/vio_backend.h) computes for one context, for `count` independent windows in one call, from the
 * host arrays a frame loop already holds (MargOldFrame / MargNewFrame build a fresh Problem from para_*: estimator.cpp:693-901).
 * No context is needed.  Both halves run on the device: k_marg_build assembles every window's H_marg / b_marg (landmark Schur
 * complement, IMU edge 0, the old prior), k_marg_tail runs the dense tail of Problem::Marginalize (problem.cc:717-779) with one
 * workgroup per window and a parallel cyclic Jacobi eigen-solver.  DESIGN.md section 14 has the math and the layout.
 *
 * Window i's result is what vio_marginalize(kind) returns on a context given the same arrays through vio_set_window,
 * vio_set_landmarks, vio_set_observations, vio_set_imu (interval 0) and vio_set_prior, to rounding: the eigen-solver is another
 * algorithm than the host tail's QL, so eigenvector signs and the basis inside degenerate eigenspaces differ (J^T J, err's norm
 * and the consistency err = -jt_inv b are what agree).
 *
 * Rules:
 *   - inverse-depth windows only (the reference never marginalises XYZ landmarks);
 *   - a landmark block without an inverse gives that window H = 0 and b, err, jt_inv NaN, and window_status VIO_ERR_NOT_FINITE;
 *     the other windows are computed, and the call returns VIO_ERR_NOT_FINITE;
 *     any non-finite entry of H_marg or b_marg gives this outcome, whatever its source (a zero or non-finite inverse depth, a non-finite
 *     observation of an edge of the graph, a non-finite entry of b_prior or of the lower triangle of H_prior, which is the one read:
 *     H_prior is taken as symmetric); what lies outside the graph (landmarks hosted in other frames, landmarks without observations)
 *     is not read;
 *   - argument errors (bad kind, null array, index out of range, host == target, a landmark with two hosts) write nothing and
 *     launch nothing: VIO_ERR_BAD_ARG, vio_marg_last_error names the window.  count == 0 does nothing and returns VIO_OK;
 *   - repeated calls are bitwise identical, and a window's result does not depend on the batch it is in (no atomics, fixed
 *     summation orders);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_MARG_H
#define VIO_MARG_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_MARG_VERSION 1

typedef struct vio_marg vio_marg;

/* cfg: device, stream (NULL: the handle creates its own), loss, edge information and gravity are used; ext_fixed is not (the
 * reference's Marginalize adds the extrinsic unmasked, as vio_marginalize does). */
vio_status vio_marg_create(const vio_config *cfg, vio_marg **out);
vio_status vio_marg_set_config(vio_marg *h, const vio_config *cfg);   /* device and stream must stay those of vio_marg_create */
void vio_marg_destroy(vio_marg *h);
const char *vio_marg_last_error(const vio_marg *h);                   /* valid until the next call on h */
int32_t vio_marg_version(void);

typedef struct vio_marg_item {
    int32_t kind;                                   /* VIO_MARG_OLD / VIO_MARG_SECOND_NEW */
    const double *poses, *speed_bias, *ext;         /* 11 x 7, 11 x 9, 7: what vio_set_window takes */
    int64_t n;                                      /* landmarks */
    const double *inv_depth;                        /* n: what vio_set_landmarks takes */
    int64_t m;                                      /* observations */
    const int32_t *lm, *host, *target;              /* m each: what vio_set_observations takes */
    const double *pts_i, *pts_j;                    /* m x 2 each */
    const vio_preint *imu0;                         /* interval 0 -> 1, or NULL for no edge */
    const double *H_prior, *b_prior;                /* 156 x 156 and 156 (vio_get_prior's b after a solve), both NULL: no prior */
    double *H, *b, *err, *jt_inv;                   /* out: 156 x 156, 156, 156, 156 x 156 (vio_marginalize's four outputs) */
} vio_marg_item;

/* For VIO_MARG_SECOND_NEW only the prior is read (the graph of MargNewFrame has no edges); the other inputs may be NULL / 0. */
vio_status vio_marg_compute_batch(vio_marg *h, int32_t count, const vio_marg_item *items, vio_status *window_status);
vio_status vio_marg_compute(vio_marg *h, const vio_marg_item *item);  /* a batch of one */
/* Times of the last call that launched, ms: [0] host pack (wall clock) + the H2D copy (HIP events), [1] k_marg_build, [2] k_marg_tail (HIP events),
 * [3] the whole call (wall clock). */
vio_status vio_marg_timing(vio_marg *h, double *out4);
/* Rows of window i's reduced system that were live (the size of its eigen-problem) in the last call; i < that call's count. */
vio_status vio_marg_live_rows(vio_marg *h, int32_t i, int32_t *rows);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
