/*
 * vio_aif.h — all_image_frame and tmp_pre_integration of many streams on the GPU (companion library libvio_aif_hip.so).
 *
 * The reference's Estimator (vins-mono/src/estimator.cpp) keeps `all_image_frame`, the map of every image since the oldest window
 * frame, each with its points, its R / T / is_key_frame and its own pre_integration, and the open `tmp_pre_integration` the next
 * image will take.  Here a handle keeps up to VIO_AIF_MAX_SLOTS such maps resident on the device, one per stream ("slot"), and every
 * method runs for `count` slots in one call with one wait:
 *   vio_aif_imu_batch        processIMU's part (:107-112, :122, :137-138) for a run of samples per slot   (k_aif_imu, one wavefront per slot)
 *   vio_aif_image_batch      processImage's part (:156-159): insert the frame, hand it the open interval    (k_aif_image, one workgroup per slot)
 *   vio_aif_slide_batch      slideWindow's erase (:1186-1199)                                             (k_aif_slide, one workgroup per slot)
 *   vio_aif_propagate_batch  repropagate of every frame's interval at given biases (initial_aligment.cpp:31-35)   (k_imu_propagate)
 *   vio_aif_structure_batch  initialStructure's frame work (:243-270, :308-374): records, excitation, key walk, PnP, R / T
 *                                                              (k_aif_bias, k_imu_propagate, k_aif_join, k_pnp_frames, k_aif_finish)
 *   vio_aif_reset            clearState's part (:46-103) for one slot
 *   vio_aif_frames_get       download of one slot, for tests and debugging
 * This library is formally unpinned: the reference's Estimator is not compiled by the oracle, so the calls are restated from
 * estimator.cpp, and tests/aif_reference.py is the pin.  DESIGN.md section 31 has the layout, the kernels and what is measured.
 *
 * A slot holds, in time order, up to VIO_AIF_MAX_FRAMES frames.  Frame j has its header t, its points (feature id, x, y) in
 * ascending id order (the iteration order of the reference's std::map<int, ...>), R, T, is_key, and interval j: the constructor
 * arguments (acc_0, gyr_0, ba, bg) of its pre_integration and that one's samples (dt, acc, gyr), the samples between frame j - 1 and
 * frame j.  Interval n_frames is the open tmp_pre_integration.  exists[j] says whether interval j is an IntegrationBase at all: the
 * first image after a reset takes a null pointer (:157 with :92), and samples that arrive before it are dropped (:118).  The points
 * of all frames lie in one pool of VIO_AIF_MAX_POINTS per slot, the samples of all intervals in one pool of VIO_AIF_MAX_SAMPLES per
 * slot, both contiguous in frame order.  An IntegrationBase is kept as its constructor arguments and its samples;
 * vio_aif_propagate_batch recomputes records from them with the kernel of libvio_imu_hip (the same text, csrc/vio_imu_body.inc).
 *
 * Orders (csrc/vio_aif_math.h is their one text):
 *   rank of a point      the number of ids of the item smaller than its id (ids are distinct), so the stored order is ascending id
 *   erase                k = the one index with t[k] == t_0 (headers are strictly increasing); frames and intervals 0 .. k leave, frame
 *                        and interval j + k + 1 become j, the open interval included; the pools close up from the front
 * The only floating-point sums are k_imu_propagate's, whose orders vio_imu.h writes down, k_pnp_frames', which vio_pnp.h writes down,
 * and those of vio_aif_structure_batch, written down at its declaration.
 *
 * Rules:
 *   - argument errors write nothing and launch nothing for the whole call (VIO_ERR_BAD_ARG, vio_aif_last_error names the item): count
 *     outside [0, VIO_AIF_MAX_SLOTS], a NULL array, a slot outside [0, VIO_AIF_MAX_SLOTS) or listed twice, n < 0 or above its limit,
 *     a non-finite sample, header, point or bias, a duplicate feature id, and a header not greater than the slot's last one (the map
 *     would ignore such an insert; the library does not guess.  The handle knows every slot's frame count and last header from the
 *     results of its own calls);
 *   - rules only the device checks leave that slot exactly as it was, give the slot's result a VIO_AIF_STATUS_* and do not touch the
 *     other slots of the call (the call returns VIO_OK).  Every kernel makes that check first and the same way in all its threads;
 *   - repeated calls are bitwise identical, and a slot's result depends neither on the batch nor on the slot index (no atomics);
 *   - the calling thread's current HIP device is restored; one handle is used by one caller thread at a time.
 */
#ifndef VIO_AIF_H
#define VIO_AIF_H

#include "vio_backend.h"
#include "vio_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define VIO_AIF_VERSION 1
#define VIO_AIF_MAX_SLOTS 256
#define VIO_AIF_MAX_FRAMES 32                       /* = VIO_INIT_MAX_FRAMES = VIO_PNP_MAX_FRAMES */
#define VIO_AIF_MAX_FRAME_POINTS 1024               /* points of one frame (VIO_FM_MAX_POINTS) */
#define VIO_AIF_MAX_POINTS 8192                     /* points a slot can hold over all its frames */
#define VIO_AIF_MAX_SAMPLES 4096                    /* raw samples a slot can hold over all its intervals (VIO_EST_MAX_SAMPLES) */
#define VIO_AIF_OFFS 34                             /* offsets of a slot: 32 frames' intervals, the open one, and the end */

/* A slot's status in a result: a rule only the device checks; the slot is as it was. */
#define VIO_AIF_STATUS_OK 0
#define VIO_AIF_STATUS_POOL_FULL 1                  /* the samples or the points would not fit into the slot's pool */
#define VIO_AIF_STATUS_FRAMES_FULL 2                /* the slot holds VIO_AIF_MAX_FRAMES frames already */
#define VIO_AIF_STATUS_NO_FRAME 3                   /* slide: t_0 is not a stored header (the reference dereferences end() here) */
#define VIO_AIF_STATUS_WALK 4                       /* structure: the key walk ran past n_key, or a header of the item is in no frame */

#define VIO_AIF_MAX_KEY 32                          /* keyframes of a structure item */
#define VIO_AIF_MAX_TRACKS 4096                     /* tracks of a structure item (VIO_SFM_MAX_TRACKS) */

typedef struct vio_aif vio_aif;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own.  Every slot starts empty, with
 * acc_0 = gyr_0 = 0. */
vio_status vio_aif_create(int32_t device, void *stream, vio_aif **out);
void vio_aif_destroy(vio_aif *h);
const char *vio_aif_last_error(const vio_aif *h);          /* valid until the next call on h */
int32_t vio_aif_version(void);

/* The IMU noise of the pre-integrations and the PnP's min_points (of vio_aif_structure_batch).  Default: noise (0.2687, 0.2121,
 * 7.07e-6, 7.07e-7), the project's synthetic defaults; min_points VIO_PNP_DEFAULT_MIN_POINTS.  Everything finite. */
typedef struct vio_aif_config {
    double noise[4];                /* acc_n, gyr_n, acc_w, gyr_w, as vio_imu_noise */
    int32_t min_points;             /* in [3, VIO_PNP_MAX_POINTS], as vio_pnp_config's */
    int32_t reserved;
} vio_aif_config;
vio_status vio_aif_set_config(vio_aif *h, const vio_aif_config *cfg);

/* clearState of one slot: the map and tmp_pre_integration go, first_imu = 0; acc_0 / gyr_0 stay, as clearState leaves them.  Waits. */
vio_status vio_aif_reset(vio_aif *h, int32_t slot);

/* What every batched call returns per item. */
typedef struct vio_aif_result {
    int32_t status;                 /* VIO_AIF_STATUS_* */
    int32_t n_frames;               /* the slot's frames after the call */
    int32_t n_points;               /* ... its points over all frames */
    int32_t n_samples;              /* ... its samples over all intervals, the open one included */
    int32_t erased_frames;          /* slide: frames that left */
    int32_t erased_samples;         /* slide: samples that left */
    int32_t records;                /* propagate: records written, n_frames - 1 (0 for an empty slot) */
    int32_t reserved;
} vio_aif_result;

/* processIMU for samples 0 .. n - 1 in order: acc_0 / gyr_0 follow always; the samples go into the open interval only once the slot
 * has had an image since its reset (exists[n_frames], the reference's frame_count != 0).  n = 0 does nothing. */
typedef struct vio_aif_imu_item {
    int32_t slot;
    int32_t n;                      /* in [0, VIO_AIF_MAX_SAMPLES] */
    const double *dt;               /* [n] */
    const double *acc;              /* [n][3] linear_acceleration */
    const double *gyr;              /* [n][3] angular_velocity */
} vio_aif_imu_item;
vio_status vio_aif_imu_batch(vio_aif *h, int32_t count, const vio_aif_imu_item *items, vio_aif_result *results);

/* processImage (:156-159): a new frame with header t and the n points, stored in ascending id; R = 0, T = 0, is_key = 0; it takes
 * the open interval, and the next one is opened with (acc_0, gyr_0, ba, bg). */
typedef struct vio_aif_image_item {
    int32_t slot;
    int32_t n;                      /* in [0, VIO_AIF_MAX_FRAME_POINTS] */
    double t;                       /* header: greater than the slot's last one */
    const int64_t *ids;             /* [n] feature ids, distinct, any order */
    const double *pts;              /* [n][2] x, y */
    double ba[3];                   /* Bas[frame_count] */
    double bg[3];                   /* Bgs[frame_count] */
} vio_aif_image_item;
vio_status vio_aif_image_batch(vio_aif *h, int32_t count, const vio_aif_image_item *items, vio_aif_result *results);

/* slideWindow's erase (:1186-1199): every frame with header <= t_0 leaves, with its points and its interval's samples.  t_0 must be
 * a stored header, else VIO_AIF_STATUS_NO_FRAME.  (The reference deletes the erased frames' pre_integrations, which are all
 * that leave; the new first frame keeps its own.) */
typedef struct vio_aif_slide_item {
    int32_t slot;
    int32_t reserved;
    double t_0;
} vio_aif_slide_item;
vio_status vio_aif_slide_batch(vio_aif *h, int32_t count, const vio_aif_slide_item *items, vio_aif_result *results);

/* Every frame's interval from the resident samples at the given biases: pre[j - 1] is interval j, frame j - 1 to frame j, for
 * j = 1 .. n_frames - 1, computed from its constructor (acc_0, gyr_0) and samples as ImuHandle.load + propagate would, byte for byte.
 * An interval without samples gives the empty record of vio_imu.h.  pre needs room for VIO_AIF_MAX_FRAMES - 1 records or, if the
 * caller knows n_frames, n_frames - 1; result.records says how many were written. */
typedef struct vio_aif_propagate_item {
    int32_t slot;
    int32_t reserved;
    double ba[3];
    double bg[3];
    vio_preint *pre;                /* [n_frames - 1] */
} vio_aif_propagate_item;
vio_status vio_aif_propagate_batch(vio_aif *h, int32_t count, const vio_aif_propagate_item *items, vio_aif_result *results);

/* initialStructure's frame work (:243-270, :308-374) on the slot's frames, in one stream-ordered sequence on the device:
 *   1. the records of intervals 1 .. F - 1, each at its constructor biases (k_imu_propagate), byte for byte ImuHandle.load + propagate;
 *   2. the excitation check over them: sum_g from zero (the reference leaves it uninitialised), frames 1 .. F - 1 in time order,
 *      tmp_g = delta_v / sum_dt, aver_g = (sum_g * 1.0) / (F - 1), var += (x x + y y) + z z of tmp_g - aver_g, var = sqrt(var / (F - 1)).
 *      Returned with the flag var < 0.25; the reference's `return false` is commented out, so it never fails a window.  var is NaN
 *      (0 / 0, as the lines give) and the flag 0 where F <= 1 or an interval has no samples (its record's sum_dt is 0); which NaN, its
 *      sign and payload, is not specified: a host's 0 / 0 and the device's differ in the sign bit;
 *   3. the key walk as written, i from 0: a frame whose header equals headers[i] is a keyframe, R = Q[i].toRotationMatrix() ric^T
 *      (Eigen's, of the quaternion as given; (A_i0 ric_j0 + A_i1 ric_j1) + A_i2 ric_j2), T = T[i], i++; otherwise
 *      `if (header > headers[i]) i++`, once, and the guess is keyframe i.  A leading non-keyframe gets guess 0.  i reaching n_key where
 *      the lines read headers[i] or Q[i], or a header matched by no frame, is VIO_AIF_STATUS_WALK: nothing is solved or written;
 *   4. the PnP items, written on the device: every observation of a non-keyframe, in its stored (ascending id) order, looks its id up by
 *      bisection in the item's tracks sorted by id; a missing id or a track with state == 0 maps to one extra point row with valid = 0,
 *      which the PnP's own skip rule drops;
 *   5. k_pnp_frames, the text of libvio_pnp_hip (csrc/vio_pnp_body.inc), under this handle's min_points: include/vio_pnp.h is its
 *      contract, and Q, T, status, iterations, n_used and cost are byte for byte vio_pnp_frames_batch's on the same items;
 *   6. R = toRotationMatrix(Q_pnp) ric^T, T = T_pnp for the non-keyframes (:365-373); R, T, is_key go into the slot and to the caller.
 * A frame that fails leaves NaN in its R and T; the frames after it are still computed (as in vio_pnp.h).  A slot one of whose
 * frames is VIO_ERR_NOT_FINITE has NaN in every non-keyframe and pnp_status VIO_ERR_NOT_FINITE; the other slots are not touched and
 * the call returns VIO_OK.  An empty slot (F = 0) is VIO_AIF_STATUS_WALK, as the walk over no frames finds none of the n_key >= 1 headers:
 * n_frames 0, n_key 0, var NaN, and no out array of the item is written. */
typedef struct vio_aif_structure_item {
    int32_t slot;
    int32_t n_key;                  /* in [1, VIO_AIF_MAX_KEY] */
    int32_t n_tracks;               /* in [0, VIO_AIF_MAX_TRACKS] */
    int32_t reserved;
    const double *headers;          /* [n_key] the estimator's Headers[], finite */
    const double *Q;                /* [n_key][4] (w, x, y, z), the SfM's, as vio_sfm_result's Q; finite (else VIO_ERR_BAD_ARG) */
    const double *T;                /* [n_key][3], finite */
    const int64_t *track_ids;       /* [n_tracks] feature ids (vio_fm_tracks_get), any order, distinct */
    const double *points;           /* [n_tracks][3] (vio_sfm_construct_batch); not read where state is 0 */
    const uint8_t *state;           /* [n_tracks] */
    double ric[9];                  /* RIC[0], row-major, finite */
    double *R;                      /* out [n_frames][9]: what vio_init_item takes */
    double *T_out;                  /* out [n_frames][3] */
    uint8_t *is_key;                /* out [n_frames], as vio_init_item's */
    vio_preint *pre;                /* out [n_frames - 1] */
    vio_pnp_frame_info *frame_info; /* out [n_frames], or NULL; a keyframe's row is VIO_OK, 0, 0, cost 0 */
} vio_aif_structure_item;

typedef struct vio_aif_structure_result {
    int32_t status;                 /* VIO_AIF_STATUS_OK / VIO_AIF_STATUS_WALK */
    int32_t pnp_status;             /* VIO_OK, the first failing frame's VIO_PNP_FAIL_*, or VIO_ERR_NOT_FINITE */
    int32_t fail_frame;             /* the first failing frame, an index into the slot's frames, else -1 */
    int32_t n_frames;
    int32_t n_key;                  /* keyframes the walk found */
    int32_t low_excitation;         /* var < 0.25 */
    double var;
} vio_aif_structure_result;

/* The out arrays need room for the slot's n_frames (VIO_AIF_MAX_FRAMES always suffices). */
vio_status vio_aif_structure_batch(vio_aif *h, int32_t count, const vio_aif_structure_item *items, vio_aif_structure_result *results);

/* One slot without its pools.  Entries at and behind n_frames are unspecified, except interval n_frames, the open one. */
typedef struct vio_aif_slot {
    int32_t n_frames;               /* in [0, VIO_AIF_MAX_FRAMES] */
    int32_t first_imu;              /* 0 / 1 */
    int32_t n_points;
    int32_t reserved;
    int32_t exists[VIO_AIF_OFFS];   /* [j]: interval j is an IntegrationBase; [33] is 0 */
    int32_t is_key[VIO_AIF_MAX_FRAMES];
    int32_t pt_off[VIO_AIF_OFFS];   /* frame j has points [pt_off[j], pt_off[j + 1]); pt_off[0] = 0; [33] unused */
    int64_t samp_off[VIO_AIF_OFFS]; /* interval j has samples [samp_off[j], samp_off[j + 1]); samp_off[0] = 0 */
    double t[VIO_AIF_MAX_FRAMES];
    double R[VIO_AIF_MAX_FRAMES][9];
    double T[VIO_AIF_MAX_FRAMES][3];
    double first[VIO_AIF_OFFS][6];  /* acc_0 | gyr_0 interval j was constructed with */
    double bias[VIO_AIF_OFFS][6];   /* ba | bg interval j was constructed with */
    double acc_0[3];
    double gyr_0[3];
} vio_aif_slot;

/* Download of one slot.  ids / pts need room for cap_points >= n_points, dt / acc / gyr for cap_samples >= the slot's samples, else
 * VIO_ERR_BAD_ARG with *slot_out written (so the caller can size the arrays); an array may be NULL when its count is 0.  Waits. */
vio_status vio_aif_frames_get(vio_aif *h, int32_t slot, vio_aif_slot *slot_out, int64_t cap_points, int64_t *ids, double *pts,
                              int64_t cap_samples, double *dt, double *acc, double *gyr);

/* ms of the last batched call that launched: host checks, packing and upload (host clock); the kernels (HIP events); the read-back
 * (HIP events); the whole call (host clock). */
vio_status vio_aif_timing(const vio_aif *h, double *out4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
