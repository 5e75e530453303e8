// vio_camera_host.h — what libvio_camera_hip (vio_camera.hip) supplies in place of the guarded part of vio_reject_host.h, so that
// vio_reject_body.inc compiles against the four camera models with a camera per item: the descriptor tables under the same names with
// a slot in each, the customisation macros of the body, and the check of a camera.  It defines REJ_CUSTOM_TABLES and includes
// vio_reject_host.h for the rest (RejRes, the defaults, the config check).  The including file has included <cmath>, <cstdint>,
// ../../include/vio_camera.h, vio_host_base.h and vio_camera_math.h.  Plain C++ apart from the macros' use in the kernels.
#define REJ_CUSTOM_TABLES
#include "vio_reject_host.h"

struct RejPair {
    int32_t n, active;
    uint32_t pair;
    int32_t finite;     // no pixel of the pair is NaN or infinite
    int64_t o_pts;      // staged floats: cur [n][2] | forw [n][2]
    int64_t o_corr;     // double scratch: corr [n][4]
    int64_t o_pt;       // the pair's first point in the flat per-point arrays (flags, mask)
    int32_t slot, pad;
};

struct RansacArgs {
    const RejPair *pairs;
    const float *pts;
    double *corr;
    int32_t *flag;      // [points of the call]: the winner's inliers
    uint8_t *mask;      // [points of the call]
    RejRes *res;
    const CamDev *cams; // [VIO_CAMERA_MAX_SLOTS]
    double focal, thr;
    uint32_t seed;
    int32_t hyps;
};

struct LiftItem {
    int32_t n, m, active, slot;
    int64_t o_pts;      // staged floats: pts [n][2]
    int64_t o_prev;     // staged floats: prev_un_pts [m][2]
    int64_t o_ids;      // staged int64: ids [n] | prev_ids [m]
    int64_t o_out;      // the item's first point in the outputs
    double dt;
};

struct LiftArgs {
    const LiftItem *items;
    const float *pts;
    const long long *ids;
    float *un;          // [points][2] un_pts | [points][2] velocity behind them (undistort)
    float *vel;
    double *lifted;     // [points][3] rays | [points][2] angles behind them (bare lift)
    double *angles;
    uint8_t *flags;     // [points]: CAM_FLAG_BAD | CAM_FLAG_CLAMPED
    const CamDev *cams; // [VIO_CAMERA_MAX_SLOTS]
    int32_t bare, count;
};

constexpr int CAM_FLAG_BAD = 1, CAM_FLAG_CLAMPED = 2;

// The customisation points of vio_reject_body.inc.  The ray is a CamRay of the item's camera; the lift kernel leaves a flag byte per
// point (the host turns a bad point into the item's VIO_ERR_NOT_FINITE); the RANSAC's prologue gathers the bad lifts of its pair in
// s_i[3], which the kernel has not begun to use, and leaves the pair's result itself.  No LDS is added.
#define REJ_RAY(r) CamRay r = {}
#define REJ_RAY_UNSET(r) CamRay r
#define REJ_ITEM_LIFT(a, D, i, u, v, r)                                                                              \
    do {                                                                                                             \
        cam_lift((a).cams[(D).slot], u, v, r);                                                                       \
        (a).flags[(D).o_out + (i)] = (uint8_t)((cam_ray_bad(r) ? CAM_FLAG_BAD : 0) | (r.clamped ? CAM_FLAG_CLAMPED : 0)); \
    } while (0)
#define REJ_STORE_BARE(a, D, i, r)                                                                                   \
    do {                                                                                                             \
        const int64_t at_ = (D).o_out + (i);                                                                         \
        (a).lifted[3 * at_] = r.x; (a).lifted[3 * at_ + 1] = r.y; (a).lifted[3 * at_ + 2] = r.z;                     \
        (a).angles[2 * at_] = r.theta; (a).angles[2 * at_ + 1] = r.phi;                                              \
    } while (0)
#define REJ_UN_X(r) cam_unpoint(r.x, r.z)
#define REJ_UN_Y(r) cam_unpoint(r.y, r.z)
#define REJ_PROLOGUE_BEGIN                                                                                           \
    const CamDev rej_cam_ = a.cams[P.slot];                                                                          \
    int rej_bad_ = 0;                                                                                                \
    if (tid == 0) s_i[3] = 0;                                                                                        \
    __syncthreads()
#define REJ_PAIR_LIFT(a, P, u, v, r)                                                                                 \
    do {                                                                                                             \
        cam_lift(rej_cam_, u, v, r);                                                                                 \
        rej_bad_ |= cam_ray_bad(r);                                                                                  \
    } while (0)
#define REJ_VIRTUAL_X(a, P, r) cam_virtual((a).focal, r.x, r.z, rej_cam_.half_w)
#define REJ_VIRTUAL_Y(a, P, r) cam_virtual((a).focal, r.y, r.z, rej_cam_.half_h)
#define REJ_PROLOGUE_END(n, tid, mask, o)                                                                            \
    if (rej_bad_) atomicOr(&s_i[3], 1);                                                                              \
    __syncthreads();                                                                                                 \
    const int rej_any_bad_ = s_i[3];                                                                                 \
    __syncthreads();                                         /* (thread 0 sets s_i[3] again right behind this) */    \
    if (rej_any_bad_) {                                                                                              \
        for (int k = tid; k < n; k += NT) mask[k] = 0;                                                               \
        if (tid == 0) { o->status = VIO_ERR_NOT_FINITE; o->hyp = -1; o->n_inliers = 0; o->pad = 0; }                  \
        if (tid < 9) o->F[tid] = NAN;                                                                                \
        return;                                                                                                      \
    }

// a camera as vio_camera_set takes it
inline vio_status cam_check_model(ErrText &err, const vio_camera_model *m) {
    if (!m) return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: NULL camera");
    if (m->model < VIO_CAMERA_MODEL_PINHOLE || m->model > VIO_CAMERA_MODEL_SCARAMUZZA)
        return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: unknown model %d", m->model);
    if (m->width < 1 || m->height < 1) return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: width and height at least 1");
    const double *p = m->params;
    for (int i = 0; i < VIO_CAMERA_MAX_PARAMS; ++i)
        if (!std::isfinite(p[i])) return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: parameter %d is not finite", i);
    if (m->model == VIO_CAMERA_MODEL_PINHOLE && (p[4] == 0.0 || p[5] == 0.0)) return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: fx, fy must not be 0");
    if (m->model == VIO_CAMERA_MODEL_MEI && (p[5] == 0.0 || p[6] == 0.0)) return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: gamma1, gamma2 must not be 0");
    if (m->model == VIO_CAMERA_MODEL_SCARAMUZZA && !(std::isfinite(1.0 / (p[5] - p[6] * p[7]))))
        return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: ac - ad ae must not be 0");
    if (m->model == VIO_CAMERA_MODEL_KANNALA_BRANDT) {
        if (p[4] == 0.0 || p[5] == 0.0) return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: mu, mv must not be 0");
        const double tm = p[8] == 0.0 ? VIO_CAMERA_KB_DEFAULT_THETA_MAX : p[8];
        if (!(tm > 0.0 && tm <= VIO_CAMERA_KB_DEFAULT_THETA_MAX)) return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: theta_max must be in (0, pi]");
        if (!cam_kb_monotone(p, tm))
            return fail(err, VIO_ERR_BAD_ARG, "vio_camera_set: theta + k2 theta^3 + .. + k5 theta^9 does not increase over [0, %g]", tm);
    }
    return VIO_OK;
}
