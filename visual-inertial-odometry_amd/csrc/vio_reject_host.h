// vio_reject_host.h — the host side of the rejection stage that needs no HIP call: the descriptor tables of the kernels in
// vio_reject_body.inc, the defaults, the camera and config checks and the settings of a RANSAC call.  libvio_reject_hip (vio_reject.hip,
// at file scope) and libvio_frame_hip (vio_frame.hip, in namespace kr) include it ahead of the body; so does
// tests/cpp/front_host_main.cpp, with a plain C++ compiler.  It includes nothing itself: the including file has included <cmath>,
// <cstdint>, ../../include/vio_reject.h, vio_host_base.h and vio_reject_math.h.
// libvio_camera_hip (vio_camera.hip) compiles the body against tables and a lift of its own: it defines REJ_CUSTOM_TABLES and supplies
// everything between the two marks below under the same names (vio_camera_host.h).
struct RejRes {
    int32_t status, hyp, n_inliers, pad;
    double F[9];
};

constexpr vio_reject_config REJ_DEFAULTS = {0u, VIO_REJECT_DEFAULT_HYPOTHESES, VIO_REJECT_DEFAULT_F_THRESHOLD, VIO_REJECT_DEFAULT_FOCAL_LENGTH};

inline vio_status rej_check_camera(ErrText &err, const char *fn, const vio_reject_camera *cam) {
    if (!cam) return fail(err, VIO_ERR_BAD_ARG, "%s: NULL camera", fn);
    if (cam->model != VIO_REJECT_MODEL_PINHOLE) return fail(err, VIO_ERR_BAD_ARG, "%s: model %d: only PINHOLE is built", fn, cam->model);
    const double v[8] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->k1, cam->k2, cam->p1, cam->p2};
    for (double x : v)
        if (!std::isfinite(x)) return fail(err, VIO_ERR_BAD_ARG, "%s: a parameter is not finite", fn);
    if (cam->fx == 0.0 || cam->fy == 0.0 || cam->width < 1 || cam->height < 1)
        return fail(err, VIO_ERR_BAD_ARG, "%s: fx, fy must not be 0, width and height at least 1", fn);
    return VIO_OK;
}

inline vio_status rej_check_config(ErrText &err, const char *fn, const vio_reject_config *c) {
    if (!c || c->ransac_hypotheses < 1 || c->ransac_hypotheses > VIO_REJECT_MAX_HYPOTHESES || !(c->f_threshold > 0.0) ||
        !std::isfinite(c->f_threshold) || !(c->focal_length > 0.0) || !std::isfinite(c->focal_length))
        return fail(err, VIO_ERR_BAD_ARG, "%s: ransac_hypotheses in [1, %d], f_threshold and focal_length finite and > 0", fn, VIO_REJECT_MAX_HYPOTHESES);
    return VIO_OK;
}

#ifndef REJ_CUSTOM_TABLES                                    // ---- from here ...
struct RejPair {
    int32_t n, active;
    uint32_t pair;
    int32_t finite;     // no point of the pair is NaN or infinite
    int64_t o_pts;      // staged floats: cur [n][2] | forw [n][2]
    int64_t o_corr;     // double scratch: corr [n][4]
    int64_t o_pt;       // the pair's first point in the flat per-point arrays (flags, mask)
};

struct RansacArgs {
    const RejPair *pairs;
    const float *pts;
    double *corr;
    int32_t *flag;      // [points of the call]: the winner's inliers
    uint8_t *mask;      // [points of the call]
    RejRes *res;
    RejCam cam;
    double focal, half_w, half_h, thr;
    uint32_t seed;
    int32_t hyps;
};

struct LiftItem {
    int32_t n, m, active, pad;
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
    double *lifted;     // [points][2] (bare lift)
    RejCam cam;
    int32_t bare, count;
};

// The customisation points of vio_reject_body.inc: the ray of one pixel of an item or a pair and what the two stages take from it.
// Here the ray is (x, y, 1), the camera is the call's, and a lift cannot fail on the device (the host has looked at every pixel).
#define REJ_RAY(r) double r##_x = 0.0, r##_y = 0.0
#define REJ_RAY_UNSET(r) double r##_x, r##_y
#define REJ_ITEM_LIFT(a, D, i, u, v, r) rej_lift((a).cam, u, v, r##_x, r##_y)
#define REJ_STORE_BARE(a, D, i, r) (a).lifted[2 * ((D).o_out + (i))] = r##_x; (a).lifted[2 * ((D).o_out + (i)) + 1] = r##_y
#define REJ_UN_X(r) rej_unpoint(r##_x)
#define REJ_UN_Y(r) rej_unpoint(r##_y)
#define REJ_PROLOGUE_BEGIN
#define REJ_PAIR_LIFT(a, P, u, v, r) rej_lift((a).cam, u, v, r##_x, r##_y)
#define REJ_VIRTUAL_X(a, P, r) rej_virtual((a).focal, r##_x, (a).half_w)
#define REJ_VIRTUAL_Y(a, P, r) rej_virtual((a).focal, r##_y, (a).half_h)
#define REJ_PROLOGUE_END(n, tid, mask, o)

// a checked camera as a handle keeps it: the caller's struct, and the form the kernels take
inline void rej_set_camera(const vio_reject_camera &in, vio_reject_camera &camera, RejCam &cam) {
    camera = in;
    camera.reserved = 0;
    cam = rej_camera(in.fx, in.fy, in.cx, in.cy, in.k1, in.k2, in.p1, in.p2);
}

// the settings of a RANSAC call; the addresses are the caller's to fill in
inline RansacArgs rej_ransac_args(const RejCam &cam, const vio_reject_camera &camera, const vio_reject_config &cfg) {
    RansacArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam = cam;
    a.focal = cfg.focal_length; a.half_w = camera.width / 2.0; a.half_h = camera.height / 2.0;
    a.thr = cfg.f_threshold * cfg.f_threshold;
    a.seed = cfg.seed; a.hyps = cfg.ransac_hypotheses;
    return a;
}
#endif                                                       // ---- ... to here
