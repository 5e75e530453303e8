// vio_reject_math.h — the per-point arithmetic of libvio_reject_hip (include/vio_reject.h): the PINHOLE camera's constants, the lift
// (PinholeCamera::liftProjective with ::distortion, VM/src/camera_models/camera_models/PinholeCamera.cc:461-521 and :657-673), the
// virtual pixel of rejectWithF, the normalised point of undistortedPoints and the velocity.  Device code of csrc/vio_reject.hip;
// plain C++ otherwise (the host side of vio_reject.hip uses rej_camera too), so that tests/test_reject_host_mirror.py can compile it for
// the host and hold it to tests/reject_reference.py bit for bit.  Every product and sum must round on its own: the including source
// sets `#pragma clang fp contract(off)` first, a host build passes -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/vio_reject.h"

#if defined(__HIPCC__)
#define REJ_FN __host__ __device__ __forceinline__
#else
#define REJ_FN inline
#endif

// what the lift reads of a camera: m_inv_K11, m_inv_K13, m_inv_K22, m_inv_K23 (PinholeCamera.cc:79-82), the distortion, m_noDistortion
struct RejCam {
    double ik11, ik13, ik22, ik23;
    double k1, k2, p1, p2;
    int32_t no_distortion, pad;
};

REJ_FN RejCam rej_camera(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2) {
    RejCam c;
    c.ik11 = 1.0 / fx; c.ik13 = -cx / fx;
    c.ik22 = 1.0 / fy; c.ik23 = -cy / fy;
    c.k1 = k1; c.k2 = k2; c.p1 = p1; c.p2 = p2;
    c.no_distortion = (k1 == 0.0) && (k2 == 0.0) && (p1 == 0.0) && (p2 == 0.0);
    c.pad = 0;
    return c;
}

// PinholeCamera::distortion
REJ_FN void rej_distortion(const RejCam &c, double x, double y, double &dx, double &dy) {
    const double mx2 = x * x, my2 = y * y, mxy = x * y;
    const double rho2 = mx2 + my2;
    const double rad = c.k1 * rho2 + c.k2 * rho2 * rho2;
    dx = x * rad + 2.0 * c.p1 * mxy + c.p2 * (rho2 + 2.0 * mx2);
    dy = y * rad + 2.0 * c.p2 * mxy + c.p1 * (rho2 + 2.0 * my2);
}

// PinholeCamera::liftProjective: pixel (u, v) -> the ray (x, y, 1)
REJ_FN void rej_lift(const RejCam &c, double u, double v, double &x, double &y) {
    const double mx_d = c.ik11 * u + c.ik13, my_d = c.ik22 * v + c.ik23;
    x = mx_d; y = my_d;
    if (c.no_distortion) return;
    double dx, dy;
    rej_distortion(c, mx_d, my_d, dx, dy);
    x = mx_d - dx; y = my_d - dy;
    for (int i = 1; i < VIO_REJECT_LIFT_EVALUATIONS; ++i) {
        rej_distortion(c, x, y, dx, dy);
        x = mx_d - dx; y = my_d - dy;
    }
}

// rejectWithF's virtual pixel of a lifted coordinate (feature_tracker.cpp:180-182): FOCAL_LENGTH * x / z + COL / 2.0 with z = 1,
// stored as cv::Point2f; returned as the double the fit reads
REJ_FN double rej_virtual(double focal, double x, double half) { return (double)(float)(focal * x / 1.0 + half); }

// undistortedPoints' normalised coordinate (feature_tracker.cpp:268): x / z, stored as cv::Point2f
REJ_FN float rej_unpoint(double x) { return (float)(x / 1.0); }

// the velocity of a matched point (feature_tracker.cpp:285-287), the difference in double
REJ_FN float rej_velocity(float un, float prev_un, double dt) { return (float)(((double)un - (double)prev_un) / dt); }
