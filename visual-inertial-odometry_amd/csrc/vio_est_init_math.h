// vio_est_init_math.h — the arithmetic of visualInitialAlign's hand-over and of the bias re-linearisation (include/vio_est_init.h,
// DESIGN.md section 33) that a host compiler can build too.  Device code of csrc/vio_est_init_body.inc; plain C++ otherwise, so that
// tests/cpp/est_init_math_main.cpp can run it on the host and tests/test_est_init_reference.py can hold it to
// tests/est_init_reference.py.  It adds to csrc/vio_est_math.h and shares its rules: no contraction, every product and sum as written.
#pragma once

#include "vio_est_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// One frame of the hand-over: pose = (p, q xyzw), sb = (V, ba, bg) as vio_init_align_batch wrote them.  Ps = p; q normalised as
// double2vector does; Rs = toRotationMatrix(q); Vs, Ba, Bg copied; lin = (0, 0, 0, bg): repropagate(Vector3d::Zero(), Bgs[i]).
EST_FN void est_init_frame(const double *pose, const double *sb, double *Rs, double *Ps, double *Vs, double *Ba, double *Bg, double *lin) {
    const double x = pose[3], y = pose[4], z = pose[5], w = pose[6];
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    const double q[4] = {x / n, y / n, z / n, w / n};
    est_quat_to_rot(q, Rs);
    for (int c = 0; c < 3; ++c) {
        Ps[c] = pose[c];
        Vs[c] = sb[c];
        Ba[c] = sb[3 + c];
        Bg[c] = sb[6 + c];
        lin[c] = 0.0;
        lin[3 + c] = sb[6 + c];
    }
}

// g = rot g (estimator.cpp:448) on the refined gravity of the SfM frame
EST_FN void est_init_gravity(const double *rot, const double *g, double *out) { est_apply(rot, g, out); }

// Has the bias of an interval's start frame moved past a threshold from the interval's linearisation biases?  Per axis, max-abs,
// strict: StreamDriver.relinearize_biases' rule.
EST_FN bool est_relin_moved(const double *Ba, const double *Bg, const double *lin, double ba_thresh, double bg_thresh) {
    double da = 0.0, dg = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double a = fabs(Ba[c] - lin[c]), g = fabs(Bg[c] - lin[3 + c]);
        if (a > da) da = a;
        if (g > dg) dg = g;
    }
    return da > ba_thresh || dg > bg_thresh;
}
