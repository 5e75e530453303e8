// vio_camera_math.h — the per-point arithmetic of libvio_camera_hip (include/vio_camera.h): the device form of a camera slot and
// liftProjective of the reference's four camera models (VM/src/camera_models/camera_models/{PinholeCamera,CataCamera,ScaramuzzaCamera,
// EquidistantCamera}.cc), in the reference's operation order, with the virtual pixel of rejectWithF and the normalised point of
// undistortedPoints over a ray whose z is not 1.  Device code of csrc/vio_camera.hip; plain C++ otherwise, so that
// tests/test_camera_host_mirror.py can compile it for the host and hold it to tests/camera_reference.py.  Every product and sum must
// round on its own: the including source sets `#pragma clang fp contract(off)` first, a host build passes -ffp-contract=off.  The
// fma() calls of the KANNALA_BRANDT root solve are explicit and are fused on both sides.  No function of a math library is called
// but sqrt, floor and fma, which are exact or correctly rounded everywhere: sin, cos and atan2 are this header's own.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/vio_camera.h"
#include "vio_reject_math.h"

#if defined(__HIPCC__)
#define CAM_UNROLLED _Pragma("unroll")
#define CAM_ROLLED _Pragma("unroll 1")
#else
#define CAM_UNROLLED
#define CAM_ROLLED
#endif

// A camera slot as the kernels read it.  c[] by model:
//   PINHOLE          ik11 ik13 ik22 ik23 k1 k2 p1 p2                   (RejCam's fields: the lift is rej_lift)
//   MEI              ik11 ik13 ik22 ik23 k1 k2 p1 p2 xi                (m_inv_K* of CataCamera.cc:320-323)
//   SCARAMUZZA       inv_scale ac ad ae cx cy poly0 .. poly4           (m_inv_scale of ScaramuzzaCamera.cc:200)
//   KANNALA_BRANDT   ik11 ik13 ik22 ik23 k2 k3 k4 k5 theta_max r_max   (r_max = r(theta_max), cam_kb_r)
struct CamDev {
    int32_t model, set, npow, no_distortion;
    double half_w, half_h;
    double c[VIO_CAMERA_MAX_PARAMS];
};

// the ray of one pixel; theta, phi and clamped are KANNALA_BRANDT's (0 otherwise)
struct CamRay {
    double x, y, z;
    double theta, phi;
    int32_t clamped;
};

// EquidistantCamera::backprojectSymmetric's npow (EquidistantCamera.cc:731-747): 9 less 2 for every zero coefficient — each one, not
// only the trailing ones, as the reference has it
REJ_FN int cam_kb_npow(double k2, double k3, double k4, double k5) {
    int npow = 9;
    if (k5 == 0.0) npow -= 2;
    if (k4 == 0.0) npow -= 2;
    if (k3 == 0.0) npow -= 2;
    if (k2 == 0.0) npow -= 2;
    return npow;
}

// r(theta) = theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9 and r'(theta), Horner in theta^2
REJ_FN double cam_kb_r(const double *k, double th) {
    const double t = th * th;
    return th * (1.0 + t * (k[0] + t * (k[1] + t * (k[2] + t * k[3]))));
}
REJ_FN double cam_kb_dr(const double *k, double th) {
    const double t = th * th;
    return 1.0 + t * (3.0 * k[0] + t * (5.0 * k[1] + t * (7.0 * k[2] + t * (9.0 * k[3]))));
}

// f(theta) = r(theta) - rho by the compensated Horner scheme on the degree-9 polynomial in theta (error-free products by fma,
// error-free sums by TwoSum): as good as Horner in twice the precision, so the residual near the root keeps its sign and size
REJ_FN double cam_kb_f(const double *k, double rho, double th) {
    const double a[10] = {-rho, 1.0, 0.0, k[0], 0.0, k[1], 0.0, k[2], 0.0, k[3]};
    double s = a[9], c = 0.0;
CAM_UNROLLED
    for (int i = 8; i >= 0; --i) {
        const double p = s * th;
        const double pe = fma(s, th, -p);
        const double sn = p + a[i];
        const double bb = sn - p;
        const double se = (p - (sn - bb)) + (a[i] - bb);
        c = c * th + (pe + se);
        s = sn;
    }
    return s + c;
}

// The root of f in [0, theta_max], which vio_camera_set has checked to be the only one there (r' > 0 on its grid).  Fixed work:
// VIO_CAMERA_KB_BISECTIONS halvings of [0, theta_max], then VIO_CAMERA_KB_NEWTON Newton steps kept inside the bracket, the bracket shrunk
// by the sign of f at every step.  A step that leaves the bracket lands on the bound it crossed (a root at the bound itself, rho = 0
// above all, is met exactly that way); a second one in a row is replaced by the midpoint, which keeps the bisection's guarantee.
REJ_FN double cam_kb_solve(const double *k, double theta_max, double rho) {
    double lo = 0.0, hi = theta_max;
CAM_ROLLED
    for (int i = 0; i < VIO_CAMERA_KB_BISECTIONS; ++i) {
        const double mid = 0.5 * (lo + hi);
        if (cam_kb_f(k, rho, mid) <= 0.0) lo = mid; else hi = mid;
    }
    double th = 0.5 * (lo + hi);
    bool was_out = false;
CAM_ROLLED
    for (int i = 0; i < VIO_CAMERA_KB_NEWTON; ++i) {
        const double f = cam_kb_f(k, rho, th);
        if (f <= 0.0) lo = th; else hi = th;
        double nx = th - f / cam_kb_dr(k, th);
        const bool out = !(nx >= lo && nx <= hi);
        if (out) nx = was_out ? 0.5 * (lo + hi) : (nx > hi ? hi : lo);
        was_out = out;
        th = nx;
    }
    return th;
}

// sin, cos and atan2 of the KANNALA_BRANDT ray, in + - * / and floor alone, so that the device, the host build and the restatement
// have one result in every bit whatever math library each of them links: the kernels and coefficients are those of the freely
// distributable fdlibm (Sun Microsystems, 1993: k_sin.c, k_cos.c, s_atan.c, e_atan2.c): sin and cos below one ulp, atan2 (with its y / x) below two.  The reduction is
// its two-step Cody-Waite subtraction of n pi/2 (pi/2 to 118 bits; n pio2_1 is exact while |n| < 2^20): arguments beyond 1e6 in
// magnitude, which no angle of a camera reaches, and arguments that are not finite give NaN.
REJ_FN double cam_ksin(double x, double y) {                 // sin(x + y), |x| <= pi/4, y the tail of x
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x, v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
REJ_FN double cam_kcos(double x, double y) {                 // cos(x + y), |x| <= pi/4
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x, w = z * z;
    const double r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6));
    const double hz = 0.5 * z, t = 1.0 - hz;
    return t + (((1.0 - t) - hz) + (z * r - x * y));
}
// x = n pi/2 + (y0 + y1), |y0| <= pi/4 (a little more at a tie); returns n mod 4, -1 if x is out of range
REJ_FN int cam_rem_pio2(double x, double &y0, double &y1) {
    const double INVPIO2 = 6.36619772367581382433e-01, PIO2_1 = 1.57079632673412561417e+00, PIO2_2 = 6.07710050630396597660e-11,
                 PIO2_2T = 2.02226624879595063154e-21;
    y0 = x; y1 = 0.0;
    if (!(x >= -1e6 && x <= 1e6)) return -1;
    const double fn = floor(x * INVPIO2 + 0.5);
    const double t = x - fn * PIO2_1;
    double w = fn * PIO2_2;
    const double r = t - w;
    w = fn * PIO2_2T - ((t - r) - w);
    y0 = r - w;
    y1 = (r - y0) - w;
    return (int)((long long)fn & 3);
}
REJ_FN double cam_sin(double x) {
    double y0, y1;
    const int q = cam_rem_pio2(x, y0, y1);
    if (q < 0) return NAN;
    const double s = cam_ksin(y0, y1), c = cam_kcos(y0, y1);
    return q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
}
REJ_FN double cam_cos(double x) {
    double y0, y1;
    const int q = cam_rem_pio2(x, y0, y1);
    if (q < 0) return NAN;
    const double s = cam_ksin(y0, y1), c = cam_kcos(y0, y1);
    return q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}
REJ_FN double cam_atan_pos(double x) {                       // atan(x), x >= 0 (or NaN)
    const double T0 = 3.33333333333329318027e-01, T1 = -1.99999999998764832476e-01, T2 = 1.42857142725034663711e-01,
                 T3 = -1.11111104054623557880e-01, T4 = 9.09088713343650656196e-02, T5 = -7.69187620504482999495e-02,
                 T6 = 6.66107313738753120669e-02, T7 = -5.83357013379057348645e-02, T8 = 4.97687799461593236017e-02,
                 T9 = -3.65315727442169155270e-02, T10 = 1.62858201153657823623e-02;
    double hi = 0.0, lo = 0.0, t = x;
    if (x >= 2.4375) { hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17; t = -1.0 / x; }
    else if (x >= 1.1875) { hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17; t = (x - 1.5) / (1.0 + 1.5 * x); }
    else if (x >= 0.6875) { hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17; t = (x - 1.0) / (x + 1.0); }
    else if (x >= 0.4375) { hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17; t = (2.0 * x - 1.0) / (2.0 + x); }
    const double z = t * t, w = z * z;
    const double s1 = z * (T0 + w * (T2 + w * (T4 + w * (T6 + w * (T8 + w * T10)))));
    const double s2 = w * (T1 + w * (T3 + w * (T5 + w * (T7 + w * T9))));
    if (!(x >= 0.4375)) return t - t * (s1 + s2);
    return hi - ((t * (s1 + s2) - lo) - t);
}
REJ_FN double cam_atan2(double y, double x) {
    const double PI = 3.1415926535897931160e+00, PI_LO = 1.2246467991473531772e-16, PI_O_2 = 1.5707963267948965580e+00;
    if (y == 0.0) return x < 0.0 ? PI : 0.0 * x;             // (0 * x: NaN stays NaN)
    if (x == 0.0) return y < 0.0 ? -PI_O_2 : PI_O_2;
    const double q = y / x;
    const double z = cam_atan_pos(q < 0.0 ? -q : q);
    if (x > 0.0) return y < 0.0 ? -z : z;
    return y < 0.0 ? (z - PI_LO) - PI : PI - (z - PI_LO);
}

// CataCamera::liftProjective (CataCamera.cc:556-626): the pinhole's recursive distortion model on gamma1, gamma2, u0, v0 (the
// distortion of :766-781 is PinholeCamera's, operation for operation), then the mirror
REJ_FN void cam_lift_mei(const CamDev &C, double u, double v, CamRay &r) {
    RejCam p;
    p.ik11 = C.c[0]; p.ik13 = C.c[1]; p.ik22 = C.c[2]; p.ik23 = C.c[3];
    p.k1 = C.c[4]; p.k2 = C.c[5]; p.p1 = C.c[6]; p.p2 = C.c[7];
    p.no_distortion = C.no_distortion; p.pad = 0;
    double mx, my;
    rej_lift(p, u, v, mx, my);
    const double xi = C.c[8];
    r.x = mx; r.y = my;
    if (xi == 1.0) {
        r.z = (1.0 - mx * mx - my * my) / 2.0;
    } else {
        const double rho2 = mx * mx + my * my;
        r.z = 1.0 - xi * (rho2 + 1.0) / (xi + sqrt(1.0 + (1.0 - xi * xi) * rho2));
    }
}

// OCAMCamera::liftProjective (ScaramuzzaCamera.cc:599-621).  The ray's x and y are xc, the pixel relative to the centre, not the
// affine-corrected xc_a: that is what the reference returns, and it is kept.
REJ_FN void cam_lift_scaramuzza(const CamDev &C, double u, double v, CamRay &r) {
    const double xc0 = u - C.c[4], xc1 = v - C.c[5];
    const double a0 = C.c[0] * (xc0 - C.c[2] * xc1);
    const double a1 = C.c[0] * (-C.c[3] * xc0 + C.c[1] * xc1);
    const double phi = sqrt(a0 * a0 + a1 * a1);
    double phi_i = 1.0, z = 0.0;
CAM_UNROLLED
    for (int i = 0; i < 5; ++i) {
        z += phi_i * C.c[6 + i];
        phi_i *= phi;
    }
    r.x = xc0; r.y = xc1; r.z = -z;
}

// EquidistantCamera::liftProjective (EquidistantCamera.cc:428-442) over backprojectSymmetric (:716-818) with the root solve above
REJ_FN void cam_lift_kb(const CamDev &C, double u, double v, CamRay &r) {
    const double px = C.c[0] * u + C.c[1], py = C.c[2] * v + C.c[3];
    const double rho = sqrt(px * px + py * py);
    const double phi = rho < 1e-10 ? 0.0 : cam_atan2(py, px);
    const double k[4] = {C.c[4], C.c[5], C.c[6], C.c[7]};
    double theta;
    if (C.npow == 1) {
        theta = rho;
    } else if (rho > C.c[9]) {
        theta = C.c[8];
        r.clamped = 1;
    } else {
        theta = cam_kb_solve(k, C.c[8], rho);
    }
    const double st = cam_sin(theta);
    r.x = st * cam_cos(phi); r.y = st * cam_sin(phi); r.z = cam_cos(theta);
    r.theta = theta; r.phi = phi;
}

REJ_FN void cam_lift(const CamDev &C, double u, double v, CamRay &r) {
    r.theta = 0.0; r.phi = 0.0; r.clamped = 0;
    if (C.model == VIO_CAMERA_MODEL_PINHOLE) {
        RejCam p;
        p.ik11 = C.c[0]; p.ik13 = C.c[1]; p.ik22 = C.c[2]; p.ik23 = C.c[3];
        p.k1 = C.c[4]; p.k2 = C.c[5]; p.p1 = C.c[6]; p.p2 = C.c[7];
        p.no_distortion = C.no_distortion; p.pad = 0;
        rej_lift(p, u, v, r.x, r.y);
        r.z = 1.0;
    } else if (C.model == VIO_CAMERA_MODEL_MEI) {
        cam_lift_mei(C, u, v, r);
    } else if (C.model == VIO_CAMERA_MODEL_SCARAMUZZA) {
        cam_lift_scaramuzza(C, u, v, r);
    } else {
        cam_lift_kb(C, u, v, r);
    }
}

// rejectWithF's virtual pixel (feature_tracker.cpp:180-187): FOCAL_LENGTH * P0 / P2 + COL / 2.0 in that order, stored as cv::Point2f
REJ_FN double cam_virtual(double focal, double p, double z, double half) { return (double)(float)(focal * p / z + half); }

// undistortedPoints' normalised coordinate (feature_tracker.cpp:268): P0 / P2, stored as cv::Point2f
REJ_FN float cam_unpoint(double p, double z) { return (float)(p / z); }

// a lift the tracker cannot use: P0 / P2 or P1 / P2 is not finite (P2 == 0 on a fisheye, or a pixel that was not finite)
REJ_FN int cam_ray_bad(const CamRay &r) {
    const double qx = r.x / r.z, qy = r.y / r.z;
    return !(qx - qx == 0.0 && qy - qy == 0.0);              // (x - x is 0 exactly when x is finite)
}

// the device form of a checked vio_camera_model
inline CamDev cam_device_form(const vio_camera_model &m) {
    CamDev C;
    for (double &x : C.c) x = 0.0;
    C.model = m.model; C.set = 1; C.npow = 0; C.no_distortion = 0;
    C.half_w = m.width / 2.0; C.half_h = m.height / 2.0;
    const double *p = m.params;
    if (m.model == VIO_CAMERA_MODEL_PINHOLE) {
        const RejCam r = rej_camera(p[4], p[5], p[6], p[7], p[0], p[1], p[2], p[3]);
        C.c[0] = r.ik11; C.c[1] = r.ik13; C.c[2] = r.ik22; C.c[3] = r.ik23;
        C.c[4] = r.k1; C.c[5] = r.k2; C.c[6] = r.p1; C.c[7] = r.p2;
        C.no_distortion = r.no_distortion;
    } else if (m.model == VIO_CAMERA_MODEL_MEI) {
        const RejCam r = rej_camera(p[5], p[6], p[7], p[8], p[1], p[2], p[3], p[4]);
        C.c[0] = r.ik11; C.c[1] = r.ik13; C.c[2] = r.ik22; C.c[3] = r.ik23;
        C.c[4] = r.k1; C.c[5] = r.k2; C.c[6] = r.p1; C.c[7] = r.p2;
        C.c[8] = p[0];
        C.no_distortion = r.no_distortion;
    } else if (m.model == VIO_CAMERA_MODEL_SCARAMUZZA) {
        C.c[0] = 1.0 / (p[5] - p[6] * p[7]);
        C.c[1] = p[5]; C.c[2] = p[6]; C.c[3] = p[7]; C.c[4] = p[8]; C.c[5] = p[9];
        for (int i = 0; i < 5; ++i) C.c[6 + i] = p[i];
    } else {
        const RejCam r = rej_camera(p[4], p[5], p[6], p[7], 0.0, 0.0, 0.0, 0.0);
        C.c[0] = r.ik11; C.c[1] = r.ik13; C.c[2] = r.ik22; C.c[3] = r.ik23;
        for (int i = 0; i < 4; ++i) C.c[4 + i] = p[i];
        C.c[8] = p[8] == 0.0 ? VIO_CAMERA_KB_DEFAULT_THETA_MAX : p[8];
        C.c[9] = cam_kb_r(C.c + 4, C.c[8]);
        C.npow = cam_kb_npow(p[0], p[1], p[2], p[3]);
    }
    return C;
}

// r' > 0 at the VIO_CAMERA_KB_GRID + 1 grid points of [0, theta_max]
inline bool cam_kb_monotone(const double *k, double theta_max) {
    for (int i = 0; i <= VIO_CAMERA_KB_GRID; ++i)
        if (!(cam_kb_dr(k, theta_max * i / VIO_CAMERA_KB_GRID) > 0.0)) return false;
    return true;
}
