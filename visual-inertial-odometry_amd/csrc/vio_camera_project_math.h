// vio_camera_project_math.h — spaceToPlane of the reference's four camera models (include/vio_camera_project.h):
// the projection table's entry of a camera slot and the pixel of one point, in the reference's operation order
// (VM/src/camera_models/camera_models/{PinholeCamera.cc:531-553, CataCamera.cc:636-659, ScaramuzzaCamera.cc:632-653,
// EquidistantCamera.cc:451-461}).  Device code of k_camera_project (csrc/vio_camera_project_body.inc); plain C++ otherwise, so that
// tests/cpp/camera_project_main.cpp can compile it for the host and tests/test_camera_project_cpu.py can hold it to
// tests/camera_project_reference.py bit for bit.  vio_camera_math.h's rules: every product and sum rounds on its own (the including
// source sets `#pragma clang fp contract(off)` first, a host build passes -ffp-contract=off); no function of a math library is called
// but sqrt; atan2, sin and cos are vio_camera_math.h's.
#pragma once

#include "../../include/vio_camera_project.h"
#include "vio_camera_math.h"

// A camera slot as k_camera_project reads it: a table of its own beside CamDev, which holds the lift's inverse constants and does not
// grow.  p[] is params[] of vio_camera_model as vio_camera_set took it; inv[] is SCARAMUZZA's inv_poly, zero beyond n_inv.
struct CamProj {
    int32_t model, set, no_distortion, n_inv;
    double p[VIO_CAMERA_MAX_PARAMS];
    double inv[VIO_CAMERA_INV_POLY_MAX];
};

inline CamProj cam_project_form(const vio_camera_model &m) {
    CamProj C;
    C.model = m.model; C.set = 1; C.n_inv = 0; C.no_distortion = 0;
    for (int i = 0; i < VIO_CAMERA_MAX_PARAMS; ++i) C.p[i] = m.params[i];
    for (double &x : C.inv) x = 0.0;
    const double *d = m.model == VIO_CAMERA_MODEL_PINHOLE ? m.params : m.model == VIO_CAMERA_MODEL_MEI ? m.params + 1 : nullptr;
    if (d) C.no_distortion = (d[0] == 0.0) && (d[1] == 0.0) && (d[2] == 0.0) && (d[3] == 0.0);      // m_noDistortion
    return C;
}

// p_d of p_u: PinholeCamera::spaceToPlane's and CataCamera::spaceToPlane's middle part, d = (k1, k2, p1, p2)
REJ_FN void cam_project_distort(const double *d, int no_distortion, double &x, double &y) {
    if (no_distortion) return;
    RejCam c;
    c.ik11 = 0.0; c.ik13 = 0.0; c.ik22 = 0.0; c.ik23 = 0.0;
    c.k1 = d[0]; c.k2 = d[1]; c.p1 = d[2]; c.p2 = d[3];
    c.no_distortion = 0; c.pad = 0;
    double dx, dy;
    rej_distortion(c, x, y, dx, dy);
    x = x + dx; y = y + dy;
}

REJ_FN int cam_project_finite(double x) { return x - x == 0.0; }     // (x - x is 0 exactly when x is finite)

// The pixel (u, v) of P and the point's flag byte.
REJ_FN int cam_project(const CamProj &C, double P0, double P1, double P2, double &u, double &v) {
    int flag = 0;
    if (C.model == VIO_CAMERA_MODEL_PINHOLE) {
        double x = P0 / P2, y = P1 / P2;
        cam_project_distort(C.p, C.no_distortion, x, y);
        u = C.p[4] * x + C.p[6]; v = C.p[5] * y + C.p[7];
        if (!(P2 > 0.0)) flag |= VIO_CAMERA_PROJECT_BEHIND;
    } else if (C.model == VIO_CAMERA_MODEL_MEI) {
        const double a = P0 * P0, b = P1 * P1, c = P2 * P2;
        const double z = P2 + C.p[0] * sqrt((a + b) + c);
        double x = P0 / z, y = P1 / z;
        cam_project_distort(C.p + 1, C.no_distortion, x, y);
        u = C.p[5] * x + C.p[7]; v = C.p[6] * y + C.p[8];
        if (!(z > 0.0)) flag |= VIO_CAMERA_PROJECT_BEHIND;
    } else if (C.model == VIO_CAMERA_MODEL_SCARAMUZZA) {
        const double a = P0 * P0, b = P1 * P1;
        const double norm = sqrt(a + b);
        const double theta = cam_atan2(-P2, norm);
        double rho = 0.0, theta_i = 1.0;
CAM_UNROLLED
        for (int i = 0; i < VIO_CAMERA_INV_POLY_MAX; ++i) {
            rho += theta_i * C.inv[i];
            theta_i *= theta;
        }
        const double inv_norm = 1.0 / norm;
        const double xn0 = P0 * inv_norm * rho, xn1 = P1 * inv_norm * rho;
        u = xn0 * C.p[5] + xn1 * C.p[6] + C.p[8];
        v = xn0 * C.p[7] + xn1 + C.p[9];
    } else {
        const double a = P0 * P0, b = P1 * P1;
        const double theta = cam_atan2(sqrt(a + b), P2);
        const double phi = cam_atan2(P1, P0);
        const double r = cam_kb_r(C.p, theta);
        const double x = r * cam_cos(phi), y = r * cam_sin(phi);
        u = C.p[4] * x + C.p[6]; v = C.p[5] * y + C.p[7];
    }
    if (!(cam_project_finite(P0) && cam_project_finite(P1) && cam_project_finite(P2) && cam_project_finite(u) && cam_project_finite(v))) {
        flag |= VIO_CAMERA_PROJECT_NOT_FINITE;
        u = NAN; v = NAN;
    }
    return flag;
}
