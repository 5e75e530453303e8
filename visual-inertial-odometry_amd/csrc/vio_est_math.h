// vio_est_math.h — the arithmetic of the batched Estimator state (include/vio_est.h) that a host compiler can
// build too: the nav-state step of processIMU, matrix -> quaternion, R2ypr / ypr2R, the re-anchoring of double2vector, the gates of
// failureDetection and the four matrices of slideWindowOld.  Device code of csrc/vio_est.hip; plain C++ otherwise, so that
// tests/cpp/est_math_main.cpp can run it on the host and tests/test_est_reference.py can hold it to tests/est_reference.py.
// Contraction is off here for every includer: every product and sum is evaluated as written, left to right; include/vio_est.h writes
// the orders down.  3 x 3 matrices are row-major, quaternions (x, y, z, w).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define EST_FN __host__ __device__ __forceinline__
#else
#define EST_FN inline
#endif

constexpr int EST_WINDOW = 10;                      // WINDOW_SIZE
constexpr int EST_FRAMES = 11;                      // WINDOW_SIZE + 1
constexpr int EST_OFFS = 12;                        // offsets of a slot: 11 intervals and the end
constexpr int EST_MAX_SLOTS = 256;                  // VIO_EST_MAX_SLOTS
constexpr int EST_MAX_SAMPLES = 4096;               // VIO_EST_MAX_SAMPLES
constexpr int EST_GATE_NONE = 0, EST_GATE_BA = 1, EST_GATE_BG = 2, EST_GATE_TRANSLATION = 3, EST_GATE_Z = 4;
constexpr double EST_PI = 3.14159265358979323846;   // M_PI

// c = a b, every element (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j; c may not alias a or b
EST_FN void est_mul33(const double *a, const double *b, double *c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double p0 = a[3 * i] * b[j], p1 = a[3 * i + 1] * b[3 + j], p2 = a[3 * i + 2] * b[6 + j];
            c[3 * i + j] = (p0 + p1) + p2;
        }
}

// o = R v, every element (R_i0 v_0 + R_i1 v_1) + R_i2 v_2; o may not alias v
EST_FN void est_apply(const double *R, const double *v, double *o) {
    for (int i = 0; i < 3; ++i) {
        const double p0 = R[3 * i] * v[0], p1 = R[3 * i + 1] * v[1], p2 = R[3 * i + 2] * v[2];
        o[i] = (p0 + p1) + p2;
    }
}

EST_FN void est_transpose(const double *a, double *t) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[3 * i + j] = a[3 * j + i];
}

// Eigen's Quaternion::toRotationMatrix on (x, y, z, w), no normalisation
EST_FN void est_quat_to_rot(const double *q, double *m) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    m[0] = 1 - (tyy + tzz); m[1] = txy - twz;       m[2] = txz + twy;
    m[3] = txy + twz;       m[4] = 1 - (txx + tzz); m[5] = tyz - twx;
    m[6] = txz - twy;       m[7] = tyz + twx;       m[8] = 1 - (txx + tyy);
}

// Eigen's Quaternion(Matrix3) (quaternionbase_assign_impl<Other, 3, 3>): the trace branch first, the largest diagonal otherwise; not
// normalised.  Returns the branch taken: 0 trace, 1 + i for diagonal i.
EST_FN int est_rot_to_quat(const double *m, double *q) {
    double t = (m[0] + m[4]) + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
        return 0;
    }
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
    q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
    q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    return 1 + i;
}

// One sample of processIMU's propagation (estimator.cpp:128-135) on Rs[j], Ps[j], Vs[j], from (acc_0, gyr_0) to (acc, gyr).
EST_FN void est_imu_step(double *Rs, double *Ps, double *Vs, const double *Ba, const double *Bg, const double *g, const double *acc0,
                         const double *gyr0, double dt, const double *acc, const double *gyr) {
    double x0[3], x1[3], r[3], un_acc_0[3], un_acc_1[3], q[4], M[9], Rn[9];
    for (int c = 0; c < 3; ++c) x0[c] = acc0[c] - Ba[c];
    est_apply(Rs, x0, r);
    for (int c = 0; c < 3; ++c) un_acc_0[c] = r[c] - g[c];                       // Rs (acc_0 - Ba) - g
    for (int c = 0; c < 3; ++c) {
        const double un_gyr = 0.5 * (gyr0[c] + gyr[c]) - Bg[c];                  // 0.5 (gyr_0 + gyr) - Bg
        q[c] = (un_gyr * dt) / 2.0;                                              // deltaQ: (theta / 2, 1), not normalised
    }
    q[3] = 1.0;
    est_quat_to_rot(q, M);
    est_mul33(Rs, M, Rn);                                                        // Rs *= deltaQ(un_gyr dt).toRotationMatrix()
    for (int c = 0; c < 9; ++c) Rs[c] = Rn[c];
    for (int c = 0; c < 3; ++c) x1[c] = acc[c] - Ba[c];
    est_apply(Rs, x1, r);
    for (int c = 0; c < 3; ++c) un_acc_1[c] = r[c] - g[c];
    const double hdd = (0.5 * dt) * dt;                                          // 0.5 * dt * dt, left to right
    for (int c = 0; c < 3; ++c) {
        const double un_acc = 0.5 * (un_acc_0[c] + un_acc_1[c]);
        Ps[c] = Ps[c] + (dt * Vs[c] + hdd * un_acc);                             // Ps += dt Vs + 0.5 dt dt un_acc
        Vs[c] = Vs[c] + dt * un_acc;                                             // Vs += dt un_acc
    }
}

// Utility::R2ypr: degrees
EST_FN void est_R2ypr(const double *R, double *ypr) {
    const double n0 = R[0], n1 = R[3], n2 = R[6], o0 = R[1], o1 = R[4], a0 = R[2], a1 = R[5];
    const double y = atan2(n1, n0);
    const double cy = cos(y), sy = sin(y);
    const double p = atan2(-n2, n0 * cy + n1 * sy);
    const double r = atan2(a0 * sy - a1 * cy, -o0 * sy + o1 * cy);
    ypr[0] = y / EST_PI * 180.0;
    ypr[1] = p / EST_PI * 180.0;
    ypr[2] = r / EST_PI * 180.0;
}

// Utility::ypr2R(y, 0, 0): Rz Ry Rx with Ry = Rx = I, that is Rz itself
EST_FN void est_yaw_rot(double y_deg, double *R) {
    const double y = y_deg / 180.0 * EST_PI;
    const double c = cos(y), s = sin(y);
    R[0] = c; R[1] = -s; R[2] = 0.0;
    R[3] = s; R[4] = c;  R[5] = 0.0;
    R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
}

// double2vector's rot_diff (estimator.cpp:551-577).  R_origin is Rs[0], or last_R0 in the failure_occur branch; Rs0 is Rs[0] either
// way (the singular branch reads it); q0 is para_Pose[0]'s quaternion.  Returns 1 in the singular branch.
EST_FN int est_rot_diff(const double *R_origin, const double *Rs0, const double *q0, double *rot_diff) {
    double o[3], o0[3], R00[9];
    est_R2ypr(R_origin, o);
    est_quat_to_rot(q0, R00);
    est_R2ypr(R00, o0);
    const double y_diff = o[0] - o0[0];
    est_yaw_rot(y_diff, rot_diff);
    if (fabs(fabs(o[1]) - 90) < 1.0 || fabs(fabs(o0[1]) - 90) < 1.0) {
        double T[9];
        est_transpose(R00, T);
        est_mul33(Rs0, T, rot_diff);
        return 1;
    }
    return 0;
}

// One frame of double2vector (:579-600): pose / sb are para_Pose[i] / para_SpeedBias[i], p0 is para_Pose[0]'s position.
EST_FN void est_update_frame(const double *rot_diff, const double *origin_P0, const double *pose, const double *p0, const double *sb,
                             double *Rs, double *Ps, double *Vs, double *Ba, double *Bg) {
    const double x = pose[3], y = pose[4], z = pose[5], w = pose[6];
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);                    // normalized()
    const double q[4] = {x / n, y / n, z / n, w / n};
    double M[9], d[3], r[3];
    est_quat_to_rot(q, M);
    est_mul33(rot_diff, M, Rs);
    for (int c = 0; c < 3; ++c) d[c] = pose[c] - p0[c];
    est_apply(rot_diff, d, r);
    for (int c = 0; c < 3; ++c) Ps[c] = r[c] + origin_P0[c];
    est_apply(rot_diff, sb, Vs);
    for (int c = 0; c < 3; ++c) { Ba[c] = sb[3 + c]; Bg[c] = sb[6 + c]; }
}

EST_FN double est_norm3(const double *v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// failureDetection (:645-691), the active gates in source order
EST_FN int est_gate(const double *Ba10, const double *Bg10, const double *P10, const double *last_P) {
    if (est_norm3(Ba10) > 2.5) return EST_GATE_BA;
    if (est_norm3(Bg10) > 1.0) return EST_GATE_BG;
    const double d[3] = {P10[0] - last_P[0], P10[1] - last_P[1], P10[2] - last_P[2]};
    if (est_norm3(d) > 5) return EST_GATE_TRANSLATION;
    if (fabs(P10[2] - last_P[2]) > 1) return EST_GATE_Z;
    return EST_GATE_NONE;
}

// slideWindowOld (:1254-1259): R0 = back_R0 ric, R1 = Rs[0] ric, P0 = back_P0 + back_R0 tic, P1 = Ps[0] + Rs[0] tic
EST_FN void est_slide_mats(const double *back_R0, const double *back_P0, const double *Rs0, const double *Ps0, const double *ric,
                           const double *tic, double *marg_R, double *marg_P, double *new_R, double *new_P) {
    double r[3];
    est_mul33(back_R0, ric, marg_R);
    est_mul33(Rs0, ric, new_R);
    est_apply(back_R0, tic, r);
    for (int c = 0; c < 3; ++c) marg_P[c] = back_P0[c] + r[c];
    est_apply(Rs0, tic, r);
    for (int c = 0; c < 3; ++c) new_P[c] = Ps0[c] + r[c];
}
