// vio_fm_predict_math.h — the arithmetic of include/vio_fm_predict.h that a host compiler can build too: the
// rule of a predicted row, the rotation matrix of a quaternion, the constant-velocity next pose and the point of one row in the next
// camera.  Device code of csrc/vio_fm_predict_body.inc; plain C++ otherwise, so that tests/cpp/fm_predict_main.cpp can run it on the
// host and tests/test_fm_predict_cpu.py can hold it to tests/fm_predict_reference.py bit for bit.  Contraction is off, as in
// vio_fm_math.h: every product and sum is rounded on its own, every dot product is (a0 b0 + a1 b1) + a2 b2.  Matrices are row-major.
#pragma once

#include <cstdint>

#include "vio_fm_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// a row is predicted iff it has a depth, two observations and ends at frame_count (start >= 0 keeps a corrupted table from indexing
// in front of the poses; vio_fm_tracks_set refuses such a row)
FM_FN bool fmp_qualifies(double depth, int32_t n_obs, int32_t start, int32_t frame_count) {
    return depth > 0 && n_obs >= 2 && start >= 0 && start + n_obs - 1 == frame_count;
}

// the expressions of d_quat_to_R (vio_device_math.h), q = (x, y, z, w), under contraction off
FM_FN void fmp_quat_to_R(const double *q, double *R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

FM_FN double fmp_dot(double a0, double a1, double a2, double b0, double b1, double b2) {
    const double p0 = a0 * b0, p1 = a1 * b1, p2 = a2 * b2;
    return (p0 + p1) + p2;
}
// o = A v and o = A^T v
FM_FN void fmp_mv(const double *A, const double *v, double *o) {
    for (int i = 0; i < 3; ++i) o[i] = fmp_dot(A[3 * i], A[3 * i + 1], A[3 * i + 2], v[0], v[1], v[2]);
}
FM_FN void fmp_tmv(const double *A, const double *v, double *o) {
    for (int i = 0; i < 3; ++i) o[i] = fmp_dot(A[i], A[3 + i], A[6 + i], v[0], v[1], v[2]);
}

// T_next = T_cur (T_prev^-1 T_cur)
FM_FN void fmp_next_pose(const double *Rp, const double *Pp, const double *Rc, const double *Pc, double *Rn, double *Pn) {
    double Rrel[9], d[3], trel[3], t[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rrel[3 * i + j] = fmp_dot(Rp[i], Rp[3 + i], Rp[6 + i], Rc[j], Rc[3 + j], Rc[6 + j]);
    for (int k = 0; k < 3; ++k) d[k] = Pc[k] - Pp[k];
    fmp_tmv(Rp, d, trel);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = fmp_dot(Rc[3 * i], Rc[3 * i + 1], Rc[3 * i + 2], Rrel[j], Rrel[3 + j], Rrel[6 + j]);
    fmp_mv(Rc, trel, t);
    for (int k = 0; k < 3; ++k) Pn[k] = t[k] + Pc[k];
}

// the row's point in the next camera: (x, y) its first observation, d its depth, (Rs, Ps) the pose of its start frame
FM_FN void fmp_point(double x, double y, double d, const double *ric, const double *tic, const double *Rs, const double *Ps,
                     const double *Rn, const double *Pn, double *out) {
    const double pc[3] = {d * x, d * y, d};
    double pi[3], pw[3], dl[3], pl[3], e[3];
    fmp_mv(ric, pc, pi);
    for (int k = 0; k < 3; ++k) pi[k] = pi[k] + tic[k];
    fmp_mv(Rs, pi, pw);
    for (int k = 0; k < 3; ++k) pw[k] = pw[k] + Ps[k];
    for (int k = 0; k < 3; ++k) dl[k] = pw[k] - Pn[k];
    fmp_tmv(Rn, dl, pl);
    for (int k = 0; k < 3; ++k) e[k] = pl[k] - tic[k];
    fmp_tmv(ric, e, out);
}
