// vio_imu_math.h — the IMU factor: its residual (IntegrationBase::evaluate, integration_base.h:160-186), the 14 non-zero 3 x 3 blocks
// of its Jacobian (edge_imu.cc:74-153) and the helpers the two share, under one floating-point rule: no contraction (see below).
//
// Included by vio_kernels.hip, at the place this code stood, by vio_marg.hip, whose IMU edge 0 -> 1 is thereby the solver's own
// linearisation, and by vio_residuals.hip, so that the residual whose chi2 the residual query reports is the solver's own function.
// The header switches contraction off on entry and back to the default (fast) on exit; the code of an includer behind the include
// is contracted again.
#ifndef VIO_IMU_MATH_H
#define VIO_IMU_MATH_H

#pragma clang fp contract(off)

#include "vio_device_math.h"
#include "vio_types.h"

// ---------------------------------------------------------------------------------------------------------
// IMU factor (one workgroup per edge, appended to the linearize grid)
// ---------------------------------------------------------------------------------------------------------
#define O_P 0
#define O_R 3
#define O_V 6
#define O_BA 9
#define O_BG 12

// The IMU factor's residual and Jacobian blocks are evaluated with NO floating-point contraction: every product and every sum is the
// IEEE operation the source states, in the order it states it (as the oracle's C is compiled).  With the compiler free to fuse a*b+c
// the result of these expressions depended on what surrounded them after inlining (a product with a second use is not fused), and two
// call sites of the same function — the IMU workgroups of d_imu_item, the chain workgroup of the GN loop — could differ in the last bit.
// The helpers of vio_device_math.h they use are restated here under the same rule.
#pragma clang fp contract(off)
__device__ __forceinline__ void nc_quat_to_R(const double *q, double *R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
__device__ __forceinline__ void nc_m3_mul(const double *A, const double *B, double *C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ dquat nc_qmul(dquat a, dquat b) {       // Eigen quaternion product
    dquat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}
__device__ __forceinline__ dquat nc_qinv(dquat q) {                // Eigen::QuaternionBase::inverse
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    dquat r = {0, 0, 0, 0};
    if (n2 > 0) { r.x = -q.x / n2; r.y = -q.y / n2; r.z = -q.z / n2; r.w = q.w / n2; }
    return r;
}
__device__ __forceinline__ void nc_qrot(dquat q, const double *v, double *o) {   // Eigen _transformVector
    double ux = q.y * v[2] - q.z * v[1], uy = q.z * v[0] - q.x * v[2], uz = q.x * v[1] - q.y * v[0];
    ux += ux; uy += uy; uz += uz;
    o[0] = v[0] + q.w * ux + (q.y * uz - q.z * uy);
    o[1] = v[1] + q.w * uy + (q.z * ux - q.x * uz);
    o[2] = v[2] + q.w * uz + (q.x * uy - q.y * ux);
}
struct ImuCommon {
    dquat Qi, Qj, Qi_inv, dq, cdq;
    double sum_dt;
    double dba[3], dbg[3];
};

__device__ __forceinline__ void d_qleft_br(dquat q, double *B) {      // Utility::Qleft bottom-right 3x3 (utility.h:48-56)
    double v[3] = {q.x, q.y, q.z};
    d_skew(v, B);
    B[0] += q.w; B[4] += q.w; B[8] += q.w;
}
__device__ __forceinline__ void d_qright_br(dquat q, double *B) {     // Utility::Qright bottom-right 3x3 (utility.h:58-66)
    double v[3] = {q.x, q.y, q.z}, S[9];
    d_skew(v, S);
#pragma unroll
    for (int k = 0; k < 9; ++k) B[k] = -S[k];
    B[0] += q.w; B[4] += q.w; B[8] += q.w;
}

__device__ void d_imu_common(const double *pre, const double *pi, const double *si, const double *pj, ImuCommon &c) {
    c.Qi = d_qload(pi); c.Qj = d_qload(pj);
    c.Qi_inv = nc_qinv(c.Qi);
    c.sum_dt = pre[PRE_SUMDT];
    c.dq.x = pre[PRE_DQ]; c.dq.y = pre[PRE_DQ + 1]; c.dq.z = pre[PRE_DQ + 2]; c.dq.w = pre[PRE_DQ + 3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { c.dba[k] = si[3 + k] - pre[PRE_BA + k]; c.dbg[k] = si[6 + k] - pre[PRE_BG + k]; }
    const double *Jm = pre + PRE_JAC;
    double th[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        th[i] = Jm[15 * (O_R + i) + O_BG] * c.dbg[0] + Jm[15 * (O_R + i) + O_BG + 1] * c.dbg[1] + Jm[15 * (O_R + i) + O_BG + 2] * c.dbg[2];
    dquat dth = {th[0] / 2.0, th[1] / 2.0, th[2] / 2.0, 1.0};      // Utility::deltaQ, not normalised
    c.cdq = nc_qmul(c.dq, dth);
}

// IntegrationBase::evaluate (integration_base.h:160-186)
__device__ void d_imu_residual(const double *pre, const double *G, const double *pi, const double *si, const double *pj,
                               const double *sj, const ImuCommon &c, double *res) {
    const double *Jm = pre + PRE_JAC;
    const double sum_dt = c.sum_dt;
    double cdp[3], cdv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double a = 0, b = 0, e = 0, f = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            a += Jm[15 * (O_V + i) + O_BA + j] * c.dba[j];
            b += Jm[15 * (O_V + i) + O_BG + j] * c.dbg[j];
            e += Jm[15 * (O_P + i) + O_BA + j] * c.dba[j];
            f += Jm[15 * (O_P + i) + O_BG + j] * c.dbg[j];
        }
        cdv[i] = pre[PRE_DV + i] + a + b;
        cdp[i] = pre[PRE_DP + i] + e + f;
    }
    double t[3], u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = 0.5 * G[k] * sum_dt * sum_dt + pj[k] - pi[k] - si[k] * sum_dt;
    nc_qrot(c.Qi_inv, t, u);
#pragma unroll
    for (int k = 0; k < 3; ++k) res[O_P + k] = u[k] - cdp[k];
    dquat qe = nc_qmul(nc_qinv(c.cdq), nc_qmul(c.Qi_inv, c.Qj));
    res[O_R] = 2 * qe.x; res[O_R + 1] = 2 * qe.y; res[O_R + 2] = 2 * qe.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = G[k] * sum_dt + sj[k] - si[k];
    nc_qrot(c.Qi_inv, t, u);
#pragma unroll
    for (int k = 0; k < 3; ++k) res[O_V + k] = u[k] - cdv[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { res[O_BA + k] = sj[3 + k] - si[3 + k]; res[O_BG + k] = sj[6 + k] - si[6 + k]; }
}

// One 3x3 block of the 15x30 Jacobian [J_pose_i | J_sb_i | J_pose_j | J_sb_j] (edge_imu.cc:74-153).
// `blk` enumerates the 14 non-zero blocks; sJ is the 15x30 row-major LDS image (zero-initialised).
// RiT = Qi.inverse().toRotationMatrix() (d_imu_rit)
__device__ __forceinline__ void d_imu_rit(const ImuCommon &c, double *RiT) {
    double qi[4] = {c.Qi_inv.x, c.Qi_inv.y, c.Qi_inv.z, c.Qi_inv.w};
    nc_quat_to_R(qi, RiT);
}
__device__ void d_imu_jac_block(int blk, const double *pre, const double *G, const double *pi, const double *si,
                                const double *pj, const double *sj, const ImuCommon &c, const double *RiT, double *sJ) {
    const double *Jm = pre + PRE_JAC;
    const double sum_dt = c.sum_dt;
    double B[9];
    int r0 = 0, c0 = 0;
    switch (blk) {
    case 0: r0 = O_P; c0 = 0 + O_P;       // jacobian_pose_i(O_P,O_P) = -Ri^T
        for (int k = 0; k < 9; ++k) B[k] = -RiT[k];
        break;
    case 1: { r0 = O_P; c0 = 0 + O_R;     // skew(Qi^-1 (0.5 G dt^2 + Pj - Pi - Vi dt))
        double t[3], u[3];
        for (int k = 0; k < 3; ++k) t[k] = 0.5 * G[k] * sum_dt * sum_dt + pj[k] - pi[k] - si[k] * sum_dt;
        nc_qrot(c.Qi_inv, t, u); d_skew(u, B);
        break; }
    case 2: { r0 = O_R; c0 = 0 + O_R;     // -(Qleft(Qj^-1 Qi) Qright(corrected_delta_q)).bottomRight
        dquat a = nc_qmul(nc_qinv(c.Qj), c.Qi), b = c.cdq;
        double La[9], Rb[9], P[9];
        d_qleft_br(a, La); d_qright_br(b, Rb); nc_m3_mul(La, Rb, P);
        const double va[3] = {a.x, a.y, a.z}, vb[3] = {b.x, b.y, b.z};
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) B[3 * i + j] = -(va[i] * (-vb[j]) + P[3 * i + j]);
        break; }
    case 3: { r0 = O_V; c0 = 0 + O_R;     // skew(Qi^-1 (G dt + Vj - Vi))
        double t[3], u[3];
        for (int k = 0; k < 3; ++k) t[k] = G[k] * sum_dt + sj[k] - si[k];
        nc_qrot(c.Qi_inv, t, u); d_skew(u, B);
        break; }
    case 4: r0 = O_P; c0 = 6 + 0;         // speedbias_i(O_P, V) = -Ri^T dt
        for (int k = 0; k < 9; ++k) B[k] = -RiT[k] * sum_dt;
        break;
    case 5: r0 = O_P; c0 = 6 + 3;         // -dp_dba
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) B[3 * i + j] = -Jm[15 * (O_P + i) + O_BA + j];
        break;
    case 6: r0 = O_P; c0 = 6 + 6;         // -dp_dbg
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) B[3 * i + j] = -Jm[15 * (O_P + i) + O_BG + j];
        break;
    case 7: { r0 = O_R; c0 = 6 + 6;       // -Qleft(Qj^-1 Qi delta_q).bottomRight * dq_dbg  (delta_q, not corrected: edge_imu.cc:107-109)
        double L[9], nL[9], D[9];
        d_qleft_br(nc_qmul(nc_qmul(nc_qinv(c.Qj), c.Qi), c.dq), L);
        for (int k = 0; k < 9; ++k) nL[k] = -L[k];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) D[3 * i + j] = Jm[15 * (O_R + i) + O_BG + j];
        nc_m3_mul(nL, D, B);
        break; }
    case 8: r0 = O_V; c0 = 6 + 0;         // -Ri^T
        for (int k = 0; k < 9; ++k) B[k] = -RiT[k];
        break;
    case 9: r0 = O_V; c0 = 6 + 3;         // -dv_dba
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) B[3 * i + j] = -Jm[15 * (O_V + i) + O_BA + j];
        break;
    case 10: r0 = O_V; c0 = 6 + 6;        // -dv_dbg
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) B[3 * i + j] = -Jm[15 * (O_V + i) + O_BG + j];
        break;
    case 11: r0 = O_P; c0 = 15 + O_P;     // pose_j(O_P,O_P) = Ri^T
        for (int k = 0; k < 9; ++k) B[k] = RiT[k];
        break;
    case 12: { r0 = O_R; c0 = 15 + O_R;   // Qleft(corrected_dq^-1 Qi^-1 Qj).bottomRight
        d_qleft_br(nc_qmul(nc_qmul(nc_qinv(c.cdq), c.Qi_inv), c.Qj), B);
        break; }
    case 13: r0 = O_V; c0 = 21 + 0;       // speedbias_j(O_V,V) = Ri^T
        for (int k = 0; k < 9; ++k) B[k] = RiT[k];
        break;
    default: return;
    }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) sJ[30 * (r0 + i) + c0 + j] = B[3 * i + j];
}

#pragma clang fp contract(fast)

#endif
