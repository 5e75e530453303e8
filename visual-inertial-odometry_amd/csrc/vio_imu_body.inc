// vio_imu_body.inc — k_imu_propagate, its helpers and ImuArgs: the one text of the IntegrationBase recurrence on the device.
// vio_imu.hip (libvio_imu_hip) and vio_est.hip (libvio_est_hip) include it after <hip/hip_runtime.h> and include/vio_backend.h;
// the comment at the head of vio_imu.hip describes the kernel (DESIGN.md sections 12 and 30).
#define IMU_NT 64                          // one wavefront per interval
#define IMU_LDF 17                         // F tile: 16 rows, row stride 17 doubles
#define IMU_LDG 21                         // G tile: 16 rows x 20 columns, row stride 21 doubles
#define IMU_REC 467                        // doubles of one vio_preint
#define R_SUMDT 0
#define R_DP 1
#define R_DQ 4
#define R_DV 8
#define R_BA 11
#define R_BG 14
#define R_JAC 17
#define R_COV (R_JAC + 225)
static_assert(sizeof(vio_preint) == IMU_REC * sizeof(double), "vio_preint is 467 contiguous doubles");

typedef double imu_v4d __attribute__((ext_vector_type(4)));     // accumulator of v_mfma_f64_16x16x4_f64

struct ImuArgs {
    const int64_t *off;        // [n + 1]
    const double *first;       // [n][6] acc0 | gyr0
    const double *dt;          // [S]
    const double *acc;         // [S][3]
    const double *gyr;         // [S][3]
    const double *bias;        // [count][6] ba | bg of the k-th listed interval
    const int *which;          // [count] interval of output k
    double *out;               // [count][IMU_REC]
    double sn[4];              // sqrt of the noise diagonal: acc_n, gyr_n, acc_w, gyr_w
};

#pragma clang fp contract(off)     // the state recurrence and the blocks of F and V: products and sums as the host routine rounds them

struct dm3 { double m[9]; };

__device__ __forceinline__ dm3 m3_mul(const dm3 &a, const dm3 &b) {
    dm3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
    return c;
}
__device__ __forceinline__ dm3 m3_hat(const double *v) { return dm3{{0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0}}; }
__device__ __forceinline__ dm3 m3_rot(const double *q) {        // Eigen toRotationMatrix on (x,y,z,w), no normalisation
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    return dm3{{1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)}};
}
__device__ __forceinline__ void m3_apply(const dm3 &R, const double *v, double *o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = R.m[3 * i] * v[0] + R.m[3 * i + 1] * v[1] + R.m[3 * i + 2] * v[2];
}
// element e of a wave-uniform 3 x 3 as a select chain (the empty asm keeps the compiler from turning the chain back into an indexed
// load of the array, which would put every block in scratch)
__device__ __forceinline__ double m3_pick(const dm3 &B, int e) {
    double v = B.m[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        double x = B.m[k];
        asm volatile("" : "+v"(x));
        v = e == k ? x : v;
    }
    return v;
}
// lanes 0..8 store the block B * s at (r0, c0) of a tile
__device__ __forceinline__ void put_block(double *T, int ld, int r0, int c0, const dm3 &B, double s, int lane) {
    if (lane < 9) T[(r0 + lane / 3) * ld + c0 + lane % 3] = m3_pick(B, lane) * s;
}
// lanes 0..2 store the diagonal of d * I at (r0, c0)
__device__ __forceinline__ void put_diag(double *T, int ld, int r0, int c0, double d, int lane) {
    if (lane < 3) T[(r0 + lane) * ld + c0 + lane] = d;
}

__global__ __launch_bounds__(IMU_NT) void k_imu_propagate(ImuArgs a) {
    __shared__ double sF[16 * IMU_LDF];
    __shared__ double sG[16 * IMU_LDG];
    const int lane = threadIdx.x;
    const int k = blockIdx.x;
    const int iv = a.which[k];
    const int64_t s0 = a.off[iv], s1 = a.off[iv + 1];
    double ba[3], bg[3], a0[3], g0[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ba[c] = a.bias[6 * k + c]; bg[c] = a.bias[6 * k + 3 + c];
        a0[c] = a.first[6 * (int64_t)iv + c]; g0[c] = a.first[6 * (int64_t)iv + 3 + c];
    }
    for (int e = lane; e < 16 * IMU_LDF; e += IMU_NT) sF[e] = 0.0;
    for (int e = lane; e < 16 * IMU_LDG; e += IMU_NT) sG[e] = 0.0;
    __syncthreads();
    put_diag(sF, IMU_LDF, 0, 0, 1.0, lane);                // the constant identity blocks of F
    put_diag(sF, IMU_LDF, 6, 6, 1.0, lane);
    put_diag(sF, IMU_LDF, 9, 9, 1.0, lane);
    put_diag(sF, IMU_LDF, 12, 12, 1.0, lane);

    const int col = lane & 15, rb = lane >> 4;
    imu_v4d J, C;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = rb + 4 * q;
        J[q] = (row == col && row < 15) ? 1.0 : 0.0;
        C[q] = 0.0;
    }
    double dp[3] = {0, 0, 0}, dv[3] = {0, 0, 0}, dq[4] = {0, 0, 0, 1}, sum_dt = 0;
    const double sn0 = a.sn[0], sn1 = a.sn[1], sn2 = a.sn[2], sn3 = a.sn[3];
    const dm3 I3{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    for (int64_t s = s0; s < s1; ++s) {
        const double h = a.dt[s];
        double a1[3], g1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { a1[c] = a.acc[3 * s + c]; g1[c] = a.gyr[3 * s + c]; }
        double ua0[3], ua1[3], w[3], x0[3], x1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { x0[c] = a0[c] - ba[c]; x1[c] = a1[c] - ba[c]; w[c] = 0.5 * (g0[c] + g1[c]) - bg[c]; }
        const dm3 Rd = m3_rot(dq);
        m3_apply(Rd, x0, ua0);
        const double iq[4] = {w[0] * h / 2, w[1] * h / 2, w[2] * h / 2, 1.0};
        const double rq[4] = {dq[3] * iq[0] + dq[0] * iq[3] + dq[1] * iq[2] - dq[2] * iq[1],
                              dq[3] * iq[1] + dq[1] * iq[3] + dq[2] * iq[0] - dq[0] * iq[2],
                              dq[3] * iq[2] + dq[2] * iq[3] + dq[0] * iq[1] - dq[1] * iq[0],
                              dq[3] * iq[3] - dq[0] * iq[0] - dq[1] * iq[1] - dq[2] * iq[2]};
        const dm3 Rr = m3_rot(rq);
        m3_apply(Rr, x1, ua1);
        double rp[3], rv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double ua = 0.5 * (ua0[c] + ua1[c]);
            rp[c] = dp[c] + dv[c] * h + 0.5 * ua * h * h;
            rv[c] = dv[c] + ua * h;
        }
        const dm3 Rw = m3_hat(w), Ra0 = m3_hat(x0), Ra1 = m3_hat(x1);
        dm3 ImW;
#pragma unroll
        for (int c = 0; c < 9; ++c) ImW.m[c] = I3.m[c] - Rw.m[c] * h;
        const dm3 RdA0 = m3_mul(Rd, Ra0), RrA1 = m3_mul(Rr, Ra1), RrA1I = m3_mul(RrA1, ImW);

        // F (the blocks the host's put() writes, same values) and G = V sqrt(N), column block by column block
        dm3 B;
#pragma unroll
        for (int c = 0; c < 9; ++c) B.m[c] = -0.25 * RdA0.m[c] * h * h + -0.25 * RrA1I.m[c] * h * h;
        put_block(sF, IMU_LDF, 0, 3, B, 1.0, lane);
        put_diag(sF, IMU_LDF, 0, 6, h, lane);
#pragma unroll
        for (int c = 0; c < 9; ++c) B.m[c] = -0.25 * (Rd.m[c] + Rr.m[c]) * h * h;
        put_block(sF, IMU_LDF, 0, 9, B, 1.0, lane);
#pragma unroll
        for (int c = 0; c < 9; ++c) B.m[c] = -0.25 * RrA1.m[c] * h * h * -h;
        put_block(sF, IMU_LDF, 0, 12, B, 1.0, lane);
        put_block(sF, IMU_LDF, 3, 3, ImW, 1.0, lane);
        put_diag(sF, IMU_LDF, 3, 12, -1.0 * h, lane);
#pragma unroll
        for (int c = 0; c < 9; ++c) B.m[c] = -0.5 * RdA0.m[c] * h + -0.5 * RrA1I.m[c] * h;
        put_block(sF, IMU_LDF, 6, 3, B, 1.0, lane);
#pragma unroll
        for (int c = 0; c < 9; ++c) B.m[c] = -0.5 * (Rd.m[c] + Rr.m[c]) * h;
        put_block(sF, IMU_LDF, 6, 9, B, 1.0, lane);
#pragma unroll
        for (int c = 0; c < 9; ++c) B.m[c] = -0.5 * RrA1.m[c] * h * -h;
        put_block(sF, IMU_LDF, 6, 12, B, 1.0, lane);

        const double v00 = 0.25 * h * h, v33 = 0.5 * h, v60 = 0.5 * h;
        put_block(sG, IMU_LDG, 0, 0, Rd, v00 * sn0, lane);     // V(0, 0) = Rd h^2 / 4, column block 0: acc_n
#pragma unroll
        for (int c = 0; c < 9; ++c) B.m[c] = 0.25 * -RrA1.m[c] * h * h * 0.5 * h;
        put_block(sG, IMU_LDG, 0, 3, B, sn1, lane);             // column blocks 3, 9: gyr_n
        put_block(sG, IMU_LDG, 0, 9, B, sn1, lane);
        put_block(sG, IMU_LDG, 0, 6, Rr, v00 * sn0, lane);      // column block 6: acc_n
        put_diag(sG, IMU_LDG, 3, 3, v33 * sn1, lane);
        put_diag(sG, IMU_LDG, 3, 9, v33 * sn1, lane);
        put_block(sG, IMU_LDG, 6, 0, Rd, v60 * sn0, lane);
#pragma unroll
        for (int c = 0; c < 9; ++c) B.m[c] = 0.5 * -RrA1.m[c] * h * 0.5 * h;
        put_block(sG, IMU_LDG, 6, 3, B, sn1, lane);
        put_block(sG, IMU_LDG, 6, 9, B, sn1, lane);
        put_block(sG, IMU_LDG, 6, 6, Rr, v60 * sn0, lane);
        put_diag(sG, IMU_LDG, 9, 12, h * sn2, lane);            // column block 12: acc_w
        put_diag(sG, IMU_LDG, 12, 15, h * sn3, lane);           // column block 15: gyr_w
        __syncthreads();
        double fa[4], ga[5];
#pragma unroll
        for (int q = 0; q < 4; ++q) fa[q] = sF[col * IMU_LDF + 4 * q + rb];
#pragma unroll
        for (int q = 0; q < 5; ++q) ga[q] = sG[col * IMU_LDG + 4 * q + rb];
        __syncthreads();                                        // (the next sample's blocks overwrite the tiles)

        imu_v4d Jn = {0, 0, 0, 0}, U = {0, 0, 0, 0}, Cn = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) Jn = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[q], J[q], Jn, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) U = __builtin_amdgcn_mfma_f64_16x16x4f64(C[q], fa[q], U, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 5; ++q) Cn = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[q], ga[q], Cn, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) Cn = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[q], U[q], Cn, 0, 0, 0);
        J = Jn;
        C = Cn;

        const double nq = sqrt(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) dq[c] = rq[c] / nq;
#pragma unroll
        for (int c = 0; c < 3; ++c) { dp[c] = rp[c]; dv[c] = rv[c]; a0[c] = a1[c]; g0[c] = g1[c]; }
        sum_dt += h;
    }

    double *o = a.out + (int64_t)k * IMU_REC;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = rb + 4 * q;
        if (row < 15 && col < 15) {
            o[R_JAC + 15 * row + col] = J[q];
            o[R_COV + 15 * row + col] = C[q];
        }
    }
    if (lane == 0) {
        o[R_SUMDT] = sum_dt;
#pragma unroll
        for (int c = 0; c < 3; ++c) { o[R_DP + c] = dp[c]; o[R_DV + c] = dv[c]; o[R_BA + c] = ba[c]; o[R_BG + c] = bg[c]; }
#pragma unroll
        for (int c = 0; c < 4; ++c) o[R_DQ + c] = dq[c];
    }
}
