// vio_reject_body.inc — k_reject_lift and k_reject_ransac with the lift's launch, the one copy libvio_reject_hip (vio_reject.hip,
// at file scope) and libvio_frame_hip (vio_frame.hip, inside a namespace of its own) compile (DESIGN.md sections 21 and 24; the
// kernels are described at the top of vio_reject.hip).  The including file has included <hip/hip_runtime.h>, <cstdint>,
// ../../include/vio_reject.h, vio_reject_math.h, vio_sfm_math.h and vio_reject_host.h (the descriptor tables), and has contraction off.
// The kernels take n, active, m and every offset from the tables in device memory: the host-array library writes them on the host,
// the resident library's glue kernels (vio_front_body.inc) write the counts on the device.
// The lift is reached through the customisation points of vio_reject_host.h (the REJ_RAY ... REJ_PROLOGUE_END macros):
// libvio_camera_hip (vio_camera.hip) compiles this text against its own, for the four camera models and a camera per item.
constexpr int NT = VIO_REJECT_THREADS;
constexpr int ROUND = VIO_REJECT_ROUND;
constexpr int CHUNK = VIO_REJECT_ID_CHUNK;
constexpr int MINP = VIO_REJECT_MIN_POINTS;
static_assert(ROUND == 64, "a round is one wavefront");
static_assert(VIO_REJECT_MAX_HYPOTHESES == VIO_SFM_MAX_HYPOTHESES && VIO_REJECT_DEFAULT_HYPOTHESES == VIO_SFM_DEFAULT_HYPOTHESES, "the RANSAC is vio_sfm.h's");
static_assert(162 * 8 * ROUND + 9 * 8 * ROUND <= 160 * 1024, "the round's matrices fit a CU's LDS");

// ---------------------------------------------------------------------------------------------------------
// k_reject_lift
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_reject_lift(LiftArgs a) {
    __shared__ long long s_ids[CHUNK];
    const int item = blockIdx.y;
    if (item >= a.count) return;
    const LiftItem &D = a.items[item];
    if ((int)blockIdx.x * NT >= D.n) return;                 // (the whole workgroup: no barrier was reached)
    const int i = blockIdx.x * NT + threadIdx.x;
    const bool on = i < D.n;
    REJ_RAY(r);
    if (on) {
        const float *p = a.pts + D.o_pts + 2 * (int64_t)i;
        REJ_ITEM_LIFT(a, D, i, (double)p[0], (double)p[1], r);
    }
    if (a.bare) {
        if (on) { REJ_STORE_BARE(a, D, i, r); }
        return;
    }
    const float ux = REJ_UN_X(r), uy = REJ_UN_Y(r);
    if (!D.active) {                                         // a point of the item is not finite
        if (on) {
            a.un[2 * (D.o_out + i)] = NAN; a.un[2 * (D.o_out + i) + 1] = NAN;
            a.vel[2 * (D.o_out + i)] = NAN; a.vel[2 * (D.o_out + i) + 1] = NAN;
        }
        return;
    }
    const long long id = on ? a.ids[D.o_ids + i] : -1ll;
    const long long *prev = a.ids + D.o_ids + D.n;
    int found = -1;
    for (int c0 = 0; c0 < D.m; c0 += CHUNK) {                // (D.m is the workgroup's: every thread meets every barrier)
        const int len = D.m - c0 < CHUNK ? D.m - c0 : CHUNK;
        __syncthreads();
        for (int j = threadIdx.x; j < len; j += NT) s_ids[j] = prev[c0 + j];
        __syncthreads();
        if (id != -1ll && found < 0)
            for (int j = 0; j < len; ++j)
                if (s_ids[j] == id) { found = c0 + j; break; }
    }
    if (!on) return;
    float vx = 0.f, vy = 0.f;
    if (found >= 0) {
        const float *q = a.pts + D.o_prev + 2 * (int64_t)found;
        vx = rej_velocity(ux, q[0], D.dt); vy = rej_velocity(uy, q[1], D.dt);
    }
    a.un[2 * (D.o_out + i)] = ux; a.un[2 * (D.o_out + i) + 1] = uy;
    a.vel[2 * (D.o_out + i)] = vx; a.vel[2 * (D.o_out + i) + 1] = vy;
}

// ---------------------------------------------------------------------------------------------------------
// k_reject_ransac
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rej_hash4(uint32_t seed, uint32_t i, uint32_t h, uint32_t k) {
    return mix32(mix32(mix32(mix32(seed + 0x9e3779b9u) + i) + h) + k);
}

// sample8 of vio_sfm.hip with every index a constant (the insertion is a chain of selects): taken and out stay in registers
__device__ __forceinline__ void rej_sample8(uint32_t seed, uint32_t pair, uint32_t h, int n, int *out) {
    int taken[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int idx = (int)(rej_hash4(seed, pair, h, (uint32_t)k) % (uint32_t)(n - k));
        int pos = 0;
#pragma unroll
        for (int m = 0; m < k; ++m)                          // taken is ascending: the entries <= idx (as it grows) are a prefix
            if (pos == m && idx >= taken[m]) { ++idx; ++pos; }
#pragma unroll
        for (int m = k; m > 0; --m)
            if (m > pos) taken[m] = taken[m - 1];
#pragma unroll
        for (int m = 0; m <= k; ++m)
            if (m == pos) taken[m] = idx;
        out[k] = idx;
    }
}

// entry t of the upper triangle of a 9 x 9 matrix, row by row: (i, j), i <= j
__device__ __forceinline__ void tri_entry(int t, int &i, int &j) {
    i = 0;
    int len = 9;
    while (t >= len) { t -= len; --len; ++i; }
    j = i + t;
}

__device__ __forceinline__ double row_entry(const double *r, int i) {
    double v = r[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) v = i == k ? r[k] : v;
    return v;
}

__global__ __launch_bounds__(NT) void k_reject_ransac(RansacArgs a) {
    __shared__ double s_N[81 * ROUND], s_V[81 * ROUND];      // entry e of lane l at [e * ROUND + l]
    __shared__ double s_F[ROUND][9];                         // the round's models
    __shared__ double s_best[9], s_E[9];
    __shared__ HartleyScale s_h;
    __shared__ double s_sum[4];
    __shared__ int s_cnt[ROUND];
    __shared__ int s_i[4];                                   // best count, best h, ok, final inliers

    const RejPair P = a.pairs[blockIdx.x];
    if (!P.active) return;                                   // (n < 8 or a point that is not finite: the host writes the result)
    const int tid = threadIdx.x, n = P.n;
    double *corr = a.corr + P.o_corr;
    int32_t *flag = a.flag + P.o_pt;
    uint8_t *mask = a.mask + P.o_pt;
    RejRes *o = a.res + blockIdx.x;

    // prologue: the lift, the virtual pixels, the float rounding
    {
        const float *cur = a.pts + P.o_pts, *forw = cur + 2 * (int64_t)n;
        REJ_PROLOGUE_BEGIN;
        for (int k = tid; k < n; k += NT) {
            REJ_RAY_UNSET(r);
            REJ_PAIR_LIFT(a, P, (double)cur[2 * k], (double)cur[2 * k + 1], r);
            corr[4 * k] = REJ_VIRTUAL_X(a, P, r); corr[4 * k + 1] = REJ_VIRTUAL_Y(a, P, r);
            REJ_PAIR_LIFT(a, P, (double)forw[2 * k], (double)forw[2 * k + 1], r);
            corr[4 * k + 2] = REJ_VIRTUAL_X(a, P, r); corr[4 * k + 3] = REJ_VIRTUAL_Y(a, P, r);
        }
        REJ_PROLOGUE_END(n, tid, mask, o);
    }
    if (tid == 0) { s_i[0] = -1; s_i[1] = -1; s_i[2] = 0; s_i[3] = 0; }
    __syncthreads();

    const double thr = a.thr;
    for (int base = 0; base < a.hyps; base += ROUND) {
        const int nh = a.hyps - base < ROUND ? a.hyps - base : ROUND;
        if (tid < ROUND) s_cnt[tid] = 0;
        if (tid < nh) {
            int idx[8];
            double Fm[9];
            rej_sample8(a.seed, P.pair, (uint32_t)(base + tid), n, idx);
            eight_point8_strided<ROUND>(corr, idx, s_N + tid, s_V + tid, Fm);
#pragma unroll
            for (int k = 0; k < 9; ++k) s_F[tid][k] = Fm[k];
        }
        __syncthreads();
        for (int e = tid; e < nh * n; e += NT) {
            const int h = e / n, k = e - h * n;
            if (epipolar_error(s_F[h], corr + 4 * k) <= thr) atomicAdd(&s_cnt[h], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int bc = s_i[0], bh = -1;
            for (int h = 0; h < nh; ++h)
                if (s_cnt[h] > bc) { bc = s_cnt[h]; bh = h; }        // (strictly more: ties stay with the lowest h)
            if (bh >= 0) {
                s_i[0] = bc; s_i[1] = base + bh;
                for (int k = 0; k < 9; ++k) s_best[k] = s_F[bh][k];
            }
        }
        __syncthreads();
    }

    const int best_c = s_i[0], hyp = s_i[1];
    bool ok = best_c >= MINP;
    if (ok) {
        // the refit on the winner's inliers, every sum in correspondence order
        for (int k = tid; k < n; k += NT) flag[k] = epipolar_error(s_best, corr + 4 * k) <= thr;
        __syncthreads();
        if (tid < 4) {
            double s = 0.0;
            for (int k = 0; k < n; ++k)
                if (flag[k]) s += corr[4 * k + tid];
            s_sum[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            s_h.ca[0] = s_sum[0] / best_c; s_h.ca[1] = s_sum[1] / best_c;
            s_h.cb[0] = s_sum[2] / best_c; s_h.cb[1] = s_sum[3] / best_c;
        }
        __syncthreads();
        if (tid < 2) {
            const double cx = tid ? s_h.cb[0] : s_h.ca[0], cy = tid ? s_h.cb[1] : s_h.ca[1];
            double s = 0.0;
            for (int k = 0; k < n; ++k)
                if (flag[k]) {
                    const double dx = corr[4 * k + 2 * tid] - cx, dy = corr[4 * k + 2 * tid + 1] - cy;
                    s += sqrt(dx * dx + dy * dy);
                }
            s_sum[tid] = sqrt(2.0) / (s / best_c);
        }
        __syncthreads();
        if (tid == 0) { s_h.sa = s_sum[0]; s_h.sb = s_sum[1]; }
        __syncthreads();
        if (tid < 45) {
            int i, j;
            tri_entry(tid, i, j);
            const HartleyScale hs = s_h;
            double s = 0.0;
            for (int k = 0; k < n; ++k)
                if (flag[k]) {
                    double r[9];
                    eight_point_row(corr + 4 * k, hs, r);
                    s += row_entry(r, i) * row_entry(r, j);
                }
            s_N[(9 * i + j) * ROUND] = s;                    // lane 0's column
            s_N[(9 * j + i) * ROUND] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double Fm[9];
            const HartleyScale hs = s_h;
            eight_point_finish_strided<ROUND>(s_N, s_V, hs, Fm);
            int fin = 1;
            for (int k = 0; k < 9; ++k) { s_E[k] = Fm[k]; fin &= isfinite(Fm[k]) != 0; }
            s_i[2] = fin;
        }
        __syncthreads();
        ok = s_i[2] != 0;
    }
    if (ok) {
        for (int k = tid; k < n; k += NT) {
            const int in = epipolar_error(s_E, corr + 4 * k) <= thr;
            mask[k] = (uint8_t)in;
            if (in) atomicAdd(&s_i[3], 1);
        }
        __syncthreads();
        if (tid == 0) { o->status = VIO_OK; o->hyp = hyp; o->n_inliers = s_i[3]; o->pad = 0; }
        if (tid < 9) o->F[tid] = s_E[tid];
    } else {
        for (int k = tid; k < n; k += NT) mask[k] = 1;
        if (tid == 0) { o->status = VIO_REJECT_FAIL_NO_MODEL; o->hyp = hyp; o->n_inliers = n; o->pad = 0; }
        if (tid < 9) o->F[tid] = NAN;
    }
}

// the lift of a.count items of at most max_n points each, on q
inline void rej_launch_lift(hipStream_t q, const LiftArgs &a, int max_n) {
    hipLaunchKernelGGL(k_reject_lift, dim3((unsigned)((max_n + NT - 1) / NT), (unsigned)a.count), dim3(NT), 0, q, a);
}
