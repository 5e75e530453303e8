// vio_flow_body.inc — the pyramid and tracking kernels and their launches, the one copy libvio_flow_hip (vio_flow.hip, at
// file scope) and libvio_frame_hip (vio_frame.hip, inside a namespace of its own) compile (DESIGN.md sections 19 and 23).  The including
// file has included <hip/hip_runtime.h>, <cstdint>, vio_flow_math.h and vio_flow_host.h (the descriptor tables and MAXL), and has
// contraction off: products and sums round as the host restatement's (tests/flow_reference.py) do.
//
//   k_flow_pyr_down   one launch per level, every image of the call in the grid (blockIdx.y), one thread per output pixel: the 5 x 5
//                     [1 4 6 4 1] x [1 4 6 4 1] sum of the level below with BORDER_REFLECT_101, (sum + 128) >> 8.  Integers only.
//   k_flow_track      one wavefront per keypoint, WAVES wavefronts per workgroup; the keypoints of every item of the call are one
//                     flat grid through the host-made descriptor table.  The levels L - 1 .. 0 run inside the kernel with the state
//                     in registers.  Patch pixel m belongs to lane m mod 64 (at most PPL pixels per lane); the template's values
//                     (inverse mode: its gradients and H too) are formed once per level and stay in registers.  Each iteration every
//                     lane adds its pixels' terms in ascending order into six accumulators, the butterfly v[i] += v[i ^ s],
//                     s = 1 .. 32, leaves the same six sums in every lane, and every lane runs the 2 x 2 solve and the decision.
//                     The Scharr gradients are formed on the fly from the 4 x 4 pixels around a sample.  The level loop is
//                     flow_levels; k_flow_track<INV, true> runs it a second time, images exchanged, for the forward-backward
//                     check (include/vio_flow_back.h, DESIGN.md section 36), and writes a FlowBackOut row beside the FlowOut row.
// Keypoints of one workgroup end after different iteration counts, so k_flow_track has no workgroup barrier: shuffles only.  Every
// lane of a wavefront holds the same loop state, so the trip counts are uniform within the wavefront.  No floating-point atomics.
// An item names every level of its two images by address and row pitch: the host-array library packs rows tightly into one buffer
// (pitch = width), the resident library points at frames that stay where they are, level 0 at the pitch the CLAHE kernels write.
constexpr int WAVE = 64;
constexpr int WAVES = 4;                // keypoints per workgroup
constexpr int NT = WAVE * WAVES;
constexpr int PPL = (4 * VIO_FLOW_MAX_HALF_PATCH * VIO_FLOW_MAX_HALF_PATCH) / WAVE;     // patch pixels per lane at the largest patch

__global__ __launch_bounds__(NT) void k_flow_pyr_down(PyrArgs a) {
    const int img = blockIdx.y;
    if (img >= a.nimg) return;
    const FlowItemD &D = a.items[a.both ? img >> 1 : img];
    if (!D.active) return;
    const bool nxt = a.both ? (img & 1) != 0 : true;
    const int k = a.level;
    const int w = D.w[k], h = D.h[k], ow = D.w[k + 1], oh = D.h[k + 1];
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= ow * oh) return;
    const int ox = id % ow, oy = id / ow;
    const uint8_t *src = nxt ? D.next[k] : D.prev[k];
    uint8_t *dst = nxt ? D.next[k + 1] : D.prev[k + 1];
    const int kw[5] = {1, 4, 6, 4, 1};
    int cols[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) cols[i] = refl(2 * ox - 2 + i, w);
    int sum = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t *row = src + (int64_t)refl(2 * oy - 2 + j, h) * D.pitch[k];
        int r = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) r += kw[i] * (int)row[cols[i]];
        sum += kw[j] * r;
    }
    dst[(int64_t)oy * D.pitch[k + 1] + ox] = (uint8_t)((sum + 128) >> 8);
}

template <int N> __device__ __forceinline__ void butterfly(double *v) {
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = v[e] + __shfl_xor(v[e], s, WAVE);
    }
}

// The levels top - 1 .. 0 of one keypoint on its wavefront: the template pyramid Tp at (px, py), the moving pyramid Ip, the start
// (gx, gy) if has_guess.  Leaves the position (sx, sy), level 0's success, its iterations and the last of their costs.
template <bool INV> __device__ __forceinline__ void flow_levels(const FlowItemD &D, uint8_t *const *Tp, uint8_t *const *Ip, float px, float py, bool has_guess,
                                                                float gx, float gy, int top, int hp, int max_iter, int early_stop, int lane,
                                                                const int *pdu, const int *pdv, float &sx, float &sy, bool &ok, int &its,
                                                                double &cost_last) {
    const int side = 2 * hp, npix = side * side;
    sx = 0.f; sy = 0.f;
    ok = false; its = 0; cost_last = NAN;
    for (int l = top - 1; l >= 0; --l) {
        const double scale = ldexp(1.0, -l);
        const float tx = (float)((double)px * scale), ty = (float)((double)py * scale);
        if (l == top - 1) {
            sx = has_guess ? (float)((double)gx * scale) : tx;
            sy = has_guess ? (float)((double)gy * scale) : ty;
        }
        const double x0 = tx, y0 = ty;
        double dx = (double)sx - x0, dy = (double)sy - y0;
        const int w = D.w[l], h = D.h[l], pitch = D.pitch[l];
        const uint8_t *T = Tp[l], *I = Ip[l];
        ok = false; its = 0; cost_last = NAN;
        if (valid_patch(x0, y0, w, h, hp)) {
            double tv[PPL], tjx[INV ? PPL : 1], tjy[INV ? PPL : 1], Hs[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                tv[j] = 0.0;
                if constexpr (INV) { tjx[j] = 0.0; tjy[j] = 0.0; }
                if (j * WAVE < npix && j * WAVE + lane < npix) {
                    double g0 = 0.0, g1 = 0.0;
                    sample_pitched<INV>(T, pitch, w, h, x0 + (double)pdu[j], y0 + (double)pdv[j], tv[j], g0, g1);
                    if constexpr (INV) {
                        tjx[j] = g0; tjy[j] = g1;
                        Hs[0] = Hs[0] + g0 * g0; Hs[1] = Hs[1] + g0 * g1; Hs[2] = Hs[2] + g1 * g1;
                    }
                }
            }
            if (INV) butterfly<3>(Hs);
            double cost_prev = DBL_MAX;
            for (int it = 0; it < max_iter; ++it) {
                const double x = x0 + dx, y = y0 + dy;
                if (!valid_patch(x, y, w, h, hp)) { ok = false; break; }
                double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < PPL; ++j) {
                    if (j * WAVE < npix && j * WAVE + lane < npix) {
                        double iv, jx = 0.0, jy = 0.0;
                        sample_pitched<!INV>(I, pitch, w, h, x + (double)pdu[j], y + (double)pdv[j], iv, jx, jy);
                        const double err = tv[j] - iv;
                        if constexpr (INV) { jx = tjx[j]; jy = tjy[j]; }
                        else { v[0] = v[0] + jx * jx; v[1] = v[1] + jx * jy; v[2] = v[2] + jy * jy; }
                        v[3] = v[3] + err * jx; v[4] = v[4] + err * jy; v[5] = v[5] + (0.5 * err) * err;
                    }
                }
                if (INV) { butterfly<3>(v + 3); v[0] = Hs[0]; v[1] = Hs[1]; v[2] = Hs[2]; }
                else butterfly<6>(v);
                double dp0, dp1;
                solve2(v[0], v[1], v[2], v[3], v[4], dp0, dp1);
                its += 1;
                cost_last = v[5];
                if (isnan(dp0) || isnan(dp1)) { ok = false; break; }
                if (cost_prev <= v[5]) break;
                if (early_stop) cost_prev = v[5];
                dx = dx + dp0; dy = dy + dp1;
                ok = true;
            }
        }
        sx = tx + (float)dx; sy = ty + (float)dy;
        if (l > 0) { sx = (float)((double)sx / 0.5); sy = (float)((double)sy / 0.5); }
    }
}

// the arguments of k_flow_track<INV, BACK>: the forward pass's alone, or those with the check's behind them
template <bool BACK> struct FlowTrackArgs { using type = FlowArgs; };
template <> struct FlowTrackArgs<true> { using type = FlowBackArgs; };
__device__ __forceinline__ const FlowArgs &flow_forward_args(const FlowArgs &a) { return a; }
__device__ __forceinline__ const FlowArgs &flow_forward_args(const FlowBackArgs &a) { return a.f; }

__device__ __forceinline__ void flow_back_row_none(FlowBackOut *b) {
    b->x = NAN; b->y = NAN; b->status = VIO_FLOW_BACK_NOT_RUN; b->iterations = 0; b->cost = NAN; b->d2 = NAN;
}

// BACK: the forward-backward check of include/vio_flow_back.h.  A keypoint whose forward verdict is VIO_OK is followed back from the
// next pyramid into the prev pyramid on the same wavefront, the forward result and the keypoint still in registers; the verdict is
// uniform within the wavefront, so the second pass adds no divergence, no barrier and no shuffle beyond the butterfly's.
template <bool INV, bool BACK> __global__ __launch_bounds__(NT) void k_flow_track(typename FlowTrackArgs<BACK>::type ka) {
    const FlowArgs &a = flow_forward_args(ka);
    const int lane = threadIdx.x & (WAVE - 1);
    const int k = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (k >= a.npts) return;                        // (whole wavefronts: no barrier follows)
    const FlowPt P = a.pts[k];
    const FlowItemD &D = a.items[P.item];
    FlowOut *o = a.out + k;
    bool bad = !isfinite(P.px) || !isfinite(P.py);
    if (P.has_guess) bad = bad || !isfinite(P.gx) || !isfinite(P.gy);
    if (bad) {
        if (lane == 0) {
            o->x = NAN; o->y = NAN; o->status = VIO_ERR_NOT_FINITE; o->iterations = 0; o->cost = NAN;
            if constexpr (BACK) { if (ka.back) flow_back_row_none(ka.back + k); }
        }
        return;
    }
    const int hp = a.half_patch, side = 2 * hp;
    // this lane's patch pixels: (du, dv) of m = lane, lane + 64, ...
    int pdu[PPL], pdv[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int m = j * WAVE + lane;
        pdu[j] = m / side - hp; pdv[j] = m % side - hp;
    }
    float sx, sy;
    bool ok;
    int its;
    double cost_last;
    flow_levels<INV>(D, D.prev, D.next, P.px, P.py, P.has_guess != 0, P.gx, P.gy, a.levels, hp, a.max_iter, a.early_stop, lane, pdu, pdv, sx, sy,
                     ok, its, cost_last);
    int status = VIO_FLOW_FAIL_LOST;
    if (ok) {
        const double rx = rint((double)sx), ry = rint((double)sy), b = (double)a.border;
        const bool inside = b <= rx && rx < (double)D.w[0] - b && b <= ry && ry < (double)D.h[0] - b;
        status = inside ? VIO_OK : VIO_FLOW_FAIL_BORDER;
    }
    if constexpr (BACK) {
        FlowBackOut *bo = ka.back ? ka.back + k : nullptr;       // (no rows asked for: the verdict alone)
        if (status == VIO_OK) {
            float bx, by;
            bool bok;
            int bits;
            double bcost, d2;
            flow_levels<INV>(D, D.next, D.prev, sx, sy, true, P.px, P.py, ka.back_levels, hp, a.max_iter, a.early_stop, lane, pdu, pdv, bx, by,
                             bok, bits, bcost);
            status = flow_back_verdict(bok, P.px, P.py, bx, by, ka.max_d2, d2);
            if (lane == 0 && bo) { bo->x = bx; bo->y = by; bo->status = bok ? VIO_OK : VIO_FLOW_FAIL_LOST; bo->iterations = bits; bo->cost = bcost; bo->d2 = d2; }
        } else if (lane == 0 && bo) {
            flow_back_row_none(bo);
        }
    }
    if (lane == 0) { o->x = sx; o->y = sy; o->status = status; o->iterations = its; o->cost = cost_last; }
}

// one k_flow_pyr_down launch per level above 0 of nimg images (PyrArgs::both says which); max_px[l]: the largest level-l image of the call
inline void flow_launch_pyramids(hipStream_t q, const FlowItemD *items_d, int nimg, int both, int levels, const int64_t *max_px) {
    for (int l = 0; l + 1 < levels; ++l) {
        PyrArgs pa;
        pa.items = items_d; pa.level = l; pa.nimg = nimg; pa.both = both; pa.pad = 0;
        hipLaunchKernelGGL(k_flow_pyr_down, dim3((unsigned)((max_px[l + 1] + NT - 1) / NT), (unsigned)nimg), dim3(NT), 0, q, pa);
    }
}

inline void flow_launch_track(hipStream_t q, const FlowArgs &a, bool inverse) {
    const dim3 grid((unsigned)((a.npts + WAVES - 1) / WAVES));
    if (inverse) hipLaunchKernelGGL((k_flow_track<true, false>), grid, dim3(NT), 0, q, a);
    else hipLaunchKernelGGL((k_flow_track<false, false>), grid, dim3(NT), 0, q, a);
}

// the same grid with the forward-backward check in it
inline void flow_launch_track_back(hipStream_t q, const FlowBackArgs &a, bool inverse) {
    const dim3 grid((unsigned)((a.f.npts + WAVES - 1) / WAVES));
    if (inverse) hipLaunchKernelGGL((k_flow_track<true, true>), grid, dim3(NT), 0, q, a);
    else hipLaunchKernelGGL((k_flow_track<false, true>), grid, dim3(NT), 0, q, a);
}
