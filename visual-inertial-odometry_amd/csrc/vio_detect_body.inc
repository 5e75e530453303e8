// vio_detect_body.inc — the four detection kernels, the greedy loop and their launches, the one copy libvio_detect_hip
// (vio_detect.hip, at file scope) and libvio_frame_hip (vio_frame.hip, inside a namespace of its own) compile (DESIGN.md sections 20 and
// 23).  The including file has included <hip/hip_runtime.h>, <cstdint>, vio_detect_math.h and vio_detect_host.h (the descriptor tables,
// TX and TY), and has contraction off (with this arithmetic it cannot change a bit).
//
//   k_detect_setmask     one workgroup per image: the greedy loop below over the tracked points, key (track_cnt, -index), disc <=.
//                        Leaves the kept centres and their indices in output order.
//   k_detect_response    a TX x TY tile per workgroup, every image of the call in the grid (blockIdx.z): the tile with a halo of 2 in
//                        LDS, the Sobel products at a halo of 1, the 3 x 3 box sums, R.  Integers up to the one sqrt.  Each wavefront
//                        then folds the R bits of its allowed pixels into the image's maximum with one integer atomicMax (the bit
//                        patterns of non-negative doubles order as the doubles do, and a maximum does not depend on the order).
//   k_detect_candidates  the same grid, one thread per pixel: the threshold, the 8 neighbours, allowed; a candidate's pixel index goes
//                        to the image's list through an integer counter.  The order of arrival is arbitrary.
//   k_detect_select      one workgroup per image: the greedy loop over the candidates, key (R bits, pixel index), disc <.
// The greedy loop: "take the sorted list in order and accept what no earlier accepted one is close to" is "repeatedly take the best
// remaining entry and strike those close to it".  A round is one pass over the list (strike against the last winner, else fold into
// the maximum), one reduction and one barrier; the rounds are bounded by a count known at launch.  No sort, no spin-waits, no
// synchronisation between workgroups; a thread only ever strikes the entries it reads itself.  No floating-point atomics.
// An item names its image and its mask by address and row pitch: the host-array library packs rows tightly (pitch = width), the
// resident library points at a frame's level 0 and at the slot's mask where they lie.  The response map is tightly packed in both.
constexpr int WAVE = 64;
constexpr int NT = TX * TY;             // threads of a tile
constexpr int NT_MASK = 256;            // threads of k_detect_setmask
constexpr int NT_SEL = 1024;            // threads of k_detect_select
constexpr uint32_t DEAD = 0x80000000u;  // a struck candidate (pixel indices are below 2^28)
static_assert(NT % WAVE == 0 && NT <= 1024, "a tile is whole wavefronts");

// ---------------------------------------------------------------------------------------------------------
// the greedy loop
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ DetKey key_shfl_xor(const DetKey &a, int s) {
    DetKey o;
    o.k = __shfl_xor(a.k, s, WAVE);
    o.x = __shfl_xor(a.x, s, WAVE);
    o.y = __shfl_xor(a.y, s, WAVE);
    return o;
}

// Src: load(i) -> DetKey (k == 0: struck) and kill(i); emit(position, winner) runs on thread 0.  slots: [2][NTH / 64] in LDS.  Every
// thread returns the number of entries taken.
template <int NTH, bool STRICT, class Src, class Emit>
__device__ __forceinline__ int greedy(Src &src, int n, int rounds, int32_t d2, Emit &emit, DetKey *slots) {
    constexpr int NW = NTH / WAVE;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    DetKey last = {0ull, 0, 0};
    int taken = 0;
    for (int r = 0; r < rounds; ++r) {
        DetKey best = {0ull, 0, 0};
        for (int i = tid; i < n; i += NTH) {
            const DetKey e = src.load(i);
            if (e.k == 0ull) continue;
            if (r > 0 && det_struck<STRICT>(e.x, e.y, last.x, last.y, d2)) {
                src.kill(i);
                continue;
            }
            if (det_key_before(e, best)) best = e;
        }
#pragma unroll
        for (int s = 1; s < WAVE; s <<= 1) {
            const DetKey o = key_shfl_xor(best, s);
            if (det_key_before(o, best)) best = o;
        }
        DetKey *slot = slots + (r & 1) * NW;            // (two sets: a round's slots are read while the next round's are written)
        if (lane == 0) slot[wv] = best;
        __syncthreads();
        best = slot[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const DetKey o = slot[w];
            if (det_key_before(o, best)) best = o;
        }
        if (best.k == 0ull) break;                      // (the same in every thread: nothing is left)
        if (tid == 0) emit(taken, best);
        last = best;
        taken += 1;
    }
    return taken;
}

struct TrackedSrc {
    const DetTrk *trk;
    unsigned long long *key;
    __device__ __forceinline__ DetKey load(int i) const {
        DetKey e;
        e.k = key[i]; e.x = trk[i].cx; e.y = trk[i].cy;
        return e;
    }
    __device__ __forceinline__ void kill(int i) const { key[i] = 0ull; }
};

struct TrackedEmit {
    int32_t *keep_order, *kept_xy;
    __device__ __forceinline__ void operator()(int pos, const DetKey &e) const {
        keep_order[pos] = (int32_t)(0xFFFFFFFFu - (uint32_t)(e.k & 0xFFFFFFFFull));
        kept_xy[2 * pos] = e.x; kept_xy[2 * pos + 1] = e.y;
    }
};

struct CandSrc {
    uint32_t *cand;
    const double *r;
    int32_t w;
    __device__ __forceinline__ DetKey load(int i) const {
        DetKey e = {0ull, 0, 0};
        const uint32_t p = cand[i];
        if (p & DEAD) return e;
        e.k = (unsigned long long)__double_as_longlong(r[p]);
        e.x = (int32_t)(p % (uint32_t)w); e.y = (int32_t)(p / (uint32_t)w);
        return e;
    }
    __device__ __forceinline__ void kill(int i) const { cand[i] |= DEAD; }
};

struct CandEmit {
    float *new_pts;
    __device__ __forceinline__ void operator()(int pos, const DetKey &e) const {
        new_pts[2 * pos] = (float)e.x; new_pts[2 * pos + 1] = (float)e.y;
    }
};

// ---------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT_MASK) void k_detect_setmask(DetArgs a) {
    __shared__ DetKey slots[2 * (NT_MASK / WAVE)];
    const int item = blockIdx.x;
    if (item >= a.count) return;
    const DetItemD &D = a.items[item];
    if (!D.active || D.n_tracked == 0) return;           // (n_kept stays 0)
    const DetTrk *trk = a.trk + D.trk;
    unsigned long long *key = a.tkey + D.trk;
    const uint8_t *mask = D.mask;
    // the keys; a point on a zero mask pixel is struck from the start.  Entry i belongs to thread i mod NT_MASK from here on.
    for (int i = threadIdx.x; i < D.n_tracked; i += NT_MASK) {
        const DetTrk t = trk[i];
        const bool on = !D.has_mask || mask[(int64_t)t.cy * D.pitch + t.cx] != 0;
        key[i] = on ? det_track_key(t.cnt, i) : 0ull;
    }
    TrackedSrc src = {trk, key};
    TrackedEmit emit = {a.keep_order + D.trk, a.kept_xy + 2 * (int64_t)D.trk};
    const int n_kept = greedy<NT_MASK, false>(src, D.n_tracked, D.n_tracked, a.d2, emit, slots);
    if (threadIdx.x == 0) a.res[item].n_kept = n_kept;
}

// allowed(p) of the contract
__device__ __forceinline__ bool allowed(const DetArgs &a, const DetItemD &D, int n_kept, int x, int y) {
    if (D.has_mask && D.mask[(int64_t)y * D.pitch + x] == 0) return false;
    const int32_t *kx = a.kept_xy + 2 * (int64_t)D.trk;
    for (int k = 0; k < n_kept; ++k)
        if (det_struck<false>(x, y, kx[2 * k], kx[2 * k + 1], a.d2)) return false;
    return true;
}

__global__ __launch_bounds__(NT) void k_detect_response(DetArgs a) {
    __shared__ int tile[TY + 4][TX + 4];
    __shared__ int pxx[TY + 2][TX + 2], pxy[TY + 2][TX + 2], pyy[TY + 2][TX + 2];
    const int item = blockIdx.z;
    if (item >= a.count) return;
    const DetItemD &D = a.items[item];
    if (!D.active || (int)blockIdx.x >= D.tiles) return;            // (the whole workgroup: no barrier was reached)
    const int w = D.w, h = D.h;
    const int x0 = ((int)blockIdx.x % D.tiles_x) * TX, y0 = ((int)blockIdx.x / D.tiles_x) * TY;
    const uint8_t *img = D.img;
    // the tile with a halo of 2, position (x0 - 2 + i, y0 - 2 + j) reflected into the image
    for (int id = threadIdx.x; id < (TX + 4) * (TY + 4); id += NT) {
        const int i = id % (TX + 4), j = id / (TX + 4);
        tile[j][i] = img[(int64_t)det_refl(y0 - 2 + j, h) * D.pitch + det_refl(x0 - 2 + i, w)];
    }
    __syncthreads();
    // the products at a halo of 1: position p outside the image is the product map's reflection, the gradient at q = refl(p), whose
    // own neighbourhood q - 1 .. q + 1 lies in the tile for every p in [-1, W]; positions past that are never summed
    for (int id = threadIdx.x; id < (TX + 2) * (TY + 2); id += NT) {
        const int i = id % (TX + 2), j = id / (TX + 2);
        const int px = x0 - 1 + i, py = y0 - 1 + j;
        int gx = 0, gy = 0;
        if (px <= w && py <= h) {
            const int c = det_refl(px, w) - (x0 - 2), r = det_refl(py, h) - (y0 - 2);
            int v[3][3];
#pragma unroll
            for (int dj = 0; dj < 3; ++dj)
#pragma unroll
                for (int di = 0; di < 3; ++di) v[dj][di] = tile[r - 1 + dj][c - 1 + di];
            det_sobel(v, gx, gy);
        }
        pxx[j][i] = gx * gx; pxy[j][i] = gx * gy; pyy[j][i] = gy * gy;
    }
    __syncthreads();
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int x = x0 + tx, y = y0 + ty;
    unsigned long long bits = 0ull;
    if (x < w && y < h) {
        int32_t sa = 0, sb = 0, sc = 0;
#pragma unroll
        for (int dj = 0; dj < 3; ++dj)
#pragma unroll
            for (int di = 0; di < 3; ++di) { sa += pxx[ty + dj][tx + di]; sb += pxy[ty + dj][tx + di]; sc += pyy[ty + dj][tx + di]; }
        const double R = det_response(sa, sb, sc);
        a.r[D.r + (int64_t)y * w + x] = R;
        if (allowed(a, D, a.res[item].n_kept, x, y)) bits = (unsigned long long)__double_as_longlong(R);
    }
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
        const unsigned long long o = __shfl_xor(bits, s, WAVE);
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && bits != 0ull) atomicMax(&a.res[item].maxbits, bits);
}

__global__ __launch_bounds__(NT) void k_detect_candidates(DetArgs a) {
    const int item = blockIdx.z;
    if (item >= a.count) return;
    const DetItemD &D = a.items[item];
    if (!D.active || (int)blockIdx.x >= D.tiles) return;
    const int w = D.w, h = D.h;
    const int x = ((int)blockIdx.x % D.tiles_x) * TX + (int)threadIdx.x % TX, y = ((int)blockIdx.x / D.tiles_x) * TY + (int)threadIdx.x / TX;
    if (x < 1 || y < 1 || x > w - 2 || y > h - 2) return;
    const double *R = a.r + D.r;
    const double t = __longlong_as_double((long long)a.res[item].maxbits) * a.quality;
    const int64_t p = (int64_t)y * w + x;
    const double v = R[p];
    if (!(v > t && v > 0.0)) return;
    bool top = true;
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
        for (int di = -1; di <= 1; ++di) top = top && v >= R[p + (int64_t)dj * w + di];
    if (!top || !allowed(a, D, a.res[item].n_kept, x, y)) return;
    const int slot = atomicAdd(&a.res[item].n_cand, 1);           // (below (w - 2) (h - 2), the list's size: a pixel arrives once)
    a.cand[D.cand + slot] = (uint32_t)p;
}

__global__ __launch_bounds__(NT_SEL) void k_detect_select(DetArgs a) {
    __shared__ DetKey slots[2 * (NT_SEL / WAVE)];
    const int item = blockIdx.x;
    if (item >= a.count) return;
    const DetItemD &D = a.items[item];
    if (!D.active) return;
    const int n = a.res[item].n_cand, n_want = D.max_total - a.res[item].n_kept;
    const int rounds = n_want < n ? n_want : n;
    if (rounds <= 0) return;                                        // (n_new stays 0)
    CandSrc src = {a.cand + D.cand, a.r + D.r, D.w};
    CandEmit emit = {a.new_pts + 2 * (int64_t)D.newp};
    const int n_new = greedy<NT_SEL, true>(src, n, rounds, a.d2, emit, slots);
    if (threadIdx.x == 0) a.res[item].n_new = n_new;
}

// The four launches of a call on q.  mask: some item has tracked points; tiles: some item has an image (max_tiles > 0).  between: three
// events recorded between the launches, or NULL.
inline void det_launch(const DetArgs &a, hipStream_t q, bool mask, bool tiles, int max_tiles, hipEvent_t *between) {
    const dim3 per_item((unsigned)a.count), per_tile((unsigned)max_tiles, 1, (unsigned)a.count);
    if (mask) hipLaunchKernelGGL(k_detect_setmask, per_item, dim3(NT_MASK), 0, q, a);
    if (between) (void)hipEventRecord(between[0], q);
    if (tiles) hipLaunchKernelGGL(k_detect_response, per_tile, dim3(NT), 0, q, a);
    if (between) (void)hipEventRecord(between[1], q);
    if (tiles) hipLaunchKernelGGL(k_detect_candidates, per_tile, dim3(NT), 0, q, a);
    if (between) (void)hipEventRecord(between[2], q);
    if (tiles) hipLaunchKernelGGL(k_detect_select, per_item, dim3(NT_SEL), 0, q, a);
}
