// vio_clahe_body.inc — the two CLAHE kernels and their launches, the one copy libvio_clahe_hip (vio_clahe.hip, at file scope)
// and libvio_frame_hip (vio_frame.hip, inside a namespace of its own) compile (DESIGN.md sections 22 and 23).  The including file has
// included <hip/hip_runtime.h>, <cstdint>, vio_clahe_math.h and vio_clahe_host.h (the descriptor tables, TX, TY and PX), and has
// contraction off: a fused multiply-add in the blend changes output bytes.
//
//   k_clahe_lut      one 256-thread workgroup per (tile, image).  The tile's histogram in LDS with integer atomicAdd, one private copy
//                    per wavefront (a flat tile puts every pixel in one bin), the source read through the reflection where the image
//                    was extended.  Then thread b owns bin b: the merged count, the clip, the tile's excess by a butterfly across the
//                    wave and one LDS slot per wave, the closed form of the redistribution, an inclusive scan (wave scan plus the
//                    waves' offsets), and the LUT byte to global memory.
//   k_clahe_apply    a TX x TY block of pixels per workgroup, every image of the call in the grid (blockIdx.z).  Four pixels per
//                    thread and pass, one 4-byte load and one 4-byte store (source and result are 4-byte aligned and have a pitch that
//                    is a multiple of 4, so every row is aligned); the four look-ups per pixel are byte gathers indexed by the pixel's
//                    value, out of LDS: the LUTs of the tiles the block of pixels can touch (a contiguous range in x and in y, known
//                    from the block's corners since the tile index is monotone in the position) are copied there first.  Gathering
//                    from global memory instead was measured and is slower (DESIGN.md section 22).
// An item names its source and its result by address, so the two need not lie in one buffer each: the resident library equalises out
// of its upload buffer straight into a frame's level 0.
constexpr int WAVE = 64;
constexpr int BINS = VIO_CLAHE_BINS;
constexpr int NT = 256;                 // threads of both kernels
constexpr int NW = NT / WAVE;
constexpr int ROWS = NT / (TX / PX);    // rows of a pass
static_assert(NT == BINS, "k_clahe_lut: thread b owns bin b");
static_assert(TX % PX == 0 && NT % (TX / PX) == 0 && TY % ROWS == 0, "k_clahe_apply: whole passes over the block of pixels");

__global__ __launch_bounds__(NT) void k_clahe_lut(ClaheArgs a) {
    __shared__ int32_t hist[NW][BINS];
    __shared__ int32_t slot[2][NW];
    const int item = blockIdx.z, tile = blockIdx.x;
    if (item >= a.count || tile >= a.tiles_x * a.tiles_y) return;      // (the whole workgroup: no barrier was reached)
    const ClaheItemD &D = a.items[item];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
#pragma unroll
    for (int k = 0; k < NW; ++k) hist[k][tid] = 0;
    __syncthreads();
    const int w = D.w, h = D.h, tile_w = D.tile_w, area = D.area;
    const int x0 = (tile % a.tiles_x) * tile_w, y0 = (tile / a.tiles_x) * D.tile_h;
    const uint8_t *img = D.src;
    // pixel i of the tile, row by row, belongs to thread i mod NT; (tx, ty) follows i without a division per pixel
    int tx = tid % tile_w, ty = tid / tile_w;
    const int step_x = NT % tile_w, step_y = NT / tile_w;
    for (int i = tid; i < area; i += NT) {
        int x = x0 + tx, y = y0 + ty;
        if (D.ext) {                                                    // (positions past the image exist only in the extended one)
            if (x >= w) x = clahe_refl(x, w);
            if (y >= h) y = clahe_refl(y, h);
        }
        atomicAdd(&hist[wv][img[(int64_t)y * D.pitch + x]], 1);
        tx += step_x; ty += step_y;
        if (tx >= tile_w) { tx -= tile_w; ty += 1; }
    }
    __syncthreads();
    int32_t v = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) v += hist[k][tid];
    if (D.clip > 0) {                                                   // (the same in every thread)
        int32_t excess = v > D.clip ? v - D.clip : 0;
#pragma unroll
        for (int s = 1; s < WAVE; s <<= 1) excess += __shfl_xor(excess, s, WAVE);
        if (lane == 0) slot[0][wv] = excess;
        __syncthreads();
        excess = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) excess += slot[0][k];
        v = clahe_redistribute(v, tid, D.clip, excess);
    }
    int32_t sum = v;
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
        const int32_t o = __shfl_up(sum, s, WAVE);
        if (lane >= s) sum += o;
    }
    if (lane == WAVE - 1) slot[1][wv] = sum;
    __syncthreads();
    for (int k = 0; k < wv; ++k) sum += slot[1][k];
    a.luts[((int64_t)item * (a.tiles_x * a.tiles_y) + tile) * BINS + tid] = clahe_lut_value(sum, D.lut_scale);
}

__global__ __launch_bounds__(NT) void k_clahe_apply(ClaheArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];                      // tiles_y * tiles_x * 256 bytes: room for every LUT of an image
    const int item = blockIdx.z;
    if (item >= a.count) return;
    const ClaheItemD &D = a.items[item];
    if ((int)blockIdx.x >= D.ptiles) return;                            // (the whole workgroup: no barrier was reached)
    const int w = D.w, h = D.h, tid = threadIdx.x;
    const int px0 = ((int)blockIdx.x % D.ptiles_x) * TX, py0 = ((int)blockIdx.x / D.ptiles_x) * TY;
    const uint8_t *glut = a.luts + (int64_t)item * (a.tiles_x * a.tiles_y) * BINS;
    // the tiles of the block's first and last pixel bound those of every pixel between them
    int tx_lo, ty_lo, tx_hi, ty_hi, t1, t2;
    float f0, f1;
    clahe_axis(px0, D.inv_tile_w, a.tiles_x, tx_lo, t2, f0, f1);
    clahe_axis((px0 + TX < w ? px0 + TX : w) - 1, D.inv_tile_w, a.tiles_x, t1, tx_hi, f0, f1);
    clahe_axis(py0, D.inv_tile_h, a.tiles_y, ty_lo, t2, f0, f1);
    clahe_axis((py0 + TY < h ? py0 + TY : h) - 1, D.inv_tile_h, a.tiles_y, t1, ty_hi, f0, f1);
    const int nx = tx_hi - tx_lo + 1, ny = ty_hi - ty_lo + 1;
    const int per = nx * (BINS / 16);                                   // a row of tiles is nx * 256 contiguous bytes: 16-byte pieces
    for (int id = tid; id < ny * per; id += NT) {
        const int j = id / per, k = id - j * per;
        ((uint4 *)lds)[id] = ((const uint4 *)(glut + (int64_t)((ty_lo + j) * a.tiles_x + tx_lo) * BINS))[k];
    }
    __syncthreads();
    // entry v of tile (ty, tx) in the staged range
    auto lut = [&](int ty, int tx, int v) -> uint8_t { return lds[((ty - ty_lo) * nx + (tx - tx_lo)) * BINS + v]; };
    const int gx = tid % (TX / PX), gy = tid / (TX / PX);
#pragma unroll
    for (int pass = 0; pass < TY / ROWS; ++pass) {
        const int x = px0 + gx * PX, y = py0 + pass * ROWS + gy;
        if (x >= w || y >= h) continue;
        int ty1, ty2;
        float ya, ya1;
        clahe_axis(y, D.inv_tile_h, a.tiles_y, ty1, ty2, ya, ya1);
        const int64_t at = (int64_t)y * D.pitch + x;                    // (a multiple of 4)
        const uint32_t in4 = *(const uint32_t *)(D.src + at);
        uint32_t out4 = 0;
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            if (x + k >= w) continue;                                   // (the row's padding stays 0)
            int tx1, tx2;
            float xa, xa1;
            clahe_axis(x + k, D.inv_tile_w, a.tiles_x, tx1, tx2, xa, xa1);
            const int v = (int)((in4 >> (8 * k)) & 255u);
            const uint8_t o = clahe_blend(lut(ty1, tx1, v), lut(ty1, tx2, v), lut(ty2, tx1, v), lut(ty2, tx2, v), xa, xa1, ya, ya1);
            out4 |= (uint32_t)o << (8 * k);
        }
        *(uint32_t *)(D.dst + at) = out4;
    }
}

// k_clahe_apply stages the LUTs of up to 16 x 16 tiles, 64 KB; a launch that asks for more than the kernel may have fails and is
// reported.  Once per process and device, from a library's create.
inline void clahe_allow_lds() {
    (void)hipFuncSetAttribute((const void *)k_clahe_apply, hipFuncAttributeMaxDynamicSharedMemorySize, VIO_CLAHE_MAX_TILES * VIO_CLAHE_MAX_TILES * BINS);
    (void)hipGetLastError();
}

// the two launches of a call on q; between: an event recorded between them, or NULL
inline void clahe_launch(hipStream_t q, const ClaheArgs &a, int max_ptiles, hipEvent_t between) {
    const int tiles = a.tiles_x * a.tiles_y;
    hipLaunchKernelGGL(k_clahe_lut, dim3((unsigned)tiles, 1, (unsigned)a.count), dim3(NT), 0, q, a);
    if (between) (void)hipEventRecord(between, q);
    hipLaunchKernelGGL(k_clahe_apply, dim3((unsigned)max_ptiles, 1, (unsigned)a.count), dim3(NT), (size_t)tiles * BINS, q, a);
}
