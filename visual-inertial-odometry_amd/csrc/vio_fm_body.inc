// vio_fm_body.inc — the kernels of the batched FeatureManager (include/vio_fm.h, DESIGN.md section 26).  One workgroup per item of the
// call (blockIdx.x), which is one slot's table:
//   k_fm_add             addFeatureCheckParallax: rank the incoming ids in LDS, look the table's ids up among them, check, append
//                        observations and rows, then the parallax sum in the header's order and the keyframe decision
//   k_fm_slide           the three slide rules as one row transform (vio_fm_math.h) and a stable compaction
//   k_fm_set_depth       setDepth / clearDepth over the usable rows' scan, then removeFailures as a compaction
//   k_fm_export          triangulate (vio_triangulate_body.h: the text k_triangulate includes), getDepthVector and the edge loop
//   k_fm_corresponding   getCorresponding as a compaction into the output rows
// A slot's table is a structure of arrays over FM_MAX_TRACKS rows, the observations frame-major (observation j of row r at
// [j][r]), so a thread per row reads coalesced.  The kernels of FM_NT = 1024 threads walk the rows in chunks of FM_NT.
// A compaction is stable and in place: per chunk every thread loads its whole row into registers, the scan's barriers stand between
// those loads and any store, and a row only ever moves to a lower index, so a chunk's stores land in rows whose loads are done (its
// own chunk's and the chunks' before it) and never in a chunk not yet read.  A ballot per wavefront, the wavefront counts through
// LDS, every thread adds the counts before its own (fm_scan; the arithmetic is csrc/vio_fm_math.h's).  No floating-point atomics;
// the only atomics are integer counts and flag bits in LDS, where no order matters.  Every count a kernel reads from device memory
// is held to the rows there are before it indexes anything.
constexpr int FM_EXPORT_NT = 256;
constexpr int64_t FM_T = FM_MAX_TRACKS;
constexpr size_t FM_TAB_BYTES = (size_t)FM_T * (8 + 8 + 2 * 8 * FM_MAX_OBS + 3 * 4);

struct FmTab {
    long long *id;                      // [FM_T]
    double *depth;                      // [FM_T]
    double *ox, *oy;                    // [FM_MAX_OBS][FM_T]
    int32_t *start, *nobs, *flag;       // [FM_T]
};

__host__ __device__ inline FmTab fm_tab(char *b) {
    FmTab T;
    T.id = (long long *)b;
    T.depth = (double *)(b + 8 * FM_T);
    T.ox = T.depth + FM_T;
    T.oy = T.ox + FM_MAX_OBS * FM_T;
    T.start = (int32_t *)(T.oy + FM_MAX_OBS * FM_T);
    T.nobs = T.start + FM_T;
    T.flag = T.nobs + FM_T;
    return T;
}

struct FmItemD {
    char *tab;                          // the slot's table
    int32_t n_tracks;                   // its rows when the call began (the host's mirror)
    int32_t a, b, c;                    // add: frame_count, n | set_depth: mode, remove_failures, n | slide: kind, frame_count |
                                        // export: triangulate, rows of the landmark arrays, of the edge arrays | corresponding: l, r, rows
    int64_t o_in;                       // the item's payload in the call's upload, in bytes
    int64_t o_out;                      // the item's arrays in the call's read-back, in bytes
};

struct FmArgs {
    const FmItemD *items;
    const char *in;
    char *out;
    vio_fm_result *res;
    double init_depth, min_parallax;
};

// one row in registers; every index is a compile-time constant after unrolling
struct FmRow {
    long long id;
    double depth;
    int32_t start, nobs, flag;
    double x[FM_MAX_OBS], y[FM_MAX_OBS];
};

__device__ __forceinline__ void fm_row_load(const FmTab &T, int r, FmRow &R) {
    R.id = T.id[r]; R.depth = T.depth[r]; R.start = T.start[r]; R.flag = T.flag[r];
    R.nobs = fm_clamp(T.nobs[r], 0, FM_MAX_OBS);
#pragma unroll
    for (int j = 0; j < FM_MAX_OBS; ++j) {
        R.x[j] = 0.0; R.y[j] = 0.0;
        if (j < R.nobs) { R.x[j] = T.ox[j * FM_T + r]; R.y[j] = T.oy[j * FM_T + r]; }
    }
}

__device__ __forceinline__ void fm_row_store(const FmTab &T, int r, const FmRow &R) {
    T.id[r] = R.id; T.depth[r] = R.depth; T.start[r] = R.start; T.flag[r] = R.flag; T.nobs[r] = R.nobs;
#pragma unroll
    for (int j = 0; j < FM_MAX_OBS; ++j)
        if (j < R.nobs) { T.ox[j * FM_T + r] = R.x[j]; T.oy[j * FM_T + r] = R.y[j]; }
}

// the exclusive prefix of `keep` over the workgroup's threads, and their total; every thread of the workgroup calls it
__device__ __forceinline__ int fm_scan(bool keep, int32_t *s_w, int &total) {
    const int lane = threadIdx.x & (FM_WAVE - 1), wv = threadIdx.x / FM_WAVE;
    const uint64_t b = __ballot(keep);
    __syncthreads();                                        // (the scan before has been read)
    if (lane == 0) s_w[wv] = fm_wave_count(b);
    __syncthreads();
    total = fm_wave_base(s_w, (int)blockDim.x / FM_WAVE);
    return fm_dest(0, s_w, wv, b, lane);
}

// ... of a count per thread
__device__ __forceinline__ int fm_scan_int(int v, int32_t *s_w, int &total) {
    const int lane = threadIdx.x & (FM_WAVE - 1), wv = threadIdx.x / FM_WAVE;
    int inc = v;
#pragma unroll
    for (int d = 1; d < FM_WAVE; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();
    if (lane == FM_WAVE - 1) s_w[wv] = inc;
    __syncthreads();
    total = fm_wave_base(s_w, (int)blockDim.x / FM_WAVE);
    return fm_wave_base(s_w, wv) + inc - v;
}

// the slot's counts over its n rows as they are now, into the result; every thread calls it (integer sums: no order)
__device__ __forceinline__ void fm_counts(const FmTab &T, int n, int32_t *s_cnt, vio_fm_result &R) {
    __syncthreads();                                        // (the rows are written; s_cnt is free)
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int nl = 0, no = 0;
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        const int s = T.start[r], k = fm_clamp(T.nobs[r], 0, FM_MAX_OBS);
        if (fm_usable(s, k)) { nl += 1; no += k - 1; }
    }
    if (nl) { atomicAdd(&s_cnt[0], nl); atomicAdd(&s_cnt[1], no); }
    __syncthreads();
    if (threadIdx.x == 0) { R.n_tracks = n; R.n_landmarks = s_cnt[0]; R.n_observations = s_cnt[1]; }
}

__device__ __forceinline__ void fm_result_clear(vio_fm_result &R) {
    R.status = VIO_FM_STATUS_OK; R.n_tracks = 0; R.n_landmarks = 0; R.n_observations = 0; R.keyframe = 0; R.last_track_num = 0;
    R.parallax_num = 0; R.n_new = 0; R.n_triangulated = 0; R.n_rows = 0; R.parallax_sum = 0.0;
}

__global__ __launch_bounds__(FM_NT) void k_fm_add(FmArgs a) {
    __shared__ long long s_id[FM_MAX_POINTS], s_sid[FM_MAX_POINTS];
    __shared__ int32_t s_src[FM_MAX_POINTS], s_match[FM_MAX_POINTS];
    __shared__ double s_red[FM_NT];
    __shared__ int32_t s_w[FM_WAVES], s_cnt[2], s_err, s_num;
    const int item = blockIdx.x, t = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n0 = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS), fc = fm_clamp(I.a, 0, FM_WINDOW), n = fm_clamp(I.b, 0, FM_MAX_POINTS);
    const long long *ids = (const long long *)(a.in + I.o_in);
    const double *pts = (const double *)(ids + n);
    vio_fm_result &R = a.res[item];
    if (t == 0) { fm_result_clear(R); s_err = 0; s_num = 0; }
    if (t < n) s_id[t] = ids[t];
    s_match[t] = -1;
    __syncthreads();
    // the incoming ids in ascending order, as the reference's std::map iterates: the ids are distinct, so the ranks are a permutation
    if (t < n) {
        const long long my = s_id[t];
        int rank = 0;
        for (int u = 0; u < n; ++u) rank += s_id[u] < my;
        s_sid[rank] = my;
        s_src[rank] = t;
    }
    __syncthreads();
    // every row of the table looks its id up among them (the table's ids are distinct: each incoming id meets at most one row, in
    // whatever order the table holds them)
    for (int r = t; r < n0; r += FM_NT) {
        const long long id = T.id[r];
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_sid[mid] < id) lo = mid + 1; else hi = mid;
        }
        if (lo < n && s_sid[lo] == id) s_match[lo] = r;
    }
    __syncthreads();
    // check phase: nothing is written before every rule holds
    const int m = t < n ? s_match[t] : -1;
    int k_obs = 0;
    if (m >= 0) {
        k_obs = fm_clamp(T.nobs[m], 0, FM_MAX_OBS);
        if (k_obs >= FM_MAX_OBS) atomicOr(&s_err, 4);
        else if (T.start[m] + k_obs != fc) atomicOr(&s_err, 2);
    }
    int n_matched, n_new;
    (void)fm_scan(m >= 0, s_w, n_matched);
    const int rank_new = fm_scan(t < n && m < 0, s_w, n_new);
    if (t == 0 && n0 + n_new > FM_MAX_TRACKS) atomicOr(&s_err, 1);
    __syncthreads();
    const int err = s_err;
    if (err) {                                              // (uniform: the slot is as it was)
        if (t == 0) R.status = (err & 1) ? VIO_FM_STATUS_TABLE_FULL : ((err & 4) ? VIO_FM_STATUS_OBS_FULL : VIO_FM_STATUS_GAP);
        fm_counts(T, n0, s_cnt, R);
        return;
    }
    // write phase
    if (t < n) {
        const int src = s_src[t];
        const double x = pts[2 * src], y = pts[2 * src + 1];
        if (m >= 0) {
            T.ox[k_obs * FM_T + m] = x; T.oy[k_obs * FM_T + m] = y;
            T.nobs[m] = k_obs + 1;
        } else {
            const int r = n0 + rank_new;
            T.id[r] = s_sid[t]; T.depth[r] = -1.0; T.start[r] = fc; T.nobs[r] = 1; T.flag[r] = 0;
            T.ox[r] = x; T.oy[r] = y;
        }
    }
    const int n1 = n0 + n_new;
    __syncthreads();
    // the parallax of the second and third last frames, summed in the order include/vio_fm.h writes down
    int keyframe = 1;
    double sum = 0.0;
    if (!(fc < 2 || n_matched < 20)) {                     // (uniform)
        double part = 0.0;
        int num = 0;
        for (int r = t; r < n1; r += FM_NT) {
            const int s = T.start[r], k = fm_clamp(T.nobs[r], 0, FM_MAX_OBS);
            if (s >= 0 && fm_parallax_row(fc, s, k)) {
                const int i = fc - 2 - s, j = fc - 1 - s;
                part = part + fm_parallax(T.ox[i * FM_T + r], T.oy[i * FM_T + r], T.ox[j * FM_T + r], T.oy[j * FM_T + r]);
                num += 1;
            }
        }
        s_red[t] = part;
        if (num) atomicAdd(&s_num, num);
        __syncthreads();
        for (int w = FM_NT / 2; w >= 1; w >>= 1) {
            if (t < w) s_red[t] = s_red[t] + s_red[t + w];
            __syncthreads();
        }
        sum = s_red[0];
        const int pn = s_num;
        keyframe = pn == 0 ? 1 : (sum / pn >= a.min_parallax);
        if (t == 0) { R.parallax_num = pn; R.parallax_sum = pn == 0 ? 0.0 : sum; }
    }
    if (t == 0) { R.keyframe = keyframe; R.last_track_num = n_matched; R.n_new = n_new; }
    fm_counts(T, n1, s_cnt, R);
}

__global__ __launch_bounds__(FM_NT) void k_fm_slide(FmArgs a) {
    __shared__ int32_t s_w[FM_WAVES], s_cnt[2];
    __shared__ double s_m[24];
    const int item = blockIdx.x, t = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS), kind = I.a, fc = I.b;
    vio_fm_result &R = a.res[item];
    if (t == 0) fm_result_clear(R);
    if (t < 24) s_m[t] = kind == FM_BACK_SHIFT_DEPTH ? ((const double *)(a.in + I.o_in))[t] : 0.0;      // marg_R | marg_P | new_R | new_P
    __syncthreads();
    int base = 0;
    for (int c = 0; c * FM_NT < n; ++c) {
        const int r = c * FM_NT + t;
        FmRow W;
        bool keep = false;
        if (r < n) {
            fm_row_load(T, r, W);
            const FmSlide s = fm_slide_row(kind, fc, W.start, W.nobs);
            keep = s.keep != 0;
            if (s.shift) W.depth = fm_shift_depth(W.x[0], W.y[0], W.depth, s_m, s_m + 9, s_m + 12, s_m + 21, a.init_depth);
            W.start = s.start;
            if (s.erase >= 0) {
#pragma unroll
                for (int j = 0; j < FM_MAX_OBS - 1; ++j)
                    if (j >= s.erase) { W.x[j] = W.x[j + 1]; W.y[j] = W.y[j + 1]; }
                W.nobs -= 1;
            }
        }
        int tot;
        const int dst = base + fm_scan(keep, s_w, tot);    // (its barriers: every load of the chunk before any store)
        if (keep) fm_row_store(T, dst, W);
        base += tot;
    }
    fm_counts(T, base, s_cnt, R);
}

__global__ __launch_bounds__(FM_NT) void k_fm_set_depth(FmArgs a) {
    __shared__ int32_t s_w[FM_WAVES], s_cnt[2];
    const int item = blockIdx.x, t = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS), mode = I.a, remove = I.b, nx = fm_clamp(I.c, 0, FM_MAX_TRACKS);
    const double *x = (const double *)(a.in + I.o_in);
    vio_fm_result &R = a.res[item];
    if (t == 0) fm_result_clear(R);
    int base = 0;
    for (int c = 0; c * FM_NT < n; ++c) {                   // (a thread writes its own rows only)
        const int r = c * FM_NT + t;
        const bool us = r < n && fm_usable(T.start[r], fm_clamp(T.nobs[r], 0, FM_MAX_OBS));
        int tot;
        const int k = base + fm_scan(us, s_w, tot);
        if (us && k < nx) {
            const double d = 1.0 / x[k];
            T.depth[r] = d;
            if (mode == VIO_FM_DEPTH_SET) T.flag[r] = d < 0 ? 2 : 1;
        }
        base += tot;
    }
    int n1 = n;
    if (remove) {                                           // removeFailures (uniform)
        n1 = 0;
        for (int c = 0; c * FM_NT < n; ++c) {
            const int r = c * FM_NT + t;
            FmRow W;
            bool keep = false;
            if (r < n) {
                fm_row_load(T, r, W);                       // (the thread's own writes above)
                keep = W.flag != 2;
            }
            int tot;
            const int dst = n1 + fm_scan(keep, s_w, tot);
            if (keep && dst != r) fm_row_store(T, dst, W);
            n1 += tot;
        }
    }
    fm_counts(T, n1, s_cnt, R);
}

__global__ __launch_bounds__(FM_EXPORT_NT) void k_fm_export(FmArgs a) {
    __shared__ double sRc[VIO_NF * 9], sTc[VIO_NF * 3];
    __shared__ int32_t s_w[FM_EXPORT_NT / FM_WAVE], s_cnt[2], s_tri;
    const int item = blockIdx.x, tid = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS), tri = I.a;
    const int64_t cap_l = fm_clamp(I.b, 0, FM_MAX_TRACKS), cap_o = fm_clamp(I.c, 0, FM_MAX_TRACKS * (FM_MAX_OBS - 1));
    const double *poses = (const double *)(a.in + I.o_in), *ext = poses + 7 * VIO_NF;
    vio_fm_result &R = a.res[item];
    if (tid == 0) { fm_result_clear(R); s_tri = 0; }
    if (tid < VIO_NF) {                                     // the camera poses, as k_triangulate stages them
        double Rf[9], ric[9], tic[3], tt[3];
        d_quat_to_R(poses + 7 * tid + 3, Rf);
        d_quat_to_R(ext + 3, ric);
        for (int k = 0; k < 3; ++k) tic[k] = ext[k];
        d_m3_mul(Rf, ric, sRc + 9 * tid);
        d_m3_vec(Rf, tic, tt);
        for (int k = 0; k < 3; ++k) sTc[3 * tid + k] = poses[7 * tid + k] + tt[k];
    }
    __syncthreads();
    char *o = a.out + I.o_out;
    long long *o_id = (long long *)o;
    double *o_inv = (double *)(o_id + cap_l), *o_pi = o_inv + cap_l, *o_pj = o_pi + 2 * cap_o;
    int32_t *o_lm = (int32_t *)(o_pj + 2 * cap_o), *o_host = o_lm + cap_o, *o_target = o_host + cap_o;
    int base_l = 0, base_o = 0;
    for (int c = 0; c * FM_EXPORT_NT < n; ++c) {
        const int r = c * FM_EXPORT_NT + tid;
        int sf = 0, K = 0;
        if (r < n) { sf = T.start[r]; K = fm_clamp(T.nobs[r], 0, FM_MAX_OBS); }
        const bool us = r < n && fm_usable(sf, K) && sf >= 0;
        int tot_l, tot_o;
        const int k = base_l + fm_scan(us, s_w, tot_l);
        const int e0 = base_o + fm_scan_int(us ? K - 1 : 0, s_w, tot_o);
        if (us) {
            double dep = T.depth[r];
            if (tri && !(dep > 0)) {                        // feature_manager.cpp:210
                dep = d_triangulate_track(sRc, sTc, sf, K, [&](int j, double &x, double &y) { x = T.ox[j * FM_T + r]; y = T.oy[j * FM_T + r]; },
                                          a.init_depth);
                T.depth[r] = dep;
                atomicAdd(&s_tri, 1);
            }
            if (k < cap_l) { o_id[k] = T.id[r]; o_inv[k] = 1.0 / dep; }
            const double xi = T.ox[r], yi = T.oy[r];
            for (int j = 1; j < K; ++j) {                   // estimator.cpp:995-1013, imu_j = imu_i skipped
                const int64_t e = e0 + j - 1;
                if (e >= cap_o) break;
                o_lm[e] = k; o_host[e] = sf; o_target[e] = sf + j;
                o_pi[2 * e] = xi; o_pi[2 * e + 1] = yi;
                o_pj[2 * e] = T.ox[j * FM_T + r]; o_pj[2 * e + 1] = T.oy[j * FM_T + r];
            }
        }
        base_l += tot_l; base_o += tot_o;
    }
    fm_counts(T, n, s_cnt, R);
    if (tid == 0) R.n_triangulated = s_tri;
}

__global__ __launch_bounds__(FM_NT) void k_fm_corresponding(FmArgs a) {
    __shared__ int32_t s_w[FM_WAVES], s_cnt[2];
    const int item = blockIdx.x, t = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS), l = fm_clamp(I.a, 0, FM_WINDOW), rr = fm_clamp(I.b, l, FM_WINDOW);
    const int cap = fm_clamp(I.c, 0, FM_MAX_TRACKS);
    double *rows = (double *)(a.out + I.o_out);
    vio_fm_result &R = a.res[item];
    if (t == 0) fm_result_clear(R);
    int base = 0;
    for (int c = 0; c * FM_NT < n; ++c) {
        const int r = c * FM_NT + t;
        int sf = 0, K = 0;
        if (r < n) { sf = T.start[r]; K = fm_clamp(T.nobs[r], 0, FM_MAX_OBS); }
        const bool keep = r < n && sf >= 0 && sf <= l && sf + K - 1 >= rr;      // :125
        int tot;
        const int dst = base + fm_scan(keep, s_w, tot);
        if (keep && dst < cap) {
            const int il = l - sf, ir = rr - sf;
            rows[4 * dst] = T.ox[il * FM_T + r]; rows[4 * dst + 1] = T.oy[il * FM_T + r];
            rows[4 * dst + 2] = T.ox[ir * FM_T + r]; rows[4 * dst + 3] = T.oy[ir * FM_T + r];
        }
        base += tot;
    }
    fm_counts(T, n, s_cnt, R);
    if (t == 0) R.n_rows = base < cap ? base : cap;
}
