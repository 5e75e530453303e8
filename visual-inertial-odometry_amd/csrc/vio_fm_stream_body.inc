// vio_fm_stream_body.inc — the two kernels of include/vio_fm_stream.h (DESIGN.md section 32), included behind vio_fm_body.inc, whose
// table, descriptors, scans and counts they use.  One workgroup per item of the call, which is one slot's table:
//   k_fm_init_depth      visualInitialAlign's depth hand-over: every usable row is triangulated anew on the item's poses, whatever
//                        depth it held, and stores depth * s.  Shaped as k_fm_export is (FM_EXPORT_NT threads, the camera poses staged
//                        in LDS by the same lines, the same call of d_triangulate_track), so that the depth in front of the product is
//                        the export kernel's bit for bit.  No device-checked rule, no output arrays: the read-back is the result.
//   k_fm_tracks          the slot's list as arrays: an integer scan of n_obs over the rows gives each row's offset and the total, the
//                        capacities are checked against it, a barrier, then thread r copies row r.  Integers and copies only.
// Every count read from device memory is held to the rows there are before it indexes anything; a row is written only below the
// capacities the host sized the read-back by.

// the payload of an init_depth item: poses [11][7] | ext [7] | s
constexpr int FM_INIT_S = 7 * VIO_NF + 7;

__global__ __launch_bounds__(FM_EXPORT_NT) void k_fm_init_depth(FmArgs a) {
    __shared__ double sRc[VIO_NF * 9], sTc[VIO_NF * 3];
    __shared__ int32_t s_cnt[2], s_tri;
    const int item = blockIdx.x, tid = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS);
    const double *poses = (const double *)(a.in + I.o_in), *ext = poses + 7 * VIO_NF;
    const double s = poses[FM_INIT_S];
    vio_fm_result &R = a.res[item];
    if (tid == 0) { fm_result_clear(R); s_tri = 0; }
    if (tid < VIO_NF) {                                     // the camera poses, as k_fm_export stages them
        double Rf[9], ric[9], tic[3], tt[3];
        d_quat_to_R(poses + 7 * tid + 3, Rf);
        d_quat_to_R(ext + 3, ric);
        for (int k = 0; k < 3; ++k) tic[k] = ext[k];
        d_m3_mul(Rf, ric, sRc + 9 * tid);
        d_m3_vec(Rf, tic, tt);
        for (int k = 0; k < 3; ++k) sTc[3 * tid + k] = poses[7 * tid + k] + tt[k];
    }
    __syncthreads();
    for (int c = 0; c * FM_EXPORT_NT < n; ++c) {            // (a thread writes its own rows only)
        const int r = c * FM_EXPORT_NT + tid;
        int sf = 0, K = 0;
        if (r < n) { sf = T.start[r]; K = fm_clamp(T.nobs[r], 0, FM_MAX_OBS); }
        const bool us = r < n && fm_usable(sf, K) && sf >= 0;
        if (us) {                                           // estimator.cpp:406-409: the depth it held is not read
            const double dep = d_triangulate_track(sRc, sTc, sf, K, [&](int j, double &x, double &y) { x = T.ox[j * FM_T + r]; y = T.oy[j * FM_T + r]; },
                                                   a.init_depth);
            T.depth[r] = dep * s;                           // :441, one product
            atomicAdd(&s_tri, 1);
        }
    }
    fm_counts(T, n, s_cnt, R);
    if (tid == 0) R.n_triangulated = s_tri;
}

// the arrays of a tracks item in the call's read-back, for nt rows and no observations: ids | depth | off (nt + 1) | pts | start | flag
__host__ __device__ inline size_t fm_tracks_bytes(size_t nt, size_t no) { return 8 * (3 * nt + 1 + 2 * no) + 8 * nt; }

__global__ __launch_bounds__(FM_NT) void k_fm_tracks(FmArgs a) {
    __shared__ int32_t s_w[FM_WAVES], s_cnt[2];
    const int item = blockIdx.x, t = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS);
    const int cap_t = fm_clamp(I.b, 0, FM_MAX_TRACKS), cap_o = fm_clamp(I.c, 0, FM_MAX_TRACKS * FM_MAX_OBS);
    const int nt = n < cap_t ? n : cap_t, no = n * FM_MAX_OBS < cap_o ? n * FM_MAX_OBS : cap_o;      // (the host's layout)
    vio_fm_result &R = a.res[item];
    if (t == 0) fm_result_clear(R);
    // pass 1: every row's offset and the total
    int off_r[FM_CHUNKS], k_r[FM_CHUNKS];
    int total = 0;
#pragma unroll
    for (int c = 0; c < FM_CHUNKS; ++c) {
        const int r = c * FM_NT + t;
        k_r[c] = r < n ? fm_clamp(T.nobs[r], 0, FM_MAX_OBS) : 0;
        int tot;
        off_r[c] = total + fm_scan_int(k_r[c], s_w, tot);
        total += tot;
    }
    const bool fits = n <= cap_t && total <= cap_o;         // (uniform)
    __syncthreads();
    // pass 2: thread r copies row r
    if (fits) {
        char *o = a.out + I.o_out;
        long long *o_id = (long long *)o;
        double *o_depth = (double *)(o_id + nt);
        long long *o_off = (long long *)(o_depth + nt);
        double *o_pts = (double *)(o_off + nt + 1);
        int32_t *o_start = (int32_t *)(o_pts + 2 * (size_t)no), *o_flag = o_start + nt;
        if (t == 0) o_off[0] = 0;
#pragma unroll
        for (int c = 0; c < FM_CHUNKS; ++c) {
            const int r = c * FM_NT + t;
            if (r >= n) continue;
            o_id[r] = T.id[r]; o_depth[r] = T.depth[r]; o_start[r] = T.start[r]; o_flag[r] = T.flag[r];
            o_off[r + 1] = off_r[c] + k_r[c];
            for (int j = 0; j < k_r[c]; ++j) {
                const int e = off_r[c] + j;
                o_pts[2 * e] = T.ox[j * FM_T + r]; o_pts[2 * e + 1] = T.oy[j * FM_T + r];
            }
        }
    }
    fm_counts(T, n, s_cnt, R);
    if (t == 0) { R.n_rows = total; if (!fits) R.status = VIO_FM_STATUS_CAPACITY; }
}
