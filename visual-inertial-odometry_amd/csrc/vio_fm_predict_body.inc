// vio_fm_predict_body.inc — the kernel of include/vio_fm_predict.h (DESIGN.md section 37), included behind vio_fm_outlier_body.inc; it
// uses vio_fm_body.inc's table, descriptors, scan and counts and vio_fm_predict_math.h's arithmetic.  One workgroup of FM_NT threads per
// item of the call, which is one slot's table:
//   k_fm_predict         predictPtsInNextFrame: threads 0 .. 10 turn the window's quaternions into matrices in LDS, thread 11 the
//                        extrinsic's, then thread 0 makes the next pose (the given one, or the constant-velocity one); the rows are
//                        walked in chunks of FM_NT, a row that qualifies (fmp_qualifies) is moved into the next camera, and the rows
//                        that qualify are written in list order: a ballot per wavefront, the wavefront counts through LDS (fm_scan).
// The table is only read.  Descriptor: a = frame_count, c = 1 where a next pose is given; payload: poses [11][7] | ext [7] |
// next_pose [7] (zeros where none).  Output: ids [n] | pts_cam [n][3] with n the slot's rows when the call began, which no compacted
// index reaches beyond.  No atomics, no floating-point sum across threads.
constexpr int FMP_IN = 7 * FM_MAX_OBS + 14;             // doubles of an item's payload

__global__ __launch_bounds__(FM_NT) void k_fm_predict(FmArgs a) {
    __shared__ double s_R[FM_MAX_OBS * 9], s_P[FM_MAX_OBS * 3], s_ric[9], s_tic[3], s_Rn[9], s_Pn[3];
    __shared__ int32_t s_w[FM_WAVES], s_cnt[2];
    const int item = blockIdx.x, t = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS), fc = fm_clamp(I.a, 0, FM_WINDOW);
    const double *poses = (const double *)(a.in + I.o_in), *ext = poses + 7 * FM_MAX_OBS, *next = ext + 7;
    vio_fm_result &R = a.res[item];
    if (t == 0) fm_result_clear(R);
    if (t < FM_MAX_OBS) {
        fmp_quat_to_R(poses + 7 * t + 3, s_R + 9 * t);
        for (int k = 0; k < 3; ++k) s_P[3 * t + k] = poses[7 * t + k];
    } else if (t == FM_MAX_OBS) {
        fmp_quat_to_R(ext + 3, s_ric);
        for (int k = 0; k < 3; ++k) s_tic[k] = ext[k];
    }
    __syncthreads();
    if (t == 0 && fc >= 2) {
        if (I.c) {
            fmp_quat_to_R(next + 3, s_Rn);
            for (int k = 0; k < 3; ++k) s_Pn[k] = next[k];
        } else {
            fmp_next_pose(s_R + 9 * (fc - 1), s_P + 3 * (fc - 1), s_R + 9 * fc, s_P + 3 * fc, s_Rn, s_Pn);
        }
    }
    __syncthreads();
    long long *o_id = (long long *)(a.out + I.o_out);
    double *o_pt = (double *)(o_id + n);
    int base = 0;
    if (fc >= 2) {                                          // (uniform)
        for (int c = 0; c * FM_NT < n; ++c) {
            const int r = c * FM_NT + t;
            int sf = 0, K = 0;
            double dep = 0.0;
            if (r < n) { sf = T.start[r]; K = fm_clamp(T.nobs[r], 0, FM_MAX_OBS); dep = T.depth[r]; }
            const bool take = r < n && fmp_qualifies(dep, K, sf, fc);
            int tot;
            const int dst = base + fm_scan(take, s_w, tot);
            if (take && dst < n) {                          // (sf is in [0, fc - 1] here)
                double p[3];
                fmp_point(T.ox[r], T.oy[r], dep, s_ric, s_tic, s_R + 9 * sf, s_P + 3 * sf, s_Rn, s_Pn, p);
                o_id[dst] = T.id[r];
                o_pt[3 * dst] = p[0]; o_pt[3 * dst + 1] = p[1]; o_pt[3 * dst + 2] = p[2];
            }
            base += tot;
        }
    }
    fm_counts(T, n, s_cnt, R);
    if (t == 0) R.n_rows = base;
}
