// Body of k_res_tail and k_res_tail_batch (vio_residuals.hip), included inside both kernels.  In scope: a (the window's ResArgs).
// A fragment for the reason vio_res_obs_body.inc gives.
    __shared__ double simu[NW];
    __shared__ double scol[P_N];
    __shared__ double sprior;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if (tid < NW) {
        const int k = tid;
        double chi = 0.0;
        if (!a.have_pre) chi = NAN;
        else if (a.pre_ok[k]) {
            const double *pre = a.pre + k * PRE_STRIDE;
            const double *pi = a.poses + 7 * k, *pj = pi + 7, *si = a.sb + 9 * k, *sj = si + 9;
            ImuCommon c;
            d_imu_common(pre, pi, si, pj, c);
            double r[15];
            d_imu_residual(pre, a.gravity, pi, si, pj, sj, c, r);
            for (int i = 0; i < 15; ++i) {                 // r^T Info r in the order of the solver's chi2 (d_backsub_imu_block)
                double t = 0;
                for (int j = 0; j < 15; ++j) t += pre[PRE_INFO + 15 * i + j] * r[j];
                chi += r[i] * t;
            }
        }
        simu[k] = chi;
    }
    for (int col = w; col < P_N; col += TAIL_NT / 64) {
        double s = 0.0;
        for (int b = lane; b < a.n_wg; b += 64) s += a.part[(size_t)b * P_STRIDE + col];
        s = d_wave_sum_to_lane63(s);
        if (lane == 63) scol[col] = s;
    }
    if (w == TAIL_NT / 64 - 1) {
        double s = 0.0;
        for (int i = lane; i < PRD; i += 64) s += a.errp[i] * a.errp[i];
        s = d_wave_sum_to_lane63(s);
        if (lane == 63) sprior = sqrt(s);
    }
    __syncthreads();
    if (tid == 0) {
        double imu = 0.0;
        for (int k = 0; k < NW; ++k) { imu += simu[k]; a.sum[S_IMUE + k] = simu[k]; }
        a.sum[S_VR] = scol[P_VR];
        a.sum[S_VP] = scol[P_VP];
        a.sum[S_IMU] = imu;
        a.sum[S_PRIOR] = sprior;
        a.sum[S_CHI] = 0.5 * (scol[P_VR] + (imu + sprior));         // vio_chi2: 0.5 * (visual + (imu + prior))
        for (int f = 0; f < NF; ++f) { a.sum[S_FR + f] = scol[P_FR + f]; a.sum[S_FE + f] = scol[P_FE + f]; }
        for (int k = 0; k < 3; ++k) a.sum[S_FL + k] = scol[P_FL + k];
    }
