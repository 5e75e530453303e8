// Body of k_res_lm<D> and k_res_lm_batch<D> (vio_residuals.hip), included inside both kernels.  In scope: D, a (the window's
// ResArgs), blk (the workgroup's index within the window; its partials go to row blk of a.part).  A fragment for the reason
// vio_res_obs_body.inc gives.
    __shared__ double red[P_N * (LM_NT / 64)];
    const int tid = threadIdx.x;
    const int l = blk * LM_NT + tid;
    double vr = 0.0, vp = 0.0, fr[NF], fe[NF], fl[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int f = 0; f < NF; ++f) { fr[f] = 0.0; fe[f] = 0.0; }
    if (l < a.n) {
        double spx = 0.0, mpx = 0.0, srho = 0.0;
        unsigned flag = 0;
        const int q0 = a.off[l], q1 = a.off[l + 1];
        for (int q = q0; q < q1; ++q) {
            const int e = a.eidx[q];
            const double2 *o = (const double2 *)(a.obs + 4 * (size_t)e);
            const double2 rr = o[0], er = o[1];
            const double px = a.focal * sqrt(rr.x * rr.x + rr.y * rr.y);
            spx += px;
            if (!isnan(mpx) && !(px <= mpx)) mpx = px;                      // max; a NaN sticks
            srho += er.y;
            vr += er.y;
            vp += er.x;
            const int f = a.fr[e];
#pragma unroll
            for (int k = 0; k < NF; ++k) {                       // (selects, not a register array indexed at run time)
                fr[k] += (f == k) ? er.y : 0.0;
                fe[k] += (f == k) ? 1.0 : 0.0;
            }
            if (a.dneg[e]) flag |= VIO_RES_FLAG_DEPTH;
        }
        const int cnt = q1 - q0;
        const double mean = cnt ? spx / cnt : 0.0;
        if (cnt && !(mean <= a.outlier_px)) flag |= VIO_RES_FLAG_REPROJ;
        if (D == 1) {
            const double lam = a.val[l];
            if (!(lam > 0.0) || !isfinite(lam)) flag |= VIO_RES_FLAG_STATE;
        } else {
            const double *p = a.val + 3 * (size_t)l;
            if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) flag |= VIO_RES_FLAG_STATE;
        }
        a.lm_out[3 * (size_t)l] = mean;
        a.lm_out[3 * (size_t)l + 1] = mpx;
        a.lm_out[3 * (size_t)l + 2] = srho;
        a.flags[l] = (unsigned char)flag;
#pragma unroll
        for (int k = 0; k < 3; ++k) fl[k] = (flag >> k) & 1u ? 1.0 : 0.0;
    }
    // workgroup partials: DPP sum inside each wave, the waves added in order
    const int w = tid >> 6;
    double v;
#define RES_WAVE_SUM(slot, x) v = d_wave_sum_to_lane63(x); if ((tid & 63) == 63) red[(slot) * (LM_NT / 64) + w] = v;
    RES_WAVE_SUM(P_VR, vr)
    RES_WAVE_SUM(P_VP, vp)
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        RES_WAVE_SUM(P_FR + k, fr[k])
        RES_WAVE_SUM(P_FE + k, fe[k])
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { RES_WAVE_SUM(P_FL + k, fl[k]) }
#undef RES_WAVE_SUM
    __syncthreads();
    if (tid < P_N) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < LM_NT / 64; ++k) s += red[tid * (LM_NT / 64) + k];
        a.part[(size_t)blk * P_STRIDE + tid] = s;
    }
