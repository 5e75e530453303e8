// Body of k_cov_pose and k_cov_pose_batch (vio_covariance.hip), included inside both kernels.  In scope: S, keep, n, cov, cc,
// status, ratio (k_cov_pose's parameters).  A fragment rather than an inline function so that k_cov_pose compiles to the
// instruction stream it had before the batch entry point existed (inlining changed its register allocation).
    __shared__ double A[TRI_MAX];
    __shared__ double col[PD + 1];           // pivot column k
    __shared__ double dg[PD];                // diagonal of S (the pivot ratio)
    __shared__ int red[PD];                  // 171-index -> reduced index, -1: held fixed
    const int tid = threadIdx.x;
    const int ntri = n * (n + 1) / 2;

    for (int q = tid; q < PD; q += POSE_NT) red[q] = -1;
    __syncthreads();
    for (int q = tid; q < n; q += POSE_NT) { red[keep[q]] = q; dg[q] = S[(size_t)keep[q] * PD + keep[q]]; }

    // the thread's packed entries and their (row, column), found once
    int ij[POSE_PER];                        // row << 16 | column
#pragma unroll
    for (int s = 0; s < POSE_PER; ++s) {
        const int p = tid + s * POSE_NT;
        int i = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
        while ((i + 1) * (i + 2) / 2 <= p) ++i;
        while (i * (i + 1) / 2 > p) --i;
        const int j = p - i * (i + 1) / 2;
        ij[s] = (i << 16) | j;
        if (p < ntri) A[p] = S[(size_t)keep[i] * PD + keep[j]];          // lower triangle of S (keep is ascending)
    }
    __syncthreads();

    double rmin = 1.0;
    for (int k = 0; k < n; ++k) {
        if (tid < n) col[tid] = A[tid >= k ? tri(tid, k) : tri(k, tid)];
        __syncthreads();
        const double d = col[k];
        if (!(d > 0.0) || !isfinite(d)) {          // uniform: every thread read the same pivot
            if (tid == 0) status[0] = k;
            return;
        }
        rmin = fmin(rmin, d / dg[k]);
        const double dinv = 1.0 / d;
#pragma unroll
        for (int s = 0; s < POSE_PER; ++s) {
            const int p = tid + s * POSE_NT;
            if (p < ntri) {
                const int i = ij[s] >> 16, j = ij[s] & 0xffff;
                if (i == k && j == k) A[p] = -dinv;
                else if (i == k) A[p] = col[j] * dinv;
                else if (j == k) A[p] = col[i] * dinv;
                else A[p] = A[p] - (col[i] * dinv) * col[j];
            }
        }
        __syncthreads();
    }
    if (tid == 0) { status[0] = -1; ratio[0] = rmin; }

    for (int q = tid; q < PD * PD; q += POSE_NT) {
        const int r = red[q / PD], c = red[q % PD];
        cov[q] = (r >= 0 && c >= 0) ? -A[r >= c ? tri(r, c) : tri(c, r)] : 0.0;
    }
    for (int q = tid; q < CD * CD; q += POSE_NT) {
        const int r = red[cam_to_full(q / CD)], c = red[cam_to_full(q % CD)];
        cc[q] = (r >= 0 && c >= 0) ? -A[r >= c ? tri(r, c) : tri(c, r)] : 0.0;
    }
