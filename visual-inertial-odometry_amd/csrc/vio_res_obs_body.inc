// Body of k_res_obs<D> and k_res_obs_batch<D> (vio_residuals.hip), included inside both kernels.  In scope: D, a (the window's
// ResArgs), blk (the workgroup's index within the window).  A fragment rather than an inline function so that k_res_obs compiles
// to the instruction stream it had before the batch entry point existed.
    __shared__ double sR[(NF + 1) * 9];         // rotations of the 11 poses and (slot 11) of the extrinsic
    const int tid = threadIdx.x;
    for (int f = tid; f <= NF; f += OBS_NT) d_quat_to_R(f < NF ? a.poses + 7 * f + 3 : a.ext + 3, sR + 9 * f);
    __syncthreads();
    const long long e = (long long)blk * OBS_NT + tid;
    if (e >= a.m) return;
    const int l = a.lm[e], fj = a.fr[e];
    double r[2], dep;
    if (D == 1) {
        const int fi = a.host[e];
        dep = d_reproj_residual(sR + 9 * fi, a.poses + 7 * fi, sR + 9 * fj, a.poses + 7 * fj, sR + 9 * NF, a.ext, a.val[l],
                                a.pts_i + 2 * e, a.pts_j + 2 * e, r);
    } else {
        dep = d_reproj_xyz_residual(sR + 9 * fj, a.poses + 7 * fj, sR + 9 * NF, a.ext, a.val + 3 * (size_t)l, a.pts_j + 2 * e, r);
    }
    const double info = a.sqrt_info * a.sqrt_info;
    const double e2 = r[0] * (info * r[0]) + r[1] * (info * r[1]);          // Edge::Chi2 (edge.cc:33-37)
    double r0, r1, r2;
    d_loss(a.loss_type, a.loss_delta, e2, r0, r1, r2);                       // RobustChi2: rho[0] (e2 itself without a loss)
    double2 *o = (double2 *)(a.obs + 4 * e);
    o[0] = make_double2(r[0], r[1]);
    o[1] = make_double2(e2, r0);
    a.dneg[e] = dep <= 0.0;
