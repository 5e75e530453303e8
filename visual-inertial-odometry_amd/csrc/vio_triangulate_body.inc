// vio_triangulate_body.inc — the text of the per-track body of FeatureManager::triangulate (feature_manager.cpp:212-254), included
// inside a function body; the one copy of it.  k_triangulate (vio_kernels.hip) includes it where the lines stood, so that the kernel
// is the token stream it was and keeps its instructions; d_triangulate_track (vio_triangulate_body.h) is the same text as a __device__
// function for everything else (k_fm_export).
//   In scope at the include: sRc, sTc (the camera poses R_f ric, P_f + R_f tic of the VIO_NF frames), int sf (the start frame), int K
//   (the observations), and the macros TRI_X(j), TRI_Y(j) (observation j) and TRI_INIT_DEPTH.  Leaves `double dep`: the depth in the
//   start frame, TRI_INIT_DEPTH where it came out below 0.1 (:251-254).
//   The reference takes the last column of V of a JacobiSVD of the 2K x 4 matrix A (:243); that is the eigenvector of the smallest
//   eigenvalue of A^T A, found here with cyclic Jacobi rotations on the 4x4 (10 accumulated entries instead of a 2K x 4 matrix per
//   thread).
    const double *R0 = sRc + 9 * sf, *t0 = sTc + 3 * sf;
    // every index below is a compile-time constant after unrolling: M and V live in registers, not in scratch
    double M[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) M[a][b] = 0.0;
    for (int j = 0; j < K; ++j) {
        const int f = min(sf + j, VIO_NF - 1);
        const double *R1 = sRc + 9 * f, *t1 = sTc + 3 * f;
        double dt[3] = {t1[0] - t0[0], t1[1] - t0[1], t1[2] - t0[2]}, t[3], R[9];
        d_m3_tvec(R0, dt, t);                                // t = R0^T (t1 - t0)
        d_m3_tmul(R0, R1, R);                                // R = R0^T R1
        double P[3][4];                                      // P = [R^T | -R^T t]
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            P[r][0] = R[r]; P[r][1] = R[3 + r]; P[r][2] = R[6 + r];
            P[r][3] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
        }
        const double x = TRI_X(j), y = TRI_Y(j);
        const double nn = sqrt(x * x + y * y + 1.0);
        const double f0 = x / nn, f1 = y / nn, f2 = 1.0 / nn;
        double ra[4], rb[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { ra[c] = f0 * P[2][c] - f2 * P[0][c]; rb[c] = f1 * P[2][c] - f2 * P[1][c]; }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) M[a][b] += ra[a] * ra[b] + rb[a] * rb[b];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a + 1; b < 4; ++b) M[a][b] = M[b][a];
    // cyclic Jacobi: M -> diagonal, V accumulates the rotations (columns = eigenvectors)
    double V[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) V[a][b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = M[0][1] * M[0][1] + M[0][2] * M[0][2] + M[0][3] * M[0][3] + M[1][2] * M[1][2] + M[1][3] * M[1][3] + M[2][3] * M[2][3];
        const double dg = M[0][0] * M[0][0] + M[1][1] * M[1][1] + M[2][2] * M[2][2] + M[3][3] * M[3][3];
        if (off <= 1e-36 * dg) break;                          // off-diagonal mass below rounding of the diagonal: converged
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = M[p][q];
                if (apq != 0.0) {
                    const double theta = (M[q][q] - M[p][p]) / (2.0 * apq);
                    const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const double mkp = M[k][p], mkq = M[k][q]; M[k][p] = c * mkp - sn * mkq; M[k][q] = sn * mkp + c * mkq; }
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const double mpk = M[p][k], mqk = M[q][k]; M[p][k] = c * mpk - sn * mqk; M[q][k] = sn * mpk + c * mqk; }
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - sn * vkq; V[k][q] = sn * vkp + c * vkq; }
                }
            }
    }
    // eigenvector of the smallest eigenvalue, picked with selects (no run-time index into V)
    double best = M[0][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
    for (int a = 1; a < 4; ++a) if (M[a][a] < best) { best = M[a][a]; v2 = V[2][a]; v3 = V[3][a]; }
    double dep = v2 / v3;                                    // svd_V[2] / svd_V[3]   (:245)
    if (dep < 0.1) dep = TRI_INIT_DEPTH;                     // :252
