// vio_triangulate_body.h — the per-track body of FeatureManager::triangulate (feature_manager.cpp:212-254) as a __device__ function
// (DESIGN.md section 26).  Its text is csrc/vio_triangulate_body.inc, the one copy: k_fm_export (vio_fm_body.inc) calls the function;
// k_triangulate (vio_kernels.hip) includes the text where its lines stood, because inlining a function there changed the loop's
// shape and with it which products the compiler fused: the depths moved in the last bits.
//   sRc / sTc: the camera poses R_f ric, P_f + R_f tic of the VIO_NF frames, staged by the caller.  The track starts at frame sf and
//   has K observations; pt(j, x, y) loads observation j.  Returns the depth in the start frame, init_depth where it came out below
//   0.1 (:251-254).
// Neither file sets a contraction pragma: each includer compiles them under its own, and vio_kernels.hip keeps the default.
// Needs vio_device_math.h (d_m3_tvec, d_m3_tmul) and VIO_NF (vio_types.h) before it.
#pragma once

template <class LoadPt> __device__ __forceinline__ double tri_point(const LoadPt &pt, int j, int c) {
    double x, y;
    pt(j, x, y);
    return c ? y : x;
}

template <class LoadPt>
__device__ __forceinline__ double d_triangulate_track(const double *sRc, const double *sTc, const int sf, const int K, const LoadPt &pt,
                                                      const double init_depth) {
#define TRI_X(j) tri_point(pt, j, 0)
#define TRI_Y(j) tri_point(pt, j, 1)
#define TRI_INIT_DEPTH init_depth
#include "vio_triangulate_body.inc"
#undef TRI_X
#undef TRI_Y
#undef TRI_INIT_DEPTH
    return dep;
}
