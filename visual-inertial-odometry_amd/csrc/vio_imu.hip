// vio_imu.hip — batched IMU pre-integration and bias re-propagation (include/vio_imu.h).
//
// The raw samples of n intervals are uploaded once (vio_imu_load) and stay on the device; vio_imu_propagate runs IntegrationBase
// (VM/include/factor/integration_base.h:13-158) over any subset of them at new biases in one launch of k_imu_propagate:
//   one wavefront (one 64-thread workgroup) per interval, the intervals independent across the grid.
//   The mid-point state (delta_p, delta_q, delta_v and the 3 x 3 blocks of F and V) is wave-uniform: every lane computes it in the
//   host routine's operation order (vio_host::preintegrate, host_dense.cpp), with contraction off, and keeps it in registers.
//   J and C are 16 x 16 zero-padded tiles held in registers in the accumulator layout of v_mfma_f64_16x16x4_f64 (lane l, register
//   q: row (l >> 4) + 4q, column l & 15).  Each sample writes F (15 x 15) and G = V sqrt(N) (15 x 18, padded to 16 x 20) into LDS
//   from their 3 x 3 blocks, every lane reads its A/B fragments of them back (row l & 15, k = 4s + (l >> 4)), and
//     J <- F J                       4 MFMAs (J's accumulator registers are the B fragments as they stand)
//     U <- C F^T                     4 MFMAs (C is symmetric: its accumulator registers are also its A fragments)
//     C <- G G^T + F U               5 + 4 MFMAs (G's fragment is its own A and B operand)
//   17 MFMAs per sample, one dependent chain per wave.
// No atomics; every sum has a fixed order, so two identical calls give bitwise the same records.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vio_imu.h"
#include "vio_companion.h"

#include "vio_imu_body.inc"

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
struct vio_imu {
    int device = 0;
    StreamEvents<2> q;                              // the caller's stream or an owned one, and the timing events
    ErrText err = {0};
    int32_t n = -1;                                 // intervals loaded (-1: nothing yet)
    vio_imu_noise noise = {0, 0, 0, 0};
    // device: off | first | dt | acc | gyr, one allocation replaced by every load
    DevBuf<char> data;
    int64_t *d_off = nullptr;
    double *d_first = nullptr, *d_dt = nullptr, *d_acc = nullptr, *d_gyr = nullptr;
    // per call: bias | which up, the records down
    Twin<char> in, out;
    double timing[3] = {0, 0, 0};
};

extern "C" {

vio_status vio_imu_create(int32_t device, void *stream, vio_imu **out) {
    if (!out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    if (device < 0) return VIO_ERR_BAD_ARG;
    vio_imu *h = new (std::nothrow) vio_imu;
    if (!h) return VIO_ERR_BAD_ARG;
    h->device = device;
    DeviceScope dev(device);
    if (!dev.ok) { delete h; return VIO_ERR_HIP; }
    if (h->q.open_stream(stream) != hipSuccess) { delete h; return VIO_ERR_HIP; }
    if (h->q.create_events() != hipSuccess) { vio_imu_destroy(h); return VIO_ERR_HIP; }
    *out = h;
    return VIO_OK;
}

void vio_imu_destroy(vio_imu *h) {
    if (!h) return;
    DeviceScope dev(h->device);
    h->q.release();
    delete h;                                       // (the buffers free themselves)
}

const char *vio_imu_last_error(const vio_imu *h) { return h ? h->err : "null handle"; }

int32_t vio_imu_version(void) { return VIO_IMU_VERSION; }

vio_status vio_imu_load(vio_imu *h, int32_t n, const int64_t *offset, const double *first, const double *dt, const double *acc,
                        const double *gyr, const vio_imu_noise *noise) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (n < 0 || !offset || !noise || (n > 0 && !first)) return fail(h->err, VIO_ERR_BAD_ARG, "n=%d, or offset / first / noise is NULL", n);
    if (offset[0] != 0) return fail(h->err, VIO_ERR_BAD_ARG, "offset[0] = %lld, not 0", (long long)offset[0]);
    for (int32_t i = 0; i < n; ++i)
        if (offset[i + 1] < offset[i])
            return fail(h->err, VIO_ERR_BAD_ARG, "offset decreases at interval %d (%lld -> %lld)", i, (long long)offset[i], (long long)offset[i + 1]);
    const int64_t S = offset[n];
    if (S > 0 && (!dt || !acc || !gyr)) return fail(h->err, VIO_ERR_BAD_ARG, "%lld samples and dt / acc / gyr is NULL", (long long)S);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;
    h->data.release();
    h->n = -1;
    const size_t oOff = 0, oFirst = align256(oOff + 8 * ((size_t)n + 1)), oDt = align256(oFirst + 48 * (size_t)n),
                 oAcc = align256(oDt + 8 * (size_t)S), oGyr = align256(oAcc + 24 * (size_t)S), total = align256(oGyr + 24 * (size_t)S);
    if ((st = hip_ck(h->err, hipMalloc((void **)&h->data.d, total), "hipMalloc")) != VIO_OK) return st;
    h->d_off = (int64_t *)(h->data.d + oOff);
    h->d_first = (double *)(h->data.d + oFirst);
    h->d_dt = (double *)(h->data.d + oDt);
    h->d_acc = (double *)(h->data.d + oAcc);
    h->d_gyr = (double *)(h->data.d + oGyr);
    struct { void *d; const void *s; size_t b; } cp[5] = {{h->d_off, offset, 8 * ((size_t)n + 1)}, {h->d_first, first, 48 * (size_t)n},
                                                          {h->d_dt, dt, 8 * (size_t)S}, {h->d_acc, acc, 24 * (size_t)S},
                                                          {h->d_gyr, gyr, 24 * (size_t)S}};
    for (auto &c : cp)
        if (c.b && (st = hip_ck(h->err, hipMemcpyAsync(c.d, c.s, c.b, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;
    h->n = n;
    h->noise = *noise;
    return VIO_OK;
}

vio_status vio_imu_propagate(vio_imu *h, int32_t count, const int32_t *which, const double *ba, const double *bg, vio_preint *out) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (h->n < 0) return fail(h->err, VIO_ERR_BAD_ARG, "nothing loaded");
    const int32_t n = h->n;
    if (!which && count != n) return fail(h->err, VIO_ERR_BAD_ARG, "which = NULL and count %d is not the %d intervals loaded", count, n);
    if (count < 0) return fail(h->err, VIO_ERR_BAD_ARG, "count %d", count);
    if (count == 0) return VIO_OK;
    if (!ba || !bg || !out) return fail(h->err, VIO_ERR_BAD_ARG, "ba / bg / out is NULL");
    if (which)
        for (int32_t k = 0; k < count; ++k)
            if (which[k] < 0 || which[k] >= n) return fail(h->err, VIO_ERR_BAD_ARG, "which[%d] = %d is not an interval (n = %d)", k, which[k], n);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    const size_t oB = 0, oW = align256(oB + 48 * (size_t)count), nin = align256(oW + 4 * (size_t)count);
    const size_t nout = (size_t)IMU_REC * 8 * count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK) return st;
    if ((st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    double *hb = (double *)(h->in.h + oB);
    int *hw = (int *)(h->in.h + oW);
    for (int32_t k = 0; k < count; ++k) {
        const int32_t i = which ? which[k] : k;
        hw[k] = i;
        for (int c = 0; c < 3; ++c) { hb[6 * k + c] = ba[3 * (size_t)i + c]; hb[6 * k + 3 + c] = bg[3 * (size_t)i + c]; }
    }
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();

    ImuArgs a;
    a.off = h->d_off; a.first = h->d_first; a.dt = h->d_dt; a.acc = h->d_acc; a.gyr = h->d_gyr;
    a.bias = (const double *)(h->in.d + oB);
    a.which = (const int *)(h->in.d + oW);
    a.out = (double *)h->out.d;
    a.sn[0] = h->noise.acc_n; a.sn[1] = h->noise.gyr_n; a.sn[2] = h->noise.acc_w; a.sn[3] = h->noise.gyr_w;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_imu_propagate, dim3(count), dim3(IMU_NT), 0, h->q.stream, a);
    if ((st = hip_ck(h->err, hipGetLastError(), "k_imu_propagate launch")) != VIO_OK) return st;
    hipEventRecord(h->q.ev[1], h->q.stream);
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->out.h, h->out.d, nout, hipMemcpyDeviceToHost, h->q.stream), "read-back")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "k_imu_propagate")) != VIO_OK) return st;

    const double *rec = (const double *)h->out.h;
    int32_t bad = -1;
    for (int32_t k = 0; k < count; ++k) {
        const int32_t i = hw[k];
        const double *r = rec + (size_t)IMU_REC * k;
        std::memcpy(&out[i], r, sizeof(vio_preint));
        if (bad < 0 || i < bad)
            for (int e = 0; e < IMU_REC; ++e)
                if (!std::isfinite(r[e])) { bad = i; break; }
    }
    float kms = 0.f;
    hipEventElapsedTime(&kms, h->q.ev[0], h->q.ev[1]);
    h->timing[0] = t_host;
    h->timing[1] = kms;
    h->timing[2] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    if (bad >= 0) return fail(h->err, VIO_ERR_NOT_FINITE, "interval %d: non-finite pre-integration (a non-finite sample or bias)", bad);
    return VIO_OK;
}

vio_status vio_imu_timing(const vio_imu *h, double *out3) {
    if (!h || !out3) return VIO_ERR_BAD_ARG;
    std::memcpy(out3, h->timing, sizeof(h->timing));
    return VIO_OK;
}

}   // extern "C"
