/*
 * vio_imu.h — batched IMU pre-integration and bias re-propagation on the GPU (companion library libvio_imu_hip.so).
 *
 * The reference pre-integrates on the host, one interval at a time: IntegrationBase(acc_0, gyr_0, Ba, Bg) + push_back
 * (VM/include/factor/integration_base.h:13-36, midPointIntegration :54-133), and repropagate (:38-52) when a bias estimate moves.
 * libvio_hip's vio_preintegrate (include/vio_backend.h) does the same, one call per interval.  This library keeps the raw samples
 * of many intervals on the device and propagates any subset of them at new biases in one launch (k_imu_propagate, one wavefront
 * per interval); the records it returns are the vio_preint that vio_set_imu_all takes.  It needs nothing from libvio_hip but the
 * vio_preint / vio_status types.  DESIGN.md section 12 has the kernel.
 *
 * Semantics are vio_preintegrate's, interval for interval: the mid-point rule, delta_q rotated before it is normalised,
 * linearized_ba/bg set to the biases used, jacobian and covariance 15x15 row-major in StateOrder (O_P=0, O_R=3, O_V=6, O_BA=9,
 * O_BG=12).  The matrix products run in another summation order than the host's (the matrix cores), so results agree with
 * vio_preintegrate to rounding, not bit for bit; two identical calls are bitwise identical (no atomics, a fixed order).
 * An interval with no samples gives sum_dt = 0, delta_q = identity, jacobian = I, covariance = 0.
 * Errors: VIO_ERR_BAD_ARG, with nothing written, for a bad argument.  Non-finite samples or biases are not refused: they go through
 * to the outputs, the call returns VIO_ERR_NOT_FINITE and vio_imu_last_error names the lowest interval with a non-finite record.
 * One handle per thread at a time.  The calling thread's current HIP device is left as the caller had it.
 */
#ifndef VIO_IMU_H
#define VIO_IMU_H

#include "vio_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VIO_IMU_API __attribute__((visibility("default")))
#else
#define VIO_IMU_API
#endif

#define VIO_IMU_VERSION 1

/* Continuous-time noise densities: ACC_N, GYR_N, ACC_W, GYR_W of the YAML (vio_simulation.yaml:60-63). */
typedef struct vio_imu_noise {
    double acc_n, gyr_n, acc_w, gyr_w;
} vio_imu_noise;

struct vio_imu;

/* A handle on `device`.  stream: a hipStream_t to enqueue on, or NULL for one of the library's own. */
VIO_IMU_API vio_status vio_imu_create(int32_t device, void *stream, struct vio_imu **out);
VIO_IMU_API void vio_imu_destroy(struct vio_imu *h);
VIO_IMU_API const char *vio_imu_last_error(const struct vio_imu *h);
VIO_IMU_API int32_t vio_imu_version(void);

/* n intervals in CSR form, uploaded once and kept on the device (a later load replaces them).  Interval i starts from
 * first[i] = (acc0, gyr0), the sample the IntegrationBase constructor takes, and folds in samples [offset[i], offset[i+1]) of
 * dt / acc / gyr.  offset: n + 1 entries, offset[0] = 0, non-decreasing; S = offset[n] samples (S = 0: dt/acc/gyr may be NULL).
 * n = 0 is allowed and loads nothing. */
VIO_IMU_API vio_status vio_imu_load(struct vio_imu *h, int32_t n, const int64_t *offset, const double *first /*[n][6]*/,
                                    const double *dt /*[S]*/, const double *acc /*[S][3]*/, const double *gyr /*[S][3]*/,
                                    const vio_imu_noise *noise);

/* IntegrationBase(acc0, gyr0, ba[i], bg[i]) + push_back over the interval's samples, for the `count` intervals listed in `which`
 * (each in [0, n); NULL: all n, and then count must be n).  ba / bg: [n][3], indexed by interval.  Writes out[which[k]] (or out[i])
 * and nothing else of out, which has n entries.  Calling it again with other biases is repropagate(). */
VIO_IMU_API vio_status vio_imu_propagate(struct vio_imu *h, int32_t count, const int32_t *which, const double *ba /*[n][3]*/,
                                         const double *bg /*[n][3]*/, vio_preint *out /*[n]*/);

/* ms of the last propagate: host packing + upload, k_imu_propagate (device events), the whole call. */
VIO_IMU_API vio_status vio_imu_timing(const struct vio_imu *h, double *out3);

#ifdef __cplusplus
}
#endif

#endif
