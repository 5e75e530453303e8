// vio_companion.h — the host plumbing every companion library (libvio_{cov,res,imu,marg,init}_hip) shares: the device scope, the
// error text, the pinned/device buffers, and the stream and timing events of a handle.  Host code only; every name has internal
// linkage, so nothing here is exported (the libraries' version scripts export their own prefix alone).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "../../include/vio_backend.h"

namespace {

// The calling thread's current device is the caller's: switched to the handle's for the library's calls, put back on the way out.
struct DeviceScope {
    int prev = -1;
    bool ok = false;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

// a handle's last error, returned by its vio_*_last_error
typedef char ErrText[512];

__attribute__((format(printf, 3, 4))) inline vio_status fail(ErrText &err, vio_status st, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof(ErrText), fmt, ap);
    va_end(ap);
    return st;
}

inline vio_status hip_ck(ErrText &err, hipError_t e, const char *what) {
    if (e == hipSuccess) return VIO_OK;
    return fail(err, VIO_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// A pinned host buffer and its device twin of one capacity, grown together (never shrunk).
template <class T> struct Twin {
    T *d = nullptr, *h = nullptr;
    size_t cap = 0;
    Twin() = default;
    Twin(const Twin &) = delete;
    Twin &operator=(const Twin &) = delete;
    ~Twin() { release(); }
    void release() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = nullptr; h = nullptr; cap = 0;
    }
    vio_status ensure(ErrText &err, size_t bytes) {
        if (bytes <= cap) return VIO_OK;
        release();
        const size_t want = bytes + bytes / 4 + 4096;
        vio_status st = hip_ck(err, hipMalloc((void **)&d, want), "hipMalloc");
        if (st != VIO_OK) return st;
        st = hip_ck(err, hipHostMalloc((void **)&h, want, hipHostMallocDefault), "hipHostMalloc");
        if (st != VIO_OK) return st;
        cap = want;
        return VIO_OK;
    }
};

// Device scratch with no host twin, grown by the same policy.
template <class T> struct DevBuf {
    T *d = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (d) (void)hipFree(d);
        d = nullptr; cap = 0;
    }
    vio_status ensure(ErrText &err, size_t bytes) {
        if (bytes <= cap) return VIO_OK;
        release();
        const size_t want = bytes + bytes / 4 + 4096;
        vio_status st = hip_ck(err, hipMalloc((void **)&d, want), "hipMalloc");
        if (st != VIO_OK) return st;
        cap = want;
        return VIO_OK;
    }
};

// A handle's stream and its N timing events.  The stream is the caller's (borrowed) or, from open_stream(nullptr), a new
// non-blocking one the handle owns.  release() waits for the stream, destroys the events and an owned stream.
template <int N> struct StreamEvents {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[N] = {};
    hipError_t open_stream(void *caller) {
        if (caller) {
            stream = (hipStream_t)caller;
            return hipSuccess;
        }
        const hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        own_stream = e == hipSuccess;
        if (!own_stream) stream = nullptr;
        return e;
    }
    hipError_t create_events() {
        for (hipEvent_t &e : ev) {
            const hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) {
                e = nullptr;
                return r;
            }
        }
        return hipSuccess;
    }
    void release() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipEvent_t &e : ev)
            if (e) (void)hipEventDestroy(e);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the time between two recorded events, in ms; NaN when it cannot be had
inline float elapsed_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : NAN;
}

}  // namespace
