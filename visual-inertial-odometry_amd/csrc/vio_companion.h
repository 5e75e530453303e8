// vio_companion.h — the host plumbing every companion library shares (libvio_{cov,res,imu,marg,init,sfm,exrot,pnp,flow,detect,
// reject,clahe,frame}_hip): the device scope, the error text (vio_host_base.h), the pinned/device buffers, the stream and timing events
// of a handle, and the create / destroy pair of the libraries whose create takes (device, stream).  Host code only; every name has
// internal linkage, so nothing here is exported (the libraries' version scripts export their own prefix alone).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "vio_host_base.h"

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

// the time between two recorded events, in ms; NaN when it cannot be had
inline float elapsed_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : NAN;
}

// an error behind work that was enqueued: the stream is drained before the caller sees it
template <class H> vio_status fail_synced(H *h, const char *msg) {
    (void)hipStreamSynchronize(h->q.stream);
    return fail(h->err, VIO_ERR_HIP, "%s", msg);
}

// The create of a handle H {int device; StreamEvents<N> q; ...} on (device, stream).  `extra(h)` is what a library adds once the stream
// and the events exist (a kernel's function attribute, more events); false fails the create, and the handle goes through `destroy`,
// the library's own.
template <class H, class Extra> vio_status create_handle(int32_t device, void *stream, H **out, void (*destroy)(H *), Extra extra) {
    if (!out) return VIO_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VIO_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return VIO_ERR_BAD_ARG;
    DeviceScope dev(device);
    if (!dev.ok) return VIO_ERR_HIP;
    H *h = new (std::nothrow) H();
    if (!h) return VIO_ERR_BAD_ARG;
    h->device = device;
    if (h->q.open_stream(stream) != hipSuccess) { delete h; return VIO_ERR_HIP; }
    if (h->q.create_events() != hipSuccess || !extra(h)) { destroy(h); return VIO_ERR_HIP; }
    *out = h;
    return VIO_OK;
}

template <class H> vio_status create_handle(int32_t device, void *stream, H **out, void (*destroy)(H *)) {
    return create_handle(device, stream, out, destroy, [](H *) { return true; });
}

// ... and its destroy: waits for the stream, then `extra(h)` frees what the library added; the buffers free themselves.
template <class H, class Extra> void destroy_handle(H *h, Extra extra) {
    if (!h) return;
    DeviceScope dev(h->device);
    h->q.release();
    extra(h);
    delete h;
}

template <class H> void destroy_handle(H *h) { destroy_handle(h, [](H *) {}); }

}  // namespace
