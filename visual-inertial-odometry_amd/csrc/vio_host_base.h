// vio_host_base.h — the part of the host plumbing that needs no HIP header: a handle's error text, the 256-byte carving and the row
// copies.  vio_companion.h includes it; the stage host files (vio_{clahe,flow,detect,reject}_host.h) need nothing else of the plumbing,
// so a plain C++ compiler can build them (tests/cpp/front_host_main.cpp).  Every name has internal linkage.
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/vio_backend.h"

namespace {

// a handle's last error, returned by its vio_*_last_error
typedef char ErrText[512];

__attribute__((format(printf, 3, 4))) inline vio_status fail(ErrText &err, vio_status st, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof(ErrText), fmt, ap);
    va_end(ap);
    return st;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// `height` rows of `width` bytes from rows `stride` apart to rows `pitch` apart
inline void copy_rows(uint8_t *dst, int pitch, const uint8_t *src, int stride, int width, int height) {
    for (int y = 0; y < height; ++y) std::memcpy(dst + (size_t)y * (size_t)pitch, src + (size_t)y * (size_t)stride, (size_t)width);
}

// ... the padding of every row zero
inline void pack_rows(uint8_t *dst, int pitch, const uint8_t *src, int width, int height, int stride) {
    copy_rows(dst, pitch, src, stride, width, height);
    for (int y = 0; y < height && pitch > width; ++y) std::memset(dst + (size_t)y * (size_t)pitch + width, 0, (size_t)(pitch - width));
}

}  // namespace
