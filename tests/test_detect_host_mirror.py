"""The detector's per-pixel arithmetic (csrc/vio_detect_math.h: BORDER_REFLECT_101, the Sobel pair, the response of the box sums, the
order of the keys, the disc tests) compiled for the host with a small driver, against tests/detect_reference.py: identical bits.  The
header is the device's code; what the kernels add around it (the tiles, the reduction, the greedy rounds) is checked on the GPU
(tests/test_gpu_detect.py)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_reference as dr  # noqa: E402
import flow_reference as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
WRAPPER = '''
#include <algorithm>
#include <vector>
#include "vio_detect_math.h"
// the response map of an image, pixel by pixel from the header's pieces
extern "C" void response_host(const uint8_t *img, int w, int h, int stride, double *out) {
    std::vector<int> gx((size_t)w * h), gy((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int v[3][3];
            for (int j = 0; j < 3; ++j)
                for (int i = 0; i < 3; ++i) v[j][i] = img[(size_t)det_refl(y - 1 + j, h) * stride + det_refl(x - 1 + i, w)];
            det_sobel(v, gx[(size_t)y * w + x], gy[(size_t)y * w + x]);
        }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int32_t a = 0, b = 0, c = 0;
            for (int j = -1; j <= 1; ++j)
                for (int i = -1; i <= 1; ++i) {
                    const size_t q = (size_t)det_refl(y + j, h) * w + det_refl(x + i, w);
                    a += gx[q] * gx[q]; b += gx[q] * gy[q]; c += gy[q] * gy[q];
                }
            out[(size_t)y * w + x] = det_response(a, b, c);
        }
}
// the indices of n keys (k, x, y) in the header's order
extern "C" void sort_keys_host(const unsigned long long *k, const int32_t *x, const int32_t *y, int n, int32_t *order) {
    std::vector<int32_t> o(n);
    for (int i = 0; i < n; ++i) o[i] = i;
    std::sort(o.begin(), o.end(), [&](int32_t p, int32_t q) {
        const DetKey a = {k[p], x[p], y[p]}, b = {k[q], x[q], y[q]};
        return det_key_before(a, b);
    });
    std::copy(o.begin(), o.end(), order);
}
extern "C" unsigned long long track_key_host(int32_t cnt, int32_t index) { return det_track_key(cnt, index); }
extern "C" int32_t d2_host(int32_t md) { return det_d2(md); }
extern "C" int struck_host(int strict, int x, int y, int cx, int cy, int d2) {
    return strict ? det_struck<true>(x, y, cx, cy, d2) : det_struck<false>(x, y, cx, cy, d2);
}
'''


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found")
    d = tmp_path_factory.mktemp("detect_mirror")
    src, so = d / "mirror.cpp", d / "libmirror.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.response_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.sort_keys_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.track_key_host.argtypes = [C.c_int32, C.c_int32]
    lib.track_key_host.restype = C.c_ulonglong
    lib.d2_host.argtypes = [C.c_int32]
    lib.d2_host.restype = C.c_int32
    lib.struck_host.argtypes = [C.c_int] * 6
    return lib


def host_response(mirror, img):
    img = np.ascontiguousarray(img)
    out = np.zeros(img.shape, dtype=np.float64)
    mirror.response_host(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], out.ctypes.data)
    return out


def test_response_matches_the_restatement(mirror):
    rng = np.random.RandomState(1)
    steep = np.zeros((16, 24), dtype=np.uint8)
    steep[:, ::2] = 255
    images = [rng.randint(0, 256, size=s).astype(np.uint8) for s in ((13, 17), (1, 1), (2, 5), (5, 2), (3, 3), (1, 9), (40, 33))]
    images += [steep, steep.T.copy(), np.full((7, 9), 200, dtype=np.uint8), fr.texture(96, 80, seed=11)]
    for img in images:
        got, ref = host_response(mirror, img), dr.response(img)
        assert got.tobytes() == ref.tobytes(), img.shape
        assert np.all(got >= 0)


def test_key_order_matches_the_restatement(mirror):
    # candidates: R descending, then the pixel index descending, with many equal responses
    rng = np.random.RandomState(2)
    w, h, n = 37, 29, 400
    pix = rng.choice(w * h, size=n, replace=False).astype(np.int64)
    r = rng.choice([0.5, 1.0, 3.25, 1e9, 5e-324], size=n)
    k = r.view(np.uint64).copy()
    x, y = (pix % w).astype(np.int32), (pix // w).astype(np.int32)
    order = np.zeros(n, dtype=np.int32)
    mirror.sort_keys_host(k.ctypes.data, x.ctypes.data, y.ctypes.data, n, order.ctypes.data)
    ref = np.lexsort((pix, r))[::-1]
    assert np.array_equal(order, ref)
    # tracked points: track_cnt descending (negative counts too), then the index ascending
    cnt = rng.randint(-3, 4, size=100).astype(np.int32)
    cnt[:4] = [2 ** 31 - 1, -2 ** 31, 0, 2 ** 31 - 1]
    k = np.array([mirror.track_key_host(int(c), i) for i, c in enumerate(cnt)], dtype=np.uint64)
    assert np.all(k != 0)
    zero = np.zeros(100, dtype=np.int32)
    order = np.zeros(100, dtype=np.int32)
    mirror.sort_keys_host(k.ctypes.data, zero.ctypes.data, zero.ctypes.data, 100, order.ctypes.data)
    assert list(order) == sorted(range(100), key=lambda i: (-int(cnt[i]), i))
    assert all(0xFFFFFFFF - (int(k[i]) & 0xFFFFFFFF) == i for i in range(100))


def test_disc_tests(mirror):
    assert [mirror.d2_host(m) for m in (0, 1, 30, 32767, 32768, 2 ** 31 - 1)] == [0, 1, 900, 32767 ** 2, 2 ** 30, 2 ** 30]
    assert 2 * (dr.MAX_DIM - 1) ** 2 < 2 ** 30                  # (every distance of two pixels is below the cap)
    for (x, y, d2) in ((3, 4, 25), (3, 4, 24), (3, 4, 26), (0, 0, 0), (1, 0, 0), (1, 0, 1)):
        dd = x * x + y * y
        assert bool(mirror.struck_host(0, x + 7, y + 9, 7, 9, d2)) == (dd <= d2)
        assert bool(mirror.struck_host(1, x + 7, y + 9, 7, 9, d2)) == (dd < d2 or dd == 0)
