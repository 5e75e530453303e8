// camera_project_main.cpp — the host build of spaceToPlane (csrc/vio_camera_project_math.h) as a stand-alone program
// (tests/test_camera_project_cpu.py; with VIO_TEST_SANITIZE=1 under ASan and UBSan).
//
//   in  (binary): int32 model, width, height, reserved; 16 doubles params            a vio_camera_model
//                 int64 n_inv; 20 doubles inv_poly (read up to n_inv); int64 n; n x 3 doubles points
//   out (binary): n x 2 doubles pixels | n bytes flags
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vio_camera_project_math.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    vio_camera_model m;
    long long n_inv = 0, n = 0;
    double inv[VIO_CAMERA_INV_POLY_MAX];
    if (std::fread(&m, sizeof(m), 1, f) != 1 || std::fread(&n_inv, sizeof(n_inv), 1, f) != 1 ||
        std::fread(inv, sizeof(double), VIO_CAMERA_INV_POLY_MAX, f) != VIO_CAMERA_INV_POLY_MAX || std::fread(&n, sizeof(n), 1, f) != 1 || n < 0 ||
        n > (1 << 20) || n_inv < 0 || n_inv > VIO_CAMERA_INV_POLY_MAX)
        return 4;
    std::vector<double> pts(3 * (size_t)n);
    if (n > 0 && std::fread(pts.data(), sizeof(double), pts.size(), f) != pts.size()) return 5;
    std::fclose(f);
    CamProj C = cam_project_form(m);
    for (int i = 0; i < VIO_CAMERA_INV_POLY_MAX; ++i) C.inv[i] = i < n_inv ? inv[i] : 0.0;      // (vio_camera_set_inv_poly)
    C.n_inv = (int32_t)n_inv;
    std::vector<double> pix(2 * (size_t)n);
    std::vector<uint8_t> flags((size_t)n);
    for (long long k = 0; k < n; ++k)
        flags[(size_t)k] = (uint8_t)cam_project(C, pts[3 * k], pts[3 * k + 1], pts[3 * k + 2], pix[2 * k], pix[2 * k + 1]);
    f = std::fopen(argv[2], "wb");
    if (!f) return 6;
    if (n > 0) {                                             // (an empty vector's data() may be null, which fwrite must not get)
        std::fwrite(pix.data(), sizeof(double), pix.size(), f);
        std::fwrite(flags.data(), 1, flags.size(), f);
    }
    return std::fclose(f) == 0 ? 0 : 7;
}
