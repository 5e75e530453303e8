// camera_math_main.cpp — the host build of the camera model library's arithmetic (csrc/vio_camera_math.h, with the camera check of
// csrc/vio_camera_host.h) as a stand-alone program (tests/test_camera_host_mirror.py; with VIO_TEST_SANITIZE=1 under ASan and UBSan).
//
//   in  (binary): int32 model, width, height, reserved; 16 doubles params            a vio_camera_model
//                 2 doubles focal, dt; int64 n; n x 2 floats pts; n x 2 floats prev_un
//   out (binary): int32 status of the camera check, npow, no_distortion, n_clamped;
//                 then, if the camera was accepted: n x 3 doubles rays | n x 2 doubles (theta, phi) | n x 2 doubles virtual pixels |
//                 n x 2 floats un_pts | n x 2 floats velocity | n bytes flags (1: the lift is bad, 2: clamped)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vio_camera_math.h"
#include "vio_host_base.h"
#include "vio_camera_host.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    vio_camera_model m;
    double c[2];
    long long n = 0;
    if (std::fread(&m, sizeof(m), 1, f) != 1 || std::fread(c, sizeof(double), 2, f) != 2 || std::fread(&n, sizeof(n), 1, f) != 1 || n < 0 ||
        n > (1 << 20))
        return 4;
    std::vector<float> pts(2 * (size_t)n), prev(2 * (size_t)n);
    if (n > 0 && (std::fread(pts.data(), sizeof(float), pts.size(), f) != pts.size() || std::fread(prev.data(), sizeof(float), prev.size(), f) != prev.size()))
        return 5;
    std::fclose(f);
    ErrText err = {0};
    int32_t head[4] = {cam_check_model(err, &m), 0, 0, 0};
    std::vector<double> rays(3 * (size_t)n), ang(2 * (size_t)n), virt(2 * (size_t)n);
    std::vector<float> un(2 * (size_t)n), vel(2 * (size_t)n);
    std::vector<uint8_t> flags((size_t)n);
    if (head[0] == VIO_OK) {
        const CamDev C = cam_device_form(m);
        head[1] = C.npow; head[2] = C.no_distortion;
        for (long long k = 0; k < n; ++k) {
            CamRay r = {};
            cam_lift(C, (double)pts[2 * k], (double)pts[2 * k + 1], r);
            rays[3 * k] = r.x; rays[3 * k + 1] = r.y; rays[3 * k + 2] = r.z;
            ang[2 * k] = r.theta; ang[2 * k + 1] = r.phi;
            virt[2 * k] = cam_virtual(c[0], r.x, r.z, C.half_w); virt[2 * k + 1] = cam_virtual(c[0], r.y, r.z, C.half_h);
            un[2 * k] = cam_unpoint(r.x, r.z); un[2 * k + 1] = cam_unpoint(r.y, r.z);
            vel[2 * k] = rej_velocity(un[2 * k], prev[2 * k], c[1]); vel[2 * k + 1] = rej_velocity(un[2 * k + 1], prev[2 * k + 1], c[1]);
            flags[(size_t)k] = (uint8_t)((cam_ray_bad(r) ? CAM_FLAG_BAD : 0) | (r.clamped ? CAM_FLAG_CLAMPED : 0));
            head[3] += r.clamped;
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 6;
    std::fwrite(head, sizeof(int32_t), 4, f);
    if (head[0] == VIO_OK && n > 0) {                        // (an empty vector's data() may be null, which fwrite must not get)
        std::fwrite(rays.data(), sizeof(double), rays.size(), f);
        std::fwrite(ang.data(), sizeof(double), ang.size(), f);
        std::fwrite(virt.data(), sizeof(double), virt.size(), f);
        std::fwrite(un.data(), sizeof(float), un.size(), f);
        std::fwrite(vel.data(), sizeof(float), vel.size(), f);
        std::fwrite(flags.data(), 1, flags.size(), f);
    }
    return std::fclose(f) == 0 ? 0 : 7;
}
