// est_math_main.cpp — the host build of the batched Estimator state's arithmetic (csrc/vio_est_math.h) driven by a script
// (tests/test_est_reference.py builds it with ASan and UBSan and compares its output with tests/est_reference.py bit for bit).
//
//   in (text), one operation per line, every number a double read with %la; out: the operation's letter, then integers with %d and
//   doubles with %a:
//     I Rs(9) Ps(3) Vs(3) Ba(3) Bg(3) g(3) acc0(3) gyr0(3) dt acc(3) gyr(3)   est_imu_step: Rs(9) Ps(3) Vs(3)
//     Q m(9)                                                                  est_rot_to_quat: branch q(4)
//     M q(4)                                                                  est_quat_to_rot: m(9)
//     Y R(9)                                                                  est_R2ypr: ypr(3)
//     Z y_deg                                                                 est_yaw_rot: R(9)
//     A R_origin(9) Rs0(9) q0(4)                                              est_rot_diff: singular rot_diff(9)
//     U rot_diff(9) origin_P0(3) pose(7) p0(3) sb(9)                          est_update_frame: Rs(9) Ps(3) Vs(3) Ba(3) Bg(3)
//     G Ba(3) Bg(3) P(3) last_P(3)                                            est_gate: gate
//     S back_R0(9) back_P0(3) Rs0(9) Ps0(3) ric(9) tic(3)                     est_slide_mats: marg_R(9) marg_P(3) new_R(9) new_P(3)
#include <cstdio>
#include <cstdlib>

#include "vio_est_math.h"

static bool read(FILE *f, double *v, int n) {
    for (int k = 0; k < n; ++k)
        if (std::fscanf(f, "%la", &v[k]) != 1) return false;
    return true;
}

static void put(FILE *o, const double *v, int n) {
    for (int k = 0; k < n; ++k) std::fprintf(o, " %a", v[k]);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "r"), *o = std::fopen(argv[2], "w");
    if (!f || !o) return 2;
    char op;
    double v[40], r[30];
    while (std::fscanf(f, " %c", &op) == 1) {
        std::fprintf(o, "%c", op);
        if (op == 'I') {
            if (!read(f, v, 37)) return 2;
            est_imu_step(v, v + 9, v + 12, v + 15, v + 18, v + 21, v + 24, v + 27, v[30], v + 31, v + 34);
            put(o, v, 15);
        } else if (op == 'Q') {
            if (!read(f, v, 9)) return 2;
            const int b = est_rot_to_quat(v, r);
            std::fprintf(o, " %d", b);
            put(o, r, 4);
        } else if (op == 'M') {
            if (!read(f, v, 4)) return 2;
            est_quat_to_rot(v, r);
            put(o, r, 9);
        } else if (op == 'Y') {
            if (!read(f, v, 9)) return 2;
            est_R2ypr(v, r);
            put(o, r, 3);
        } else if (op == 'Z') {
            if (!read(f, v, 1)) return 2;
            est_yaw_rot(v[0], r);
            put(o, r, 9);
        } else if (op == 'A') {
            if (!read(f, v, 22)) return 2;
            const int s = est_rot_diff(v, v + 9, v + 18, r);
            std::fprintf(o, " %d", s);
            put(o, r, 9);
        } else if (op == 'U') {
            if (!read(f, v, 31)) return 2;
            est_update_frame(v, v + 9, v + 12, v + 19, v + 22, r, r + 9, r + 12, r + 15, r + 18);
            put(o, r, 21);
        } else if (op == 'G') {
            if (!read(f, v, 12)) return 2;
            std::fprintf(o, " %d", est_gate(v, v + 3, v + 6, v + 9));
        } else if (op == 'S') {
            if (!read(f, v, 36)) return 2;
            est_slide_mats(v, v + 9, v + 12, v + 21, v + 24, v + 33, r, r + 9, r + 12, r + 21);
            put(o, r, 24);
        } else {
            return 2;
        }
        std::fprintf(o, "\n");
    }
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
