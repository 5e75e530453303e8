// aif_math_main.cpp — the host build of the resident all_image_frame's arithmetic (csrc/vio_aif_math.h) driven by a script
// (tests/test_aif_reference.py builds it, with ASan and UBSan when VIO_TEST_SANITIZE=1, and compares its output with
// tests/aif_reference.py bit for bit).
//
//   in (text), one operation per line, integers read with %lld and doubles with %la; out: the operation's letter, then integers with
//   %d / %lld and doubles with %a:
//     K n ids(n)                      aif_rank of every id: ranks(n)
//     F n t(n) t_0                    aif_find: k
//     A open held n                   aif_imu_status: status
//     B n_frames held n               aif_image_status: status
//     O last k off(last + 1)          aif_slid_off for j = 0 .. last: off(last + 1)
//     Q q(4)                          aif_quat_to_rot: R(9)
//     M A(9) ric(9)                   aif_mul_rict: C(9)
//     E n (sum_dt dv(3))(n)           aif_excitation over records of stride 467: var
//     W F t(F) n_key headers(n_key)   aif_walk: status is_key(F) guess(F)
//     S n ids(n) id                   aif_bisect: index
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vio_aif_math.h"

static bool rd(FILE *f, double *v, int n) {
    for (int k = 0; k < n; ++k)
        if (std::fscanf(f, "%la", &v[k]) != 1) return false;
    return true;
}

static bool ri(FILE *f, long long *v, int n) {
    for (int k = 0; k < n; ++k)
        if (std::fscanf(f, "%lld", &v[k]) != 1) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "r"), *o = std::fopen(argv[2], "w");
    if (!f || !o) return 2;
    char op;
    long long a[4];
    while (std::fscanf(f, " %c", &op) == 1) {
        std::fprintf(o, "%c", op);
        if (op == 'K' || op == 'S') {
            if (!ri(f, a, 1)) return 2;
            const int n = (int)a[0];
            std::vector<long long> raw((size_t)n + 1);
            if (!ri(f, raw.data(), n + (op == 'S' ? 1 : 0))) return 2;
            std::vector<int64_t> ids(raw.begin(), raw.begin() + n);
            if (op == 'K')
                for (int i = 0; i < n; ++i) std::fprintf(o, " %d", aif_rank(ids.data(), n, i));
            else
                std::fprintf(o, " %d", aif_bisect(ids.data(), n, (int64_t)raw[(size_t)n]));
        } else if (op == 'F') {
            if (!ri(f, a, 1)) return 2;
            std::vector<double> t((size_t)a[0] + 1);
            if (!rd(f, t.data(), (int)a[0] + 1)) return 2;
            std::fprintf(o, " %d", aif_find(t.data(), (int)a[0], t[(size_t)a[0]]));
        } else if (op == 'A' || op == 'B') {
            if (!ri(f, a, 3)) return 2;
            std::fprintf(o, " %d", op == 'A' ? aif_imu_status((int)a[0], (int)a[1], (int)a[2]) : aif_image_status((int)a[0], (int)a[1], (int)a[2]));
        } else if (op == 'O') {
            if (!ri(f, a, 2)) return 2;
            const int last = (int)a[0];
            std::vector<long long> raw((size_t)last + 1);
            if (!ri(f, raw.data(), last + 1)) return 2;
            std::vector<int64_t> off(raw.begin(), raw.end());
            for (int j = 0; j <= last; ++j) std::fprintf(o, " %lld", (long long)aif_slid_off(off.data(), last, (int)a[1], j));
        } else if (op == 'Q') {
            double q[4], R[9];
            if (!rd(f, q, 4)) return 2;
            aif_quat_to_rot(q, R);
            for (int k = 0; k < 9; ++k) std::fprintf(o, " %a", R[k]);
        } else if (op == 'M') {
            double v[18], C[9];
            if (!rd(f, v, 18)) return 2;
            aif_mul_rict(v, v + 9, C);
            for (int k = 0; k < 9; ++k) std::fprintf(o, " %a", C[k]);
        } else if (op == 'E') {
            if (!ri(f, a, 1)) return 2;
            const int n = (int)a[0];
            std::vector<double> rec((size_t)467 * (size_t)(n > 0 ? n : 1), 0.0);
            for (int j = 0; j < n; ++j) {
                double v[4];
                if (!rd(f, v, 4)) return 2;
                rec[(size_t)467 * j] = v[0];
                for (int c = 0; c < 3; ++c) rec[(size_t)467 * j + 8 + c] = v[1 + c];
            }
            std::fprintf(o, " %a", aif_excitation(rec.data(), 467, n));
        } else if (op == 'W') {
            if (!ri(f, a, 1)) return 2;
            const int F = (int)a[0];
            std::vector<double> t((size_t)F + 1);
            if (!rd(f, t.data(), F) || !ri(f, a + 1, 1)) return 2;
            const int nk = (int)a[1];
            std::vector<double> hd((size_t)nk + 1);
            if (!rd(f, hd.data(), nk)) return 2;
            std::vector<int32_t> key((size_t)F + 1, 0), guess((size_t)F + 1, 0);
            const int st = aif_walk(t.data(), F, hd.data(), nk, key.data(), guess.data());
            std::fprintf(o, " %d", st);
            if (st == 0) {
                for (int j = 0; j < F; ++j) std::fprintf(o, " %d", key[(size_t)j]);
                for (int j = 0; j < F; ++j) std::fprintf(o, " %d", guess[(size_t)j]);
            }
        } else {
            return 2;
        }
        std::fprintf(o, "\n");
    }
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
