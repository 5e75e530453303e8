// est_init_math_main.cpp — the host build of the hand-over's and the re-linearisation's arithmetic (csrc/vio_est_init_math.h) driven by
// a script (tests/test_est_init_reference.py builds it with ASan and UBSan and compares its output with tests/est_init_reference.py bit
// for bit).  The format is est_math_main.cpp's:
//
//   in (text), one operation per line, every number a double read with %la; out: the operation's letter, then integers with %d and
//   doubles with %a:
//     F pose(7) sb(9)                          est_init_frame: Rs(9) Ps(3) Vs(3) Ba(3) Bg(3) lin_bias(6)
//     V rot(9) g(3)                            est_init_gravity: g(3)
//     R Ba(3) Bg(3) lin_bias(6) tba tbg        est_relin_moved: moved
#include <cstdio>
#include <cstdlib>

#include "vio_est_init_math.h"

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
    double v[16], r[27];
    while (std::fscanf(f, " %c", &op) == 1) {
        std::fprintf(o, "%c", op);
        if (op == 'F') {
            if (!read(f, v, 16)) return 2;
            est_init_frame(v, v + 7, r, r + 9, r + 12, r + 15, r + 18, r + 21);
            put(o, r, 27);
        } else if (op == 'V') {
            if (!read(f, v, 12)) return 2;
            est_init_gravity(v, v + 9, r);
            put(o, r, 3);
        } else if (op == 'R') {
            if (!read(f, v, 14)) return 2;
            std::fprintf(o, " %d", est_relin_moved(v, v + 3, v + 6, v[12], v[13]) ? 1 : 0);
        } else {
            return 2;
        }
        std::fprintf(o, "\n");
    }
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
