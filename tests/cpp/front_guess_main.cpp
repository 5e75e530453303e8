// front_guess_main.cpp — csrc/vio_front_guess_math.h on the host, for tests/test_front_guess_cpu.py: the text vio_frame.hip and
// k_front_guess / k_front_fallback compile, run over one slot's table the way the library runs it (normalise once, then a lookup per
// row, the listed pixel on a hit and the row's own otherwise).  With VIO_TEST_SANITIZE=1 it is built with ASan and UBSan.
//
//   in  (binary): int32 n, p, c; n int64 ids | n x 2 floats cur | p int64 prediction ids | p x 2 floats pixels |
//                 c x 3 int32 (guessed, n_ok, min_tracked)
//   out (binary): int32 m; m int64 sorted ids | m x 2 floats pixels | n int32 rows found | n x 2 floats guess | int32 n_guessed |
//                 c int32 falls back
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vio_front_guess_math.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[3];
    if (std::fread(head, sizeof(int32_t), 3, f) != 3 || head[0] < 0 || head[0] > FRONT_CAP || head[1] < 0 || head[1] > FRONT_CAP || head[2] < 0) return 4;
    const size_t N = (size_t)head[0], P = (size_t)head[1], C = (size_t)head[2];
    std::vector<long long> ids(N), pids(P), sids(P);
    std::vector<float> cur(2 * N), ppx(2 * P), spx(2 * P), guess(2 * N);
    std::vector<int32_t> cases(3 * C), found(N), falls(C);
    static_assert(sizeof(long long) == 8, "ids are int64");
    if ((N && (std::fread(ids.data(), 8, N, f) != N || std::fread(cur.data(), 4, 2 * N, f) != 2 * N)) ||
        (P && (std::fread(pids.data(), 8, P, f) != P || std::fread(ppx.data(), 4, 2 * P, f) != 2 * P)) ||
        (C && std::fread(cases.data(), 4, 3 * C, f) != 3 * C))
        return 5;
    std::fclose(f);
    const int32_t m = front_guess_normalise(pids.data(), ppx.data(), (int32_t)P, sids.data(), spx.data());
    int32_t n_guessed = 0;
    for (size_t t = 0; t < N; ++t) {
        const int32_t k = front_guess_find(sids.data(), m, ids[t]);
        found[t] = k;
        n_guessed += k >= 0 ? 1 : 0;
        guess[2 * t] = k >= 0 ? spx[2 * (size_t)k] : cur[2 * t];
        guess[2 * t + 1] = k >= 0 ? spx[2 * (size_t)k + 1] : cur[2 * t + 1];
    }
    for (size_t k = 0; k < C; ++k) falls[k] = front_guess_falls_back(cases[3 * k], cases[3 * k + 1], cases[3 * k + 2]) ? 1 : 0;
    f = std::fopen(argv[2], "wb");
    if (!f) return 6;
    std::fwrite(&m, 4, 1, f);
    if (m > 0) { std::fwrite(sids.data(), 8, (size_t)m, f); std::fwrite(spx.data(), 4, 2 * (size_t)m, f); }
    if (N) { std::fwrite(found.data(), 4, N, f); std::fwrite(guess.data(), 4, 2 * N, f); }
    std::fwrite(&n_guessed, 4, 1, f);
    if (C) std::fwrite(falls.data(), 4, C, f);
    return std::fclose(f) == 0 ? 0 : 7;
}
