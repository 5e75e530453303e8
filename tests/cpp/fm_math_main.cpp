// fm_math_main.cpp — the host build of the batched FeatureManager's arithmetic (csrc/vio_fm_math.h) driven by a script
// (tests/test_fm_cpu.py; with VIO_TEST_SANITIZE=1 under ASan and UBSan).  The compaction loop below walks a table the way a workgroup of
// vio_fm_body.inc does: chunks of FM_NT rows, row r of a chunk belongs to wavefront r / 64, lane r % 64; a ballot per wavefront, the
// wavefront counts, then every kept row's destination from the chunk's base.
//
//   in (text), one operation per line:
//     K n (keep) x n                                   the destinations of a stable compaction: "K total" then dest (-1: dropped) per row
//     S kind frame_count n (start n_obs) x n           fm_slide_row: "S" then "start erase keep shift" per row
//     U n (start n_obs) x n                            fm_usable: "U" then 0 / 1 per row
//     P frame_count start n_obs xi yi xj yj            fm_parallax_row and fm_parallax: "P take term" (term as a hex double)
//     D x y depth mR(9) mP(3) nR(9) nP(3) init         fm_shift_depth: "D depth" (hex double)
//   doubles are read with %la and written with %a: bit for bit.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vio_fm_math.h"

static int compact(const std::vector<int> &keep, std::vector<int32_t> &dest) {
    const int n = (int)keep.size();
    dest.assign((size_t)n, -1);
    int base = 0;
    for (int c = 0; c * FM_NT < n; ++c) {
        uint64_t ballot[FM_WAVES] = {0};
        int32_t counts[FM_WAVES] = {0};
        for (int t = 0; t < FM_NT && c * FM_NT + t < n; ++t)
            if (keep[(size_t)(c * FM_NT + t)]) ballot[t / FM_WAVE] |= 1ull << (t % FM_WAVE);
        for (int w = 0; w < FM_WAVES; ++w) counts[w] = fm_wave_count(ballot[w]);
        for (int t = 0; t < FM_NT && c * FM_NT + t < n; ++t)
            if (keep[(size_t)(c * FM_NT + t)]) dest[(size_t)(c * FM_NT + t)] = fm_dest(base, counts, t / FM_WAVE, ballot[t / FM_WAVE], t % FM_WAVE);
        base += fm_wave_base(counts, FM_WAVES);
    }
    return base;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "r"), *o = std::fopen(argv[2], "w");
    if (!f || !o) return 2;
    char op;
    while (std::fscanf(f, " %c", &op) == 1) {
        if (op == 'K') {
            int n = 0;
            if (std::fscanf(f, "%d", &n) != 1 || n < 0 || n > FM_MAX_TRACKS) return 2;
            std::vector<int> keep((size_t)n);
            for (int &k : keep)
                if (std::fscanf(f, "%d", &k) != 1) return 2;
            std::vector<int32_t> dest;
            std::fprintf(o, "K %d", compact(keep, dest));
            for (int32_t d : dest) std::fprintf(o, " %d", d);
            std::fprintf(o, "\n");
        } else if (op == 'S') {
            int kind = 0, fc = 0, n = 0;
            if (std::fscanf(f, "%d %d %d", &kind, &fc, &n) != 3 || n < 0) return 2;
            std::fprintf(o, "S");
            for (int i = 0; i < n; ++i) {
                int start = 0, k = 0;
                if (std::fscanf(f, "%d %d", &start, &k) != 2) return 2;
                const FmSlide s = fm_slide_row(kind, fc, start, k);
                std::fprintf(o, " %d %d %d %d", s.start, s.erase, s.keep, s.shift);
            }
            std::fprintf(o, "\n");
        } else if (op == 'U') {
            int n = 0;
            if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
            std::fprintf(o, "U");
            for (int i = 0; i < n; ++i) {
                int start = 0, k = 0;
                if (std::fscanf(f, "%d %d", &start, &k) != 2) return 2;
                std::fprintf(o, " %d", fm_usable(start, k) ? 1 : 0);
            }
            std::fprintf(o, "\n");
        } else if (op == 'P') {
            int fc = 0, start = 0, k = 0;
            double v[4];
            if (std::fscanf(f, "%d %d %d %la %la %la %la", &fc, &start, &k, &v[0], &v[1], &v[2], &v[3]) != 7) return 2;
            std::fprintf(o, "P %d %a\n", fm_parallax_row(fc, start, k) ? 1 : 0, fm_parallax(v[0], v[1], v[2], v[3]));
        } else if (op == 'D') {
            double v[28];
            for (double &x : v)
                if (std::fscanf(f, "%la", &x) != 1) return 2;
            std::fprintf(o, "D %a\n", fm_shift_depth(v[0], v[1], v[2], v + 3, v + 12, v + 15, v + 24, v[27]));
        } else {
            return 2;
        }
    }
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
