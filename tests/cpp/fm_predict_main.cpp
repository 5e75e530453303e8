// fm_predict_main.cpp — csrc/vio_fm_predict_math.h on the host, for tests/test_fm_predict_cpu.py: the text k_fm_predict compiles, run
// over one track list the way the kernel runs it (rows in list order, the qualifying ones compacted).  With VIO_TEST_SANITIZE=1 it is
// built with ASan and UBSan.
//
//   in  (binary): int32 frame_count, has_next; 77 doubles poses; 7 doubles ext; 7 doubles next_pose; int64 n;
//                 n int64 ids | n int32 start | n int32 n_obs | n doubles depth | n x 2 doubles first observation
//   out (binary): int64 rows; rows int64 ids | rows x 3 doubles pts_cam | 9 doubles R_next | 3 doubles P_next
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vio_fm_predict_math.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[2];
    double poses[7 * FM_MAX_OBS], ext[7], next[7];
    long long n = 0;
    if (std::fread(head, sizeof(int32_t), 2, f) != 2 || std::fread(poses, sizeof(double), 7 * FM_MAX_OBS, f) != 7 * FM_MAX_OBS ||
        std::fread(ext, sizeof(double), 7, f) != 7 || std::fread(next, sizeof(double), 7, f) != 7 || std::fread(&n, sizeof(n), 1, f) != 1 || n < 0 ||
        n > FM_MAX_TRACKS || head[0] < 0 || head[0] > FM_WINDOW)
        return 4;
    const size_t N = (size_t)n;
    std::vector<int64_t> ids(N);
    std::vector<int32_t> start(N), nobs(N);
    std::vector<double> depth(N), obs(2 * N);
    if (n > 0 && (std::fread(ids.data(), 8, N, f) != N || std::fread(start.data(), 4, N, f) != N || std::fread(nobs.data(), 4, N, f) != N ||
                  std::fread(depth.data(), 8, N, f) != N || std::fread(obs.data(), 8, 2 * N, f) != 2 * N))
        return 5;
    std::fclose(f);
    const int fc = head[0];
    double R[9 * FM_MAX_OBS], ric[9], Rn[9] = {0}, Pn[3] = {0};
    for (int k = 0; k < FM_MAX_OBS; ++k) fmp_quat_to_R(poses + 7 * k + 3, R + 9 * k);
    fmp_quat_to_R(ext + 3, ric);
    std::vector<int64_t> o_id;
    std::vector<double> o_pt;
    if (fc >= 2) {
        if (head[1]) {
            fmp_quat_to_R(next + 3, Rn);
            for (int k = 0; k < 3; ++k) Pn[k] = next[k];
        } else {
            fmp_next_pose(R + 9 * (fc - 1), poses + 7 * (fc - 1), R + 9 * fc, poses + 7 * fc, Rn, Pn);
        }
        for (size_t r = 0; r < N; ++r) {
            const int K = fm_clamp(nobs[r], 0, FM_MAX_OBS);
            if (!fmp_qualifies(depth[r], K, start[r], fc)) continue;
            double p[3];
            fmp_point(obs[2 * r], obs[2 * r + 1], depth[r], ric, ext, R + 9 * start[r], poses + 7 * start[r], Rn, Pn, p);
            o_id.push_back(ids[r]);
            o_pt.insert(o_pt.end(), p, p + 3);
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 6;
    const long long rows = (long long)o_id.size();
    std::fwrite(&rows, sizeof(rows), 1, f);
    if (rows > 0) {
        std::fwrite(o_id.data(), 8, o_id.size(), f);
        std::fwrite(o_pt.data(), 8, o_pt.size(), f);
    }
    std::fwrite(Rn, 8, 9, f);
    std::fwrite(Pn, 8, 3, f);
    return std::fclose(f) == 0 ? 0 : 7;
}
