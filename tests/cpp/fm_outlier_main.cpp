// fm_outlier_main.cpp — csrc/vio_fm_outlier_math.h on the host, for tests/test_fm_outlier_cpu.py: the text k_fm_remove and
// vio_fm_remove_batch compile.  Usage: fm_outlier <in> <out>; one output line per input line.
//   Q n id[n] m key[m]   ->   Q distinct perm[n] lower_bound[m] find[m] erased[n]
// ids: the caller's list, sorted here with fm_sort_ids; every key is bisected in the sorted list; a hit byte is set per id a key
// found, and the hit bytes go back to the caller's order (fm_unpermute_hits).  Every array is allocated at its exact length.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "vio_fm_outlier_math.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string op, tok;
        ss >> op;
        if (op != "Q") return 3;
        int n = 0, m = 0;
        ss >> n;
        std::vector<int64_t> ids((size_t)n), sorted((size_t)n);
        std::vector<int32_t> perm((size_t)n);
        for (int i = 0; i < n; ++i) { ss >> tok; ids[(size_t)i] = (int64_t)std::strtoll(tok.c_str(), nullptr, 10); }
        ss >> m;
        std::vector<int64_t> keys((size_t)m);
        for (int i = 0; i < m; ++i) { ss >> tok; keys[(size_t)i] = (int64_t)std::strtoll(tok.c_str(), nullptr, 10); }
        if (!ss) return 4;
        const bool distinct = fm_sort_ids(ids.data(), n, sorted.data(), perm.data());
        out << "Q " << (distinct ? 1 : 0);
        for (int i = 0; i < n; ++i) out << ' ' << perm[(size_t)i];
        std::vector<uint8_t> hit((size_t)n, 0), erased((size_t)n, 7);
        std::vector<int32_t> found((size_t)m);
        for (int i = 0; i < m; ++i) out << ' ' << fm_id_lower_bound(sorted.data(), n, keys[(size_t)i]);
        for (int i = 0; i < m; ++i) {
            found[(size_t)i] = fm_id_find(sorted.data(), n, keys[(size_t)i]);
            if (found[(size_t)i] >= 0) hit[(size_t)found[(size_t)i]] = 1;
            out << ' ' << found[(size_t)i];
        }
        fm_unpermute_hits(hit.data(), perm.data(), n, erased.data());
        for (int i = 0; i < n; ++i) out << ' ' << (int)erased[(size_t)i];
        out << '\n';
    }
    return 0;
}
