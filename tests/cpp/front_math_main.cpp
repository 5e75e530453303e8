// front_math_main.cpp — the host build of the join's index arithmetic (csrc/vio_front_math.h) and the point bookkeeping of the slot
// table (csrc/vio_frame_slots.h) driven by a script, with malloc for hipMalloc (tests/test_front_cpu.py; with VIO_TEST_SANITIZE=1 under
// ASan and UBSan).  The loops below walk a table the way a workgroup of vio_front_body.inc does: row r belongs to wavefront r / 64, lane
// r % 64; a ballot per wavefront, the wavefront counts, then every row's destination.
//
//   in (text), one operation per line:
//     K border w h n (x y status) x n     k_front_filter's decision and compaction: "K nk" then "keep dest" per row
//     U n (id) x n                        k_front_finish's ids: prev_un takes the ids as they are, then updateID from the program's
//                                         counter: "U counter" then "prev_un_id new_id" per row
//     E publish n (slot w h time rows next_id) x n     check_read; if it passes, push and points_after_read of every item
//     P slot w h                          a direct push (check_push, push)
//     S slot n                            check_points_set, points_set
//     R slot      L levels      M slot w h      C slot          reset, set_levels, set_mask, clear_mask
//   out: after E, P, S, R, L, M, C: the letter, the outcome (a FrameCheck; -1: the allocator failed), the failing item (or -1), then every
//   slot that holds something as "slot s n_frames n_pts n_prev_un next_id n_read time".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vio_frame_slots.h"
#include "vio_front_math.h"

static void *host_block(int64_t bytes) { return std::malloc((size_t)bytes); }

// the destinations of the kept rows among n <= FRONT_CAP, and their total
static int compact(const std::vector<uint8_t> &keep, std::vector<int32_t> &dest) {
    const int n = (int)keep.size();
    uint64_t ballot[FRONT_WAVES] = {0};
    int32_t counts[FRONT_WAVES] = {0};
    for (int r = 0; r < n; ++r)
        if (keep[(size_t)r]) ballot[r / FRONT_WAVE] |= 1ull << (r % FRONT_WAVE);
    for (int w = 0; w < FRONT_WAVES; ++w) counts[w] = front_wave_count(ballot[w]);
    dest.assign((size_t)n, -1);
    for (int r = 0; r < n; ++r)
        if (keep[(size_t)r]) dest[(size_t)r] = front_wave_base(counts, r / FRONT_WAVE) + front_lane_rank(ballot[r / FRONT_WAVE], r % FRONT_WAVE);
    return front_wave_base(counts, FRONT_WAVES);
}

static void print_table(FILE *o, const FrameTable &t) {
    for (int s = 0; s < FRAME_MAX_SLOTS; ++s) {
        const FrameSlot &f = t.slots[s];
        if (f.n_frames == 0 && f.n_pts == 0 && f.n_prev_un == 0 && f.next_id == 0 && f.n_read == 0) continue;
        std::fprintf(o, " slot %d %d %d %d %lld %u %.17g", s, f.n_frames, f.n_pts, f.n_prev_un, (long long)f.next_id, f.n_read, f.time);
    }
    std::fprintf(o, "\n");
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "r"), *o = std::fopen(argv[2], "w");
    if (!f || !o) return 2;
    FrameTable *t = new FrameTable();
    long long counter = 0;
    char op;
    while (std::fscanf(f, " %c", &op) == 1) {
        int code = 0, bad = -1;
        if (op == 'K') {
            int b = 0, w = 0, h = 0, n = 0;
            if (std::fscanf(f, "%d %d %d %d", &b, &w, &h, &n) != 4 || n < 0 || n > FRONT_CAP) return 2;
            std::vector<uint8_t> keep((size_t)n);
            for (int r = 0; r < n; ++r) {
                float x = 0.f, y = 0.f;
                int status = 0;
                if (std::fscanf(f, "%f %f %d", &x, &y, &status) != 3) return 2;
                keep[(size_t)r] = status == 0 && front_in_border(x, y, w, h, b);
            }
            std::vector<int32_t> dest;
            std::fprintf(o, "K %d", compact(keep, dest));
            for (int r = 0; r < n; ++r) std::fprintf(o, " %d %d", (int)keep[(size_t)r], dest[(size_t)r]);
            std::fprintf(o, "\n");
            continue;
        }
        if (op == 'U') {
            int n = 0;
            if (std::fscanf(f, "%d", &n) != 1 || n < 0 || n > FRONT_CAP) return 2;
            std::vector<long long> ids((size_t)n), prev_un((size_t)n);
            std::vector<uint8_t> fresh((size_t)n);
            for (int r = 0; r < n; ++r) {
                if (std::fscanf(f, "%lld", &ids[(size_t)r]) != 1) return 2;
                fresh[(size_t)r] = ids[(size_t)r] == -1;
            }
            std::vector<int32_t> rank;
            const int n_fresh = compact(fresh, rank);
            for (int r = 0; r < n; ++r) {
                prev_un[(size_t)r] = ids[(size_t)r];                                    // before updateID: the kept quirk
                ids[(size_t)r] = front_new_id(ids[(size_t)r], counter, rank[(size_t)r]);
            }
            counter += n_fresh;
            std::fprintf(o, "U %lld", counter);
            for (int r = 0; r < n; ++r) std::fprintf(o, " %lld %lld", prev_un[(size_t)r], ids[(size_t)r]);
            std::fprintf(o, "\n");
            continue;
        }
        if (op == 'E') {
            int publish = 0, n = 0;
            if (std::fscanf(f, "%d %d", &publish, &n) != 2 || n < 0 || n > FRAME_MAX_SLOTS) return 2;
            std::vector<int32_t> s((size_t)n), w((size_t)n), h((size_t)n), rows((size_t)n);
            std::vector<double> time((size_t)n);
            std::vector<long long> next((size_t)n);
            for (int i = 0; i < n; ++i)
                if (std::fscanf(f, "%d %d %d %lf %d %lld", &s[(size_t)i], &w[(size_t)i], &h[(size_t)i], &time[(size_t)i], &rows[(size_t)i],
                                &next[(size_t)i]) != 6) return 2;
            code = t->check_read(n, s.data(), w.data(), h.data(), time.data(), publish != 0, &bad);
            for (int i = 0; code == FRAME_OK && i < n; ++i) {
                if (t->push(s[(size_t)i], w[(size_t)i], h[(size_t)i], host_block) < 0) { code = -1; bad = i; break; }
                t->points_after_read(s[(size_t)i], rows[(size_t)i], next[(size_t)i], time[(size_t)i]);
            }
        } else if (op == 'P') {
            int32_t s = 0, w = 0, h = 0;
            if (std::fscanf(f, "%d %d %d", &s, &w, &h) != 3) return 2;
            code = t->check_push(1, &s, &w, &h, &bad);
            if (code == FRAME_OK && t->push(s, w, h, host_block) < 0) code = -1;
        } else if (op == 'S') {
            int s = 0, n = 0;
            if (std::fscanf(f, "%d %d", &s, &n) != 2) return 2;
            code = t->check_points_set(s, n);
            t->points_set(s, n);
        } else if (op == 'R' || op == 'C' || op == 'L') {
            int v = 0;
            if (std::fscanf(f, "%d", &v) != 1) return 2;
            if (op == 'R') t->reset(v);
            if (op == 'C') t->clear_mask(v);
            if (op == 'L') {
                if (v < 1 || v > FRAME_MAX_LEVELS) return 2;
                t->set_levels(v);
            }
        } else if (op == 'M') {
            int s = 0, w = 0, h = 0;
            if (std::fscanf(f, "%d %d %d", &s, &w, &h) != 3) return 2;
            code = t->set_mask(s, w, h, host_block) < 0 ? -1 : 0;
        } else {
            return 2;
        }
        std::fprintf(o, "%c %d %d", op, code, bad);
        print_table(o, *t);
    }
    t->pool.destroy([](void *p) { std::free(p); });
    delete t;
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
