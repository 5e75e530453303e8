// frame_slots_main.cpp — the host bookkeeping of libvio_frame_hip (csrc/vio_frame_slots.h) driven by a script, with malloc for
// hipMalloc (tests/test_frame_host_units.py; with VIO_TEST_SANITIZE=1 under ASan and UBSan).
//
//   in (text), one operation per line:
//     P n (slot w h) x n     a push of n items: check_push, then, if it passed, push of each item and a write of every level's bytes
//     R slot                 reset            L levels   set_levels
//     M slot w h             set_mask (and a write of its bytes)            C slot   clear_mask
//     T slot                 check_track      D slot     check_detect       F slot which level   check_frame
//     Y w h levels           frame_layout
//   out (text), one line per operation: the operation's letter, its outcome (a FrameCheck; -1 after P, M: the allocator failed) and
//   the failing item (or -1); then "blocks in_use count total"; then every slot that holds something as
//   "slot n_frames width height prev next mask mask_w mask_h".  Y prints "levels bytes" and "w h pitch off" per level instead.
// After every operation the program itself checks what a line cannot show: no block has moved or shrunk, and no two references of the
// table name one block.  A violation ends it with status 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "vio_frame_slots.h"

static void *host_block(int64_t bytes) { return std::malloc((size_t)bytes); }

static void write_frame(FrameTable &t, int blk, const FrameLayout &L, int value) {
    for (int l = 0; l < L.levels; ++l) std::memset(t.level_ptr(blk, L, l), value, (size_t)L.pitch[l] * (size_t)L.h[l]);
}

static bool consistent(const FrameTable &t, std::vector<FrameBlock> &seen) {
    for (size_t i = 0; i < seen.size(); ++i)
        if (i >= t.pool.blocks.size() || t.pool.blocks[i].base != seen[i].base || t.pool.blocks[i].bytes != seen[i].bytes) return false;
    seen = t.pool.blocks;
    std::set<int> refs;
    int n = 0;
    for (int s = 0; s < FRAME_MAX_SLOTS; ++s) {
        const FrameSlot &f = t.slots[s];
        const int ids[3] = {f.n_frames == 2 ? f.prev : -1, f.n_frames >= 1 ? f.next : -1, f.mask};
        if ((f.n_frames < 2 && f.prev != -1) || (f.n_frames < 1 && f.next != -1)) return false;
        for (int id : ids) {
            if (id < 0) continue;
            if (id >= (int)t.pool.blocks.size() || !t.pool.blocks[(size_t)id].in_use || !refs.insert(id).second) return false;
            n += 1;
        }
    }
    return n == t.pool.in_use();
}

static void print_table(FILE *o, const FrameTable &t) {
    std::fprintf(o, " blocks %d %d %lld", t.pool.in_use(), (int)t.pool.blocks.size(), (long long)t.pool.total);
    for (int s = 0; s < FRAME_MAX_SLOTS; ++s) {
        const FrameSlot &f = t.slots[s];
        if (f.n_frames == 0 && f.mask < 0) continue;
        std::fprintf(o, " slot %d %d %d %d %d %d %d %d %d", s, f.n_frames, f.width, f.height, f.prev, f.next, f.mask, f.mask_w, f.mask_h);
    }
    std::fprintf(o, "\n");
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "r"), *o = std::fopen(argv[2], "w");
    if (!f || !o) return 2;
    FrameTable *t = new FrameTable();
    std::vector<FrameBlock> seen;
    char op;
    int writes = 0;
    while (std::fscanf(f, " %c", &op) == 1) {
        int code = 0, bad = -1;
        if (op == 'P') {
            int n = 0;
            if (std::fscanf(f, "%d", &n) != 1 || n < 0 || n > 4096) return 2;
            std::vector<int32_t> s((size_t)n), w((size_t)n), h((size_t)n);
            for (int i = 0; i < n; ++i)
                if (std::fscanf(f, "%d %d %d", &s[(size_t)i], &w[(size_t)i], &h[(size_t)i]) != 3) return 2;
            code = t->check_push(n, s.data(), w.data(), h.data(), &bad);
            for (int i = 0; code == FRAME_OK && i < n; ++i) {
                const int blk = t->push(s[(size_t)i], w[(size_t)i], h[(size_t)i], host_block);
                if (blk < 0) { code = -1; bad = i; break; }
                FrameLayout L;
                frame_layout(w[(size_t)i], h[(size_t)i], t->levels, L);
                write_frame(*t, blk, L, ++writes & 255);
            }
        } else if (op == 'R' || op == 'C' || op == 'T' || op == 'D') {
            int s = 0;
            if (std::fscanf(f, "%d", &s) != 1) return 2;
            if (op == 'R') t->reset(s);
            if (op == 'C') t->clear_mask(s);
            if (op == 'T') code = t->check_track(s);
            if (op == 'D') code = t->check_detect(s);
        } else if (op == 'L') {
            int n = 0;
            if (std::fscanf(f, "%d", &n) != 1 || n < 1 || n > FRAME_MAX_LEVELS) return 2;
            t->set_levels(n);
        } else if (op == 'M') {
            int s = 0, w = 0, h = 0;
            if (std::fscanf(f, "%d %d %d", &s, &w, &h) != 3) return 2;
            const int blk = t->set_mask(s, w, h, host_block);
            code = blk < 0 ? -1 : 0;
            FrameLayout L;
            if (blk >= 0 && frame_mask_layout(w, h, L)) write_frame(*t, blk, L, ++writes & 255);
        } else if (op == 'F') {
            int s = 0, which = 0, level = 0;
            if (std::fscanf(f, "%d %d %d", &s, &which, &level) != 3) return 2;
            code = t->check_frame(s, which, level);
        } else if (op == 'Y') {
            int w = 0, h = 0, levels = 0;
            if (std::fscanf(f, "%d %d %d", &w, &h, &levels) != 3) return 2;
            FrameLayout L;
            FrameCheck why;
            const bool ok = frame_layout(w, h, levels, L, &why);
            std::fprintf(o, "Y %d -1 layout %d %lld", (int)why, ok ? L.levels : 0, (long long)(ok ? L.bytes : 0));
            for (int l = 0; ok && l < L.levels; ++l) std::fprintf(o, " %d %d %d %lld", L.w[l], L.h[l], L.pitch[l], (long long)L.off[l]);
            std::fprintf(o, "\n");
            continue;
        } else {
            return 2;
        }
        if (!consistent(*t, seen)) return 3;
        std::fprintf(o, "%c %d %d", op, code, bad);
        print_table(o, *t);
    }
    t->pool.destroy([](void *p) { std::free(p); });
    delete t;
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
