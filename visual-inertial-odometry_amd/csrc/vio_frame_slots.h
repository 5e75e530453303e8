// vio_frame_slots.h — the host bookkeeping of libvio_frame_hip (include/vio_frame.h) with no HIP in it: the
// layout of a frame's levels, the pool of device blocks frames and masks live in, and the slot table with its roll, its geometry
// check and its invalidation.  vio_frame.hip gives the pool an allocator that calls hipMalloc; tests/cpp/frame_slots_main.cpp gives it
// one that calls malloc and runs a scripted sequence under ASan and UBSan (tests/test_frame_host_units.py).
// A slot also mirrors what the host knows of its resident points: the rows of its point table and of its
// prev_un table, which it learns from each read's read-back, the id counter, the frames read and the last time stamp.  The tables
// themselves are on the device; tests/cpp/front_math_main.cpp runs this part (tests/test_front_cpu.py).
//
// The pool never moves and never frees a block before it is destroyed: growing is adding a block.  A block is IN USE while the table
// refers to it and FREE otherwise; a free block is handed out again to a request it fits.  That is safe without waiting because every
// reader and the next writer of a block are enqueued on the handle's one stream, in call order.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int FRAME_MAX_SLOTS = 256;            // VIO_FRAME_MAX_SLOTS
constexpr int FRAME_MAX_LEVELS = 8;             // VIO_FLOW_MAX_LEVELS
constexpr int FRAME_MAX_DIM = 16384;            // VIO_FRAME_MAX_DIM
constexpr int FRAME_ALIGN = 256;                // of a block and of every level in it
constexpr int FRAME_MAX_TRACK_POINTS = 1024;    // VIO_FRAME_MAX_TRACK_POINTS

// outcomes of the checks, in the order they are made
enum FrameCheck { FRAME_OK = 0, FRAME_BAD_SLOT, FRAME_TWICE, FRAME_BAD_DIMS, FRAME_SMALL_LEVEL, FRAME_GEOMETRY, FRAME_TOO_FEW, FRAME_MASK_GEOMETRY,
                  FRAME_BAD_TIME, FRAME_BAD_POINTS };

inline int64_t frame_align(int64_t x) { return (x + FRAME_ALIGN - 1) / FRAME_ALIGN * FRAME_ALIGN; }

// Where the levels of a width x height frame lie in its block.  Level 0 has the pitch the CLAHE kernels need (a multiple of 4, with
// 4-byte accesses); the levels above are tightly packed.  A mask is a frame of one level.
struct FrameLayout {
    int32_t levels = 0;
    int32_t w[FRAME_MAX_LEVELS] = {0}, h[FRAME_MAX_LEVELS] = {0}, pitch[FRAME_MAX_LEVELS] = {0};
    int64_t off[FRAME_MAX_LEVELS] = {0};
    int64_t bytes = 0;
};

inline int32_t frame_pitch0(int32_t width) { return (width + 3) / 4 * 4; }

// false: a dimension outside [1, FRAME_MAX_DIM] or levels outside [1, FRAME_MAX_LEVELS] (FRAME_BAD_DIMS), or a level below 2 x 2
// (FRAME_SMALL_LEVEL, the rule of include/vio_flow.h); `why` says which.
inline bool frame_layout(int32_t width, int32_t height, int32_t levels, FrameLayout &L, FrameCheck *why = nullptr) {
    FrameCheck dummy;
    FrameCheck &r = why ? *why : dummy;
    r = FRAME_BAD_DIMS;
    if (width < 1 || height < 1 || width > FRAME_MAX_DIM || height > FRAME_MAX_DIM || levels < 1 || levels > FRAME_MAX_LEVELS) return false;
    L = FrameLayout();
    L.levels = levels;
    int64_t at = 0;
    for (int l = 0; l < levels; ++l) {
        L.w[l] = l ? L.w[l - 1] / 2 : width;
        L.h[l] = l ? L.h[l - 1] / 2 : height;
        r = FRAME_SMALL_LEVEL;
        if (L.w[l] < 2 || L.h[l] < 2) return false;
        L.pitch[l] = l ? L.w[l] : frame_pitch0(width);
        L.off[l] = at;
        at = frame_align(at + (int64_t)L.pitch[l] * L.h[l]);
    }
    L.bytes = at;
    r = FRAME_OK;
    return true;
}

// a mask's layout: one level at level 0's pitch, whatever its size (a 1 x 1 mask is a mask)
inline bool frame_mask_layout(int32_t width, int32_t height, FrameLayout &L) {
    if (width < 1 || height < 1 || width > FRAME_MAX_DIM || height > FRAME_MAX_DIM) return false;
    L = FrameLayout();
    L.levels = 1; L.w[0] = width; L.h[0] = height; L.pitch[0] = frame_pitch0(width);
    L.bytes = frame_align((int64_t)L.pitch[0] * height);
    return true;
}

struct FrameBlock {
    void *base = nullptr;
    int64_t bytes = 0;
    bool in_use = false;
};

struct FramePool {
    std::vector<FrameBlock> blocks;
    int64_t total = 0;                  // bytes of every block
    // A block of at least `bytes`: a free one that is not more than twice as large (the smallest such), else a new one from
    // alloc(bytes) -> address or nullptr.  -1: the allocator failed, nothing changed.
    template <class Alloc> int acquire(int64_t bytes, Alloc &&alloc) {
        int best = -1;
        for (int i = 0; i < (int)blocks.size(); ++i) {
            const FrameBlock &b = blocks[(size_t)i];
            if (b.in_use || b.bytes < bytes || b.bytes > 2 * bytes) continue;
            if (best < 0 || b.bytes < blocks[(size_t)best].bytes) best = i;
        }
        if (best < 0) {
            void *p = alloc(bytes);
            if (!p) return -1;
            FrameBlock b;
            b.base = p; b.bytes = bytes;
            blocks.push_back(b);
            total += bytes;
            best = (int)blocks.size() - 1;
        }
        blocks[(size_t)best].in_use = true;
        return best;
    }
    void release(int id) {
        if (id >= 0 && id < (int)blocks.size()) blocks[(size_t)id].in_use = false;
    }
    int in_use() const {
        int n = 0;
        for (const FrameBlock &b : blocks) n += b.in_use ? 1 : 0;
        return n;
    }
    // the owner frees every block with the allocator's counterpart, once nothing reads them any more
    template <class Free> void destroy(Free &&free_block) {
        for (FrameBlock &b : blocks) free_block(b.base);
        blocks.clear();
        total = 0;
    }
};

struct FrameSlot {
    int32_t n_frames = 0;               // 0, 1 (next alone) or 2
    int32_t width = 0, height = 0;      // of the resident frames; meaningful while n_frames > 0
    int prev = -1, next = -1;           // blocks
    int mask = -1;
    int32_t mask_w = 0, mask_h = 0;
    // the resident points (vio_frame_read_batch): rows of the slot's point table, which belong to its next frame, and of its prev_un
    // table; the next free id; the frames read (rejectWithF's `pair`); the time of the last one
    int32_t n_pts = 0, n_prev_un = 0;
    int64_t next_id = 0;
    uint32_t n_read = 0;
    double time = 0.0;
};

struct FrameTable {
    int32_t levels = 4;                 // VIO_FLOW_DEFAULT_LEVELS
    FrameSlot slots[FRAME_MAX_SLOTS];
    FramePool pool;

    static bool slot_ok(int32_t s) { return s >= 0 && s < FRAME_MAX_SLOTS; }

    // The checks of a push of `count` items, none of which changes anything.  FRAME_OK, or the first failing check with its item.
    FrameCheck check_push(int32_t count, const int32_t *slot, const int32_t *width, const int32_t *height, int32_t *bad) const {
        std::vector<uint8_t> seen((size_t)FRAME_MAX_SLOTS, 0);
        for (int32_t i = 0; i < count; ++i) {
            *bad = i;
            if (!slot_ok(slot[i])) return FRAME_BAD_SLOT;
            if (seen[(size_t)slot[i]]) return FRAME_TWICE;
            seen[(size_t)slot[i]] = 1;
            FrameLayout L;
            FrameCheck why;
            if (!frame_layout(width[i], height[i], levels, L, &why)) return why;
            const FrameSlot &s = slots[slot[i]];
            if (s.n_frames > 0 && (s.width != width[i] || s.height != height[i])) return FRAME_GEOMETRY;
        }
        *bad = -1;
        return FRAME_OK;
    }

    // The roll of one checked item: the block of the new frame, which is the slot's next from here on; the former next is its prev and
    // the former prev's block is free.  The new block is acquired before the old one is released, so the frame being written never
    // shares a block with the two a queued call may name.  -1: the allocator failed and the slot is as it was.
    template <class Alloc> int push(int32_t slot, int32_t width, int32_t height, Alloc &&alloc) {
        FrameLayout L;
        if (!slot_ok(slot) || !frame_layout(width, height, levels, L)) return -1;
        const int blk = pool.acquire(L.bytes, alloc);
        if (blk < 0) return -1;
        FrameSlot &s = slots[slot];
        pool.release(s.prev);
        s.prev = s.next;
        s.next = blk;
        s.n_pts = 0;                    // (the points were the rolled frame's; a read puts its own back: points_after_read)
        s.n_frames = s.n_frames < 2 ? s.n_frames + 1 : 2;
        s.width = width; s.height = height;
        return blk;
    }

    void reset(int32_t slot) {
        if (!slot_ok(slot)) return;
        FrameSlot &s = slots[slot];
        pool.release(s.prev);
        pool.release(s.next);
        s.prev = s.next = -1;
        s.n_frames = 0; s.width = s.height = 0;
        s.n_pts = s.n_prev_un = 0;      // (the id counter stays: ids are never handed out twice)
        s.n_read = 0; s.time = 0.0;
    }

    // a change of the levels drops every frame: its layout is another
    void set_levels(int32_t n) {
        if (n == levels) return;
        for (int32_t s = 0; s < FRAME_MAX_SLOTS; ++s) reset(s);
        levels = n;
    }

    // the slot's new mask block (-1: the allocator failed, the old mask stays); clear_mask drops it
    template <class Alloc> int set_mask(int32_t slot, int32_t width, int32_t height, Alloc &&alloc) {
        FrameLayout L;
        if (!slot_ok(slot) || !frame_mask_layout(width, height, L)) return -1;
        const int blk = pool.acquire(L.bytes, alloc);
        if (blk < 0) return -1;
        FrameSlot &s = slots[slot];
        pool.release(s.mask);
        s.mask = blk; s.mask_w = width; s.mask_h = height;
        return blk;
    }
    void clear_mask(int32_t slot) {
        if (!slot_ok(slot)) return;
        FrameSlot &s = slots[slot];
        pool.release(s.mask);
        s.mask = -1; s.mask_w = s.mask_h = 0;
    }

    FrameCheck check_track(int32_t slot) const {
        if (!slot_ok(slot)) return FRAME_BAD_SLOT;
        return slots[slot].n_frames < 2 ? FRAME_TOO_FEW : FRAME_OK;
    }
    FrameCheck check_detect(int32_t slot) const {
        if (!slot_ok(slot)) return FRAME_BAD_SLOT;
        const FrameSlot &s = slots[slot];
        if (s.n_frames < 1) return FRAME_TOO_FEW;
        if (s.mask >= 0 && (s.mask_w != s.width || s.mask_h != s.height)) return FRAME_MASK_GEOMETRY;
        return FRAME_OK;
    }
    // which: 0 prev, 1 next
    FrameCheck check_frame(int32_t slot, int32_t which, int32_t level) const {
        if (!slot_ok(slot)) return FRAME_BAD_SLOT;
        if ((which != 0 && which != 1) || level < 0 || level >= levels) return FRAME_BAD_DIMS;
        return slots[slot].n_frames < (which == 0 ? 2 : 1) ? FRAME_TOO_FEW : FRAME_OK;
    }

    // The checks of a read of `count` items besides check_push's, none of which changes anything: a time that is finite and, while the
    // slot's prev_un holds rows, after the slot's last; with `publish`, a mask of the frame's geometry.
    FrameCheck check_read(int32_t count, const int32_t *slot, const int32_t *width, const int32_t *height, const double *time, bool publish,
                          int32_t *bad) const {
        const FrameCheck ck = check_push(count, slot, width, height, bad);
        if (ck != FRAME_OK) return ck;
        for (int32_t i = 0; i < count; ++i) {
            *bad = i;
            const FrameSlot &s = slots[slot[i]];
            if (!std::isfinite(time[i]) || (s.n_prev_un > 0 && !(time[i] > s.time))) return FRAME_BAD_TIME;
            if (publish && s.mask >= 0 && (s.mask_w != width[i] || s.mask_h != height[i])) return FRAME_MASK_GEOMETRY;
        }
        *bad = -1;
        return FRAME_OK;
    }
    // what a read's read-back says of a slot: n rows in both tables, the counter, one more frame read
    void points_after_read(int32_t slot, int32_t n, int64_t next_id, double time) {
        if (!slot_ok(slot)) return;
        FrameSlot &s = slots[slot];
        s.n_pts = s.n_prev_un = n < 0 ? 0 : (n > FRAME_MAX_TRACK_POINTS ? FRAME_MAX_TRACK_POINTS : n);
        s.next_id = next_id;
        s.n_read += 1u;
        s.time = time;
    }
    // seeding a slot's points needs a frame they lie in
    FrameCheck check_points_set(int32_t slot, int32_t n) const {
        if (!slot_ok(slot)) return FRAME_BAD_SLOT;
        if (slots[slot].n_frames < 1) return FRAME_TOO_FEW;
        return n < 0 || n > FRAME_MAX_TRACK_POINTS ? FRAME_BAD_POINTS : FRAME_OK;
    }
    void points_set(int32_t slot, int32_t n) {
        if (check_points_set(slot, n) == FRAME_OK) slots[slot].n_pts = n;
    }

    // the address of level l of a block laid out by L
    uint8_t *level_ptr(int blk, const FrameLayout &L, int l) const { return (uint8_t *)pool.blocks[(size_t)blk].base + L.off[l]; }
};
