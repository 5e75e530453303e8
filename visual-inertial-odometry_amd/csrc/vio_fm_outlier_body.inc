// vio_fm_outlier_body.inc — the kernel of include/vio_fm_outlier.h (DESIGN.md section 34), included behind vio_fm_stream_body.inc; it
// uses vio_fm_body.inc's table, descriptors, row loads and stores, scan and counts.  One workgroup of FM_NT threads per item of the
// call, which is one slot's table:
//   k_fm_remove          removeOutlier by id: the item's ids, sorted by the host, are staged in LDS with a cleared hit byte each; the
//                        rows are walked in chunks of FM_NT, every thread bisects its row's id among them (vio_fm_outlier_math.h) and
//                        a row whose id is found is dropped and sets that id's hit byte.  The rows that stay are compacted in place as
//                        k_fm_set_depth's removeFailures branch compacts them: whole rows in registers, the scan's barriers between
//                        a chunk's loads and any store, rows only move down, a row is stored only where its index changes.  A chunk
//                        in front of the first erased row is neither loaded beyond its ids nor written.
// Integers and copies only: no floating-point operation, no atomics (a hit byte is written by the one row that has its id; if a
// corrupted table held an id twice both rows would store the same 1).  Every count read from device memory is held to the rows and
// ids there are before it indexes anything.  The hit bytes go to the call's read-back in sorted order; the host un-permutes them.

__global__ __launch_bounds__(FM_NT) void k_fm_remove(FmArgs a) {
    __shared__ int64_t s_id[FM_MAX_TRACKS];
    __shared__ uint8_t s_hit[FM_MAX_TRACKS];
    __shared__ int32_t s_w[FM_WAVES], s_cnt[2];
    const int item = blockIdx.x, t = threadIdx.x;
    const FmItemD &I = a.items[item];
    const FmTab T = fm_tab(I.tab);
    const int n = fm_clamp(I.n_tracks, 0, FM_MAX_TRACKS), nid = fm_clamp(I.b, 0, FM_MAX_TRACKS);
    const int64_t *ids = (const int64_t *)(a.in + I.o_in);
    vio_fm_result &R = a.res[item];
    if (t == 0) fm_result_clear(R);
    for (int k = t; k < FM_MAX_TRACKS; k += FM_NT) {
        s_hit[k] = 0;
        if (k < nid) s_id[k] = ids[k];
    }
    __syncthreads();
    int n1 = 0;
    for (int c = 0; c * FM_NT < n; ++c) {
        const int r = c * FM_NT + t;
        int found = -1;
        if (r < n) found = fm_id_find(s_id, nid, (int64_t)T.id[r]);
        const bool keep = r < n && found < 0;
        if (found >= 0) s_hit[found] = 1;
        // (uniform) the chunk's rows move only if a row in front of them went or one of its own goes
        const bool moves = __syncthreads_or(r < n && !keep) != 0 || n1 != c * FM_NT;
        FmRow W;
        if (moves && keep) fm_row_load(T, r, W);
        int tot;
        const int dst = n1 + fm_scan(keep, s_w, tot);      // (its barriers: every load of the chunk before any store)
        if (moves && keep && dst != r) fm_row_store(T, dst, W);
        n1 += tot;
    }
    fm_counts(T, n1, s_cnt, R);                             // (its barriers: the hit bytes are all written)
    if (t == 0) R.n_rows = n - n1;
    uint8_t *o = (uint8_t *)(a.out + I.o_out);
    for (int k = t; k < nid; k += FM_NT) o[k] = s_hit[k];
}
