// vio_front_guess_body.inc — the prediction in the device-side join of vio_frame_read_batch (include/vio_frame_predict.h, DESIGN.md
// section 39): three kernels that stand between k_front_begin, k_flow_track and k_front_filter when a listed slot has a pending
// prediction.  vio_frame.hip includes this text behind vio_front_body.inc, in the same two places; it reads FrontItem, kf::FlowPt and
// kf::FlowOut only, so both instantiations are the same text.
//
// One workgroup of FRONT_CAP threads per item of the call (blockIdx.x), one thread per row of the slot's point table.
//   k_front_guess      a guessed item: the item's sorted prediction ids into LDS, a bisection per row (front_guess_find), and the
//                      row's FlowPt gets has_guess = 1 with the listed pixel on a hit and the row's own pixel otherwise; n_guessed.
//                      An item that is not guessed keeps the rows k_front_begin wrote.
//   k_front_fallback   the rows of the guessed pass with status 0, the decision (front_guess_falls_back), and with a second list to
//                      write: the rows again without a guess for an item that falls back, rows with a NaN keypoint (k_flow_track
//                      leaves such a wavefront at its first branch) for every other
//   k_front_take       the second pass's FlowOut rows over the first's, for the items that fell back
// Counts are ballots and sixteen integer sums (front_scan), as in vio_front_body.inc: no atomics, every order is fixed.  Every count
// read from device memory is held to the rows there are before it indexes anything.
struct GuessItem {
    int32_t off, m;                     // the item's first row in the call's prediction ids and pixels, and its rows
    int32_t guessed;                    // 1: the slot had a pending prediction and points to track
    int32_t pad;
};

struct GuessRes {
    int32_t n_guessed, n_ok_guessed, fell_back, pad;
};

struct GuessArgs {
    const FrontItem *items;
    const GuessItem *gitems;
    const long long *gids;              // [g_rows], per item ascending and distinct
    const float *gpx;                   // [g_rows][2]
    kf::FlowPt *fpts;
    kf::FlowPt *fpts2;                  // the second pass's list, or nullptr: no fallback is armed, k_front_fallback counts only
    kf::FlowOut *fout;
    const kf::FlowOut *fout2;
    GuessRes *gres;
    int32_t g_rows, min_tracked;
};

__global__ __launch_bounds__(FNT) void k_front_guess(GuessArgs a) {
    __shared__ long long s_ids[FRONT_CAP];
    __shared__ int32_t s_w[FRONT_WAVES];
    const int item = blockIdx.x, t = threadIdx.x;
    const FrontItem &I = a.items[item];
    const GuessItem G = a.gitems[item];
    if (!G.guessed) {                                       // (uniform: the whole workgroup leaves before a barrier)
        if (t == 0) { GuessRes r = {0, 0, 0, 0}; a.gres[item] = r; }
        return;
    }
    const int n = front_clamp(I.n, 0, FRONT_CAP);
    const int off = front_clamp(G.off, 0, a.g_rows), m = front_clamp(G.m, 0, front_clamp(a.g_rows - off, 0, FRONT_CAP));
    if (t < m) s_ids[t] = a.gids[off + t];
    __syncthreads();
    bool hit = false;
    if (t < n) {
        const int k = front_guess_find(s_ids, m, I.ids[t]);
        hit = k >= 0;
        kf::FlowPt p;
        p.item = (int32_t)blockIdx.x; p.has_guess = 1;
        p.px = I.cur_pts[2 * t]; p.py = I.cur_pts[2 * t + 1];
        p.gx = hit ? a.gpx[2 * (off + k)] : p.px; p.gy = hit ? a.gpx[2 * (off + k) + 1] : p.py;
        a.fpts[I.flow_off + t] = p;
    }
    int n_hit;
    (void)front_scan(hit, s_w, n_hit);
    if (t == 0) { GuessRes r = {n_hit, 0, 0, 0}; a.gres[item] = r; }
}

__global__ __launch_bounds__(FNT) void k_front_fallback(GuessArgs a) {
    __shared__ int32_t s_w[FRONT_WAVES];
    const int item = blockIdx.x, t = threadIdx.x;
    const FrontItem &I = a.items[item];
    const int guessed = a.gitems[item].guessed;
    const int n = front_clamp(I.n, 0, FRONT_CAP);
    const bool ok = t < n && a.fout[I.flow_off + t].status == 0;
    int n_ok;
    (void)front_scan(ok, s_w, n_ok);
    const bool again = front_guess_falls_back(guessed, n_ok, a.min_tracked);
    if (a.fpts2 && t < n) {
        kf::FlowPt p;
        p.item = (int32_t)blockIdx.x; p.has_guess = 0;
        p.px = again ? I.cur_pts[2 * t] : NAN; p.py = again ? I.cur_pts[2 * t + 1] : NAN;
        p.gx = 0.f; p.gy = 0.f;
        a.fpts2[I.flow_off + t] = p;
    }
    if (t == 0) {
        a.gres[item].n_ok_guessed = guessed ? n_ok : 0;
        a.gres[item].fell_back = again ? 1 : 0;
    }
}

__global__ __launch_bounds__(FNT) void k_front_take(GuessArgs a) {
    const int item = blockIdx.x, t = threadIdx.x;
    const FrontItem &I = a.items[item];
    if (!a.gres[item].fell_back || t >= front_clamp(I.n, 0, FRONT_CAP)) return;
    a.fout[I.flow_off + t] = a.fout2[I.flow_off + t];
}
