// vio_front_body.inc — the device-side join of FeatureTracker::readImage's steps (include/vio_frame.h, DESIGN.md section 24): five
// kernels that stand where frontend.FeatureTracker has numpy between its four calls.  vio_frame.hip includes it after the bodies of
// the flow (kf), detect (kd) and reject (kr) kernels, whose descriptor tables these kernels read and write in device memory.
//
// One workgroup of FRONT_CAP = 1024 threads per item of the call (blockIdx.x), one thread per row of the slot's point table.
//   k_front_begin          the FlowPt rows of the slot's cur_pts (no guess), at the item's offset of the call's flat keypoint list
//   k_front_filter         keep a row when the tracker found it (status 0) and it rounds inside the border; compact; track_cnt + 1;
//                          the pair's RejPair (n, active, finite) and its staged cur | forw floats; with the forward-backward check
//                          (include/vio_frame_back.h) the counts of the rows it ran on and of those it failed
//   k_front_after_reject   compact by k_reject_ransac's mask (an inactive pair keeps every row); DetItemD.n_tracked and the DetTrk rows
//   k_front_merge          the kept rows in keep_order, then new_pts with id -1 and count 1; the LiftItem (n, m) with its staged points
//                          and ids, the slot's prev_un behind them
//   k_front_finish         prev_un := (ids, un_pts) as they are now, then updateID in row order from the slot's counter; the slot's
//                          cur_pts, ids and track_cnt; the packed result rows
// A compaction is stable: a ballot per wavefront, the sixteen wavefront counts through LDS, every thread adds the counts before its
// own (front_scan; the arithmetic is csrc/vio_front_math.h's).  Integers and float copies only, no atomics: every order is fixed.
// Every count a kernel reads from device memory is held to the rows there are before it indexes anything.
//
// The including file names the namespace of the reject tables as FRONT_REJ.  vio_frame.hip includes this text twice: at file scope with
// FRONT_REJ = kr (the PINHOLE tables of vio_reject_host.h), and inside namespace fq with FRONT_REJ = kq (the tables of
// vio_camera_host.h, a camera slot in each) and FRONT_CAMERAS defined (DESIGN.md section 29).  With FRONT_CAMERAS k_front_finish folds
// the flag bytes k_reject_lift left: one bad lift makes every un_pts and velocity of the slot NaN, in the rows and in prev_un, which is
// what vio_camera_undistort_batch does to the item on the host.  k_front_after_reject needs nothing more: a pair whose prologue found
// a bad lift is active, its mask is all zeros and its result says VIO_ERR_NOT_FINITE with hyp -1, so every row goes and the status is
// reported; the keep-everything branch is the inactive pair's alone.
constexpr int FNT = FRONT_CAP;
static_assert(FNT == 1024 && FNT % FRONT_WAVE == 0, "a slot's table is one workgroup of whole wavefronts");

struct FrontItem {
    float *cur_pts;                     // the slot's table: [FRONT_CAP][2]
    long long *ids;                     // [FRONT_CAP]
    int32_t *cnt;                       // [FRONT_CAP]
    long long *prev_un_ids;             // [FRONT_CAP]
    float *prev_un_pts;                 // [FRONT_CAP][2]
    long long *next_id;                 // the slot's next free id
    int32_t n, m;                       // rows of cur_pts and of prev_un when the call began (the host's mirror)
    int32_t w, h;
    int32_t flow_off;                   // the item's first row in the call's FlowPt and FlowOut
    int32_t pad;
};

struct FrontRes {
    int32_t n, n_new, n_tracked_in, n_after_track, n_after_reject, reject_status, reject_hyp, n_candidates;
    long long next_id;
#ifdef FRONT_CAMERAS
    int32_t n_clamped, n_bad;           // of the undistort stage: the clamped points (0 where a lift is bad), the bad lifts
#endif
    int32_t n_checked, n_back_lost, n_back_far, pad_back;      // of the forward-backward check (0 with it off)
};

struct FrontArgs {
    const FrontItem *items;
    kf::FlowPt *fpts;
    const kf::FlowOut *fout;
    FRONT_REJ::RejPair *pairs;
    float *rstage;                      // k_reject_ransac's staged floats
    const uint8_t *rmask;
    const FRONT_REJ::RejRes *rres;
    float *fa;                          // after the filter, item i at row i * FRONT_CAP: forw [2], ids, track_cnt
    long long *ida;
    int32_t *cnta;
    float *fb;                          // after the reject
    long long *idb;
    int32_t *cntb;
    kd::DetItemD *ditems;
    kd::DetTrk *dtrk;
    const kd::DetRes *dres;
    const int32_t *keep_order;
    const float *new_pts;
    FRONT_REJ::LiftItem *litems;
    float *lstage;                      // k_reject_lift's staged floats and ids
    long long *lids;
    const float *un, *vel;
    int32_t *cntm;                      // the merged track_cnt
    FrontRes *res;
    char *rows;                         // the packed result rows, item i at i * row_bytes: ids | pts | un_pts | velocity | track_cnt
    int64_t row_bytes;
    int32_t rows_cap;                   // rows of an item's result arrays
    int32_t count, publish, border;
    int32_t reject, flow_back;          // 0: a published read runs no rejectWithF; 1: the tracker ran the forward-backward check
#ifdef FRONT_CAMERAS
    const uint8_t *lflags;              // k_reject_lift's flag byte per point: CAM_FLAG_BAD | CAM_FLAG_CLAMPED
#endif
};

// the exclusive prefix of `keep` over the workgroup's rows, and their total; every thread of the workgroup calls it
__device__ __forceinline__ int front_scan(bool keep, int32_t *s_w, int &total) {
    const int lane = threadIdx.x & (FRONT_WAVE - 1), wv = threadIdx.x / FRONT_WAVE;
    const uint64_t b = __ballot(keep);
    __syncthreads();                                        // (the scan before has been read)
    if (lane == 0) s_w[wv] = front_wave_count(b);
    __syncthreads();
    total = front_wave_base(s_w, FRONT_WAVES);
    return front_wave_base(s_w, wv) + front_lane_rank(b, lane);
}

__global__ __launch_bounds__(FNT) void k_front_begin(FrontArgs a) {
    const FrontItem &I = a.items[blockIdx.x];
    const int t = threadIdx.x;
    if (t >= front_clamp(I.n, 0, FRONT_CAP)) return;
    kf::FlowPt p;
    p.item = (int32_t)blockIdx.x; p.has_guess = 0;
    p.px = I.cur_pts[2 * t]; p.py = I.cur_pts[2 * t + 1];
    p.gx = 0.f; p.gy = 0.f;
    a.fpts[I.flow_off + t] = p;
}

__global__ __launch_bounds__(FNT) void k_front_filter(FrontArgs a) {
    __shared__ int32_t s_w[FRONT_WAVES];
    const int item = blockIdx.x, t = threadIdx.x;
    const FrontItem &I = a.items[item];
    const int n = front_clamp(I.n, 0, FRONT_CAP);
    float fx = 0.f, fy = 0.f;
    bool keep = false;
    int st = -1;
    if (t < n) {
        const kf::FlowOut o = a.fout[I.flow_off + t];
        fx = o.x; fy = o.y; st = o.status;
        keep = o.status == 0 && front_in_border(fx, fy, I.w, I.h, a.border);
    }
    int n_ok = 0, n_lost = 0, n_far = 0;
    if (a.flow_back) {                                      // (uniform: every thread of the workgroup takes the barriers)
        (void)front_scan(st == 0, s_w, n_ok);
        (void)front_scan(st == VIO_FLOW_FAIL_BACK_LOST, s_w, n_lost);
        (void)front_scan(st == VIO_FLOW_FAIL_BACK_FAR, s_w, n_far);
    }
    int nk;
    const int dst = front_scan(keep, s_w, nk);
    FRONT_REJ::RejPair &P = a.pairs[item];
    const int64_t row = (int64_t)item * FRONT_CAP + dst;
    if (keep) {
        float *cur = a.rstage + P.o_pts, *forw = cur + 2 * (int64_t)nk;
        cur[2 * dst] = I.cur_pts[2 * t]; cur[2 * dst + 1] = I.cur_pts[2 * t + 1];
        forw[2 * dst] = fx; forw[2 * dst + 1] = fy;
        a.fa[2 * row] = fx; a.fa[2 * row + 1] = fy;
        a.ida[row] = I.ids[t];
        a.cnta[row] = I.cnt[t] + 1;
    }
    if (t == 0) {
        P.n = nk; P.finite = 1;
        P.active = a.publish && a.reject && nk >= VIO_REJECT_MIN_POINTS;
        FrontRes &R = a.res[item];
        R.n_checked = n_ok + n_lost + n_far; R.n_back_lost = n_lost; R.n_back_far = n_far; R.pad_back = 0;
        R.n = nk; R.n_new = 0; R.n_tracked_in = n; R.n_after_track = nk; R.n_after_reject = nk;
        R.reject_status = VIO_OK; R.reject_hyp = -1; R.n_candidates = 0; R.next_id = 0;
    }
}

__global__ __launch_bounds__(FNT) void k_front_after_reject(FrontArgs a) {
    __shared__ int32_t s_w[FRONT_WAVES];
    const int item = blockIdx.x, t = threadIdx.x;
    const FRONT_REJ::RejPair &P = a.pairs[item];
    const int nk = front_clamp(P.n, 0, FRONT_CAP);
    const bool keep = t < nk && (!P.active || a.rmask[P.o_pt + t] != 0);
    int n2;
    const int dst = front_scan(keep, s_w, n2);
    kd::DetItemD &D = a.ditems[item];
    if (keep) {
        const int64_t src = (int64_t)item * FRONT_CAP + t, row = (int64_t)item * FRONT_CAP + dst;
        const float x = a.fa[2 * src], y = a.fa[2 * src + 1];
        const int32_t c = a.cnta[src];
        a.fb[2 * row] = x; a.fb[2 * row + 1] = y;
        a.idb[row] = a.ida[src];
        a.cntb[row] = c;
        kd::DetTrk k;
        k.cx = front_pixel(x); k.cy = front_pixel(y); k.cnt = c; k.pad = 0;         // (inside the border: inside the image)
        a.dtrk[D.trk + dst] = k;
    }
    if (t == 0) {
        D.n_tracked = n2;
        FrontRes &R = a.res[item];
        R.n_after_reject = n2;
        if (P.active) { R.reject_status = a.rres[item].status; R.reject_hyp = a.rres[item].hyp; }
    }
}

__global__ __launch_bounds__(FNT) void k_front_merge(FrontArgs a) {
    const int item = blockIdx.x, t = threadIdx.x;
    const FrontItem &I = a.items[item];
    FRONT_REJ::LiftItem &L = a.litems[item];
    const float *sf = a.publish ? a.fb : a.fa;
    const long long *si = a.publish ? a.idb : a.ida;
    const int32_t *sc = a.publish ? a.cntb : a.cnta;
    int n_kept, n_new = 0, n_cand = 0, nt;
    if (a.publish) {
        const kd::DetItemD &D = a.ditems[item];
        nt = front_clamp(D.n_tracked, 0, FRONT_CAP);
        n_kept = front_clamp(a.dres[item].n_kept, 0, nt);
        n_new = front_clamp(a.dres[item].n_new, 0, front_clamp(D.max_total, 0, FRONT_CAP));
        n_new = front_clamp(n_new, 0, FRONT_CAP - n_kept);
        n_cand = a.dres[item].n_cand;
    } else {
        nt = front_clamp(a.pairs[item].n, 0, FRONT_CAP);
        n_kept = nt;
    }
    const int n = n_kept + n_new, m = front_clamp(I.m, 0, FRONT_CAP);
    float *pts = a.lstage + L.o_pts, *prev = a.lstage + L.o_prev;
    long long *ids = a.lids + L.o_ids;
    if (t < n) {
        float x, y;
        long long id = -1ll;
        int32_t c = 1;
        if (t < n_kept) {
            const int k = a.publish ? front_clamp(a.keep_order[a.ditems[item].trk + t], 0, nt - 1) : t;
            const int64_t src = (int64_t)item * FRONT_CAP + k;
            x = sf[2 * src]; y = sf[2 * src + 1]; id = si[src]; c = sc[src];
        } else {
            const float *q = a.new_pts + 2 * ((int64_t)a.ditems[item].newp + (t - n_kept));
            x = q[0]; y = q[1];
        }
        pts[2 * t] = x; pts[2 * t + 1] = y;
        ids[t] = id;
        a.cntm[(int64_t)item * FRONT_CAP + t] = c;
    }
    if (t < m) {
        ids[n + t] = I.prev_un_ids[t];
        prev[2 * t] = I.prev_un_pts[2 * t]; prev[2 * t + 1] = I.prev_un_pts[2 * t + 1];
    }
    if (t == 0) {
        L.n = n; L.m = m;
        FrontRes &R = a.res[item];
        R.n = n; R.n_new = n_new; R.n_candidates = n_cand;
    }
}

__global__ __launch_bounds__(FNT) void k_front_finish(FrontArgs a) {
    __shared__ int32_t s_w[FRONT_WAVES];
    const int item = blockIdx.x, t = threadIdx.x;
    const FrontItem &I = a.items[item];
    const FRONT_REJ::LiftItem &L = a.litems[item];
    const int n = front_clamp(L.n, 0, FRONT_CAP);
    const long long next = *I.next_id;
    long long id = 0;
    float x = 0.f, y = 0.f, ux = 0.f, uy = 0.f, vx = 0.f, vy = 0.f;
    if (t < n) {
        id = a.lids[L.o_ids + t];
        x = a.lstage[L.o_pts + 2 * t]; y = a.lstage[L.o_pts + 2 * t + 1];
        ux = a.un[2 * (L.o_out + t)]; uy = a.un[2 * (L.o_out + t) + 1];
        vx = a.vel[2 * (L.o_out + t)]; vy = a.vel[2 * (L.o_out + t) + 1];
    }
#ifdef FRONT_CAMERAS
    const int lf = t < n ? (int)a.lflags[L.o_out + t] : 0;
    int n_bad, n_clamped;
    (void)front_scan((lf & FRONT_REJ::CAM_FLAG_BAD) != 0, s_w, n_bad);      // (ballots and sixteen integer counts: the order is fixed)
    (void)front_scan((lf & FRONT_REJ::CAM_FLAG_CLAMPED) != 0, s_w, n_clamped);
    if (n_bad > 0) { ux = NAN; uy = NAN; vx = NAN; vy = NAN; }
#endif
    int n_fresh;
    const int rank = front_scan(t < n && id == -1ll, s_w, n_fresh);             // (every thread has read the counter behind its barriers)
    if (t < n) {
        I.prev_un_ids[t] = id;                                                  // as it is now, before updateID: the kept quirk
        I.prev_un_pts[2 * t] = ux; I.prev_un_pts[2 * t + 1] = uy;
        const long long nid = front_new_id(id, next, rank);
        const int32_t c = a.cntm[(int64_t)item * FRONT_CAP + t];
        I.cur_pts[2 * t] = x; I.cur_pts[2 * t + 1] = y;
        I.ids[t] = nid;
        I.cnt[t] = c;
        if (t < a.rows_cap) {
            const int64_t R = a.rows_cap;
            char *base = a.rows + (int64_t)item * a.row_bytes;
            long long *o_id = (long long *)base;
            float *o_pts = (float *)(base + 8 * R), *o_un = o_pts + 2 * R, *o_vel = o_un + 2 * R;
            int32_t *o_cnt = (int32_t *)(o_vel + 2 * R);
            o_id[t] = nid;
            o_pts[2 * t] = x; o_pts[2 * t + 1] = y;
            o_un[2 * t] = ux; o_un[2 * t + 1] = uy;
            o_vel[2 * t] = vx; o_vel[2 * t + 1] = vy;
            o_cnt[t] = c;
        }
    }
    if (t == 0) {
        *I.next_id = next + n_fresh;
        a.res[item].next_id = next + n_fresh;
#ifdef FRONT_CAMERAS
        a.res[item].n_clamped = n_bad > 0 ? 0 : n_clamped;
        a.res[item].n_bad = n_bad;
#endif
    }
}
