// vio_est_init_body.inc — visualInitialAlign's hand-over into a slot and the bias re-linearisation (include/vio_est_init.h; DESIGN.md
// section 33).  Included at the end of csrc/vio_est.hip: the handle, the tables and the host helpers are that file's.
//   k_est_init_apply    one wavefront per item: every lane reads the device rule (full window, intervals 0 .. 10 exist), lane i < 11
//                       writes frame i and interval i's linearisation biases, lane 11 the gravity; with commit_last lane 10 also
//                       writes last_R / last_P and lane 0 last_R0 / last_P0, as k_est_update does
//   k_est_relinearize   one wavefront per item: lane j in 1 .. 10 tests interval j against frame j - 1's biases and rewrites its
//                       linearisation biases; the mask is the wavefront's ballot
// A lane writes only what no other lane reads (lane i: row i of Ps / Rs / Vs / Bas / Bgs / lin_bias and the last_* arrays, none of
// which the rule reads; lane j: lin_bias[j]), so there is no barrier, no LDS and no atomic.
#include "../../include/vio_est_init.h"
#include "vio_est_init_math.h"

static_assert(sizeof(vio_est_init_item) == 8 + 188 * 8 && sizeof(vio_est_relin_item) == 24 && sizeof(vio_est_relin_result) == 16,
              "the layouts the binding mirrors");

struct EstInitArgs {
    EstTables t;
    const vio_est_init_item *items;     // [count]
    vio_est_result *res;                // [count]
};

__global__ __launch_bounds__(EST_WAVE) void k_est_init_apply(EstInitArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const vio_est_init_item *it = a.items + i;
    vio_est_state *S = a.t.state + it->slot;
    const int fc = S->frame_count;
    bool ready = fc == EST_WINDOW;
    for (int j = 0; j < EST_FRAMES; ++j) ready = ready && S->exists[j] != 0;
    if (lane == 0) {
        vio_est_result *r = a.res + i;
        est_result_clear(r);
        r->status = ready ? VIO_EST_STATUS_OK : VIO_EST_STATUS_NOT_READY;
        r->frame_count = fc;
    }
    if (!ready) return;
    if (lane < EST_FRAMES) {                        // :397-404, :419-425, :433, :450-455 as vio_init_align_batch left the rows
        double R[9], P[3], V[3], Ba[3], Bg[3], L[6];
        est_init_frame(it->poses[lane], it->speed_bias[lane], R, P, V, Ba, Bg, L);
        for (int c = 0; c < 9; ++c) S->Rs[lane][c] = R[c];
        for (int c = 0; c < 3; ++c) { S->Ps[lane][c] = P[c]; S->Vs[lane][c] = V[c]; S->Bas[lane][c] = Ba[c]; S->Bgs[lane][c] = Bg[c]; }
        for (int c = 0; c < 6; ++c) S->lin_bias[lane][c] = L[c];
        if (it->commit_last != 0 && lane == EST_WINDOW)
            for (int c = 0; c < 9; ++c) { S->last_R[c] = R[c]; if (c < 3) S->last_P[c] = P[c]; }
        if (it->commit_last != 0 && lane == 0)
            for (int c = 0; c < 9; ++c) { S->last_R0[c] = R[c]; if (c < 3) S->last_P0[c] = P[c]; }
    } else if (lane == EST_FRAMES) {                // :448
        double g[3];
        est_init_gravity(it->rot, it->g, g);
        for (int c = 0; c < 3; ++c) S->g[c] = g[c];
    }
}

struct EstRelinArgs {
    EstTables t;
    const vio_est_relin_item *items;    // [count]
    vio_est_relin_result *res;          // [count]
};

__global__ __launch_bounds__(EST_WAVE) void k_est_relinearize(EstRelinArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const vio_est_relin_item *it = a.items + i;
    vio_est_state *S = a.t.state + it->slot;
    bool moved = false;
    if (lane >= 1 && lane < EST_FRAMES && S->exists[lane] != 0) {      // interval `lane` starts at frame lane - 1
        double Ba[3], Bg[3], L[6];
        for (int c = 0; c < 3; ++c) { Ba[c] = S->Bas[lane - 1][c]; Bg[c] = S->Bgs[lane - 1][c]; }
        for (int c = 0; c < 6; ++c) L[c] = S->lin_bias[lane][c];
        moved = est_relin_moved(Ba, Bg, L, it->ba_thresh, it->bg_thresh);
        if (moved)
            for (int c = 0; c < 3; ++c) { S->lin_bias[lane][c] = Ba[c]; S->lin_bias[lane][3 + c] = Bg[c]; }
    }
    const unsigned long long m = __ballot(moved);
    if (lane == 0) {
        vio_est_relin_result *r = a.res + i;
        r->status = VIO_EST_STATUS_OK;
        r->frame_count = S->frame_count;
        r->n_relinearized = __popcll(m);
        r->mask = (int32_t)m;
    }
}

extern "C" {

vio_status vio_est_init_apply_batch(vio_est *h, int32_t count, const vio_est_init_item *items, vio_est_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "init_apply_batch")) != VIO_OK || (st = check_distinct(h, count, items, "init_apply_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    for (int32_t i = 0; i < count; ++i)
        if (!all_finite(&items[i].poses[0][0], 188))
            return fail(h->err, VIO_ERR_BAD_ARG, "init_apply_batch: item %d: a non-finite pose, speed-bias, g or rot", i);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t nin = align256(sizeof(vio_est_init_item) * (size_t)count), nout = sizeof(vio_est_result) * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    std::memcpy(h->in.h, items, sizeof(vio_est_init_item) * (size_t)count);
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    EstInitArgs a;
    a.t = h->t;
    a.items = (const vio_est_init_item *)h->in.d;
    a.res = (vio_est_result *)h->out.d;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_est_init_apply, dim3(count), dim3(EST_WAVE), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_est_init_apply launch");
    return finish(h, clk, t_host, count, nout, results, "k_est_init_apply");
}

vio_status vio_est_relinearize_batch(vio_est *h, int32_t count, const vio_est_relin_item *items, vio_est_relin_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "relinearize_batch")) != VIO_OK || (st = check_distinct(h, count, items, "relinearize_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    for (int32_t i = 0; i < count; ++i) {
        const double ta = items[i].ba_thresh, tg = items[i].bg_thresh;
        if (!std::isfinite(ta) || !std::isfinite(tg) || ta < 0.0 || tg < 0.0)
            return fail(h->err, VIO_ERR_BAD_ARG, "relinearize_batch: item %d: a threshold that is not finite or negative", i);
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t nin = align256(sizeof(vio_est_relin_item) * (size_t)count), nout = sizeof(vio_est_relin_result) * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    std::memcpy(h->in.h, items, sizeof(vio_est_relin_item) * (size_t)count);
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    EstRelinArgs a;
    a.t = h->t;
    a.items = (const vio_est_relin_item *)h->in.d;
    a.res = (vio_est_relin_result *)h->out.d;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_est_relinearize, dim3(count), dim3(EST_WAVE), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_est_relinearize launch");
    return finish(h, clk, t_host, count, nout, results, "k_est_relinearize", sizeof(vio_est_relin_result));
}

}   // extern "C"
