// vio_aif.hip — all_image_frame and tmp_pre_integration of many streams (include/vio_aif.h).
//
// A handle keeps, for VIO_AIF_MAX_SLOTS slots: one vio_aif_slot each (d_slot; its samp_off and first are filled on download only),
// VIO_AIF_OFFS absolute sample offsets each (d_off), the constructor samples of every interval (d_first, VIO_AIF_OFFS rows of 6 per
// slot, row 33 unused), one region of VIO_AIF_MAX_SAMPLES samples each in d_dt / d_acc / d_gyr and one region of VIO_AIF_MAX_POINTS
// points each in d_ids / d_pts.  Interval (slot, j) is thereby CSR interval VIO_AIF_OFFS slot + j of csrc/vio_imu_body.inc's
// ImuArgs, and vio_aif_propagate_batch launches k_imu_propagate, the kernel of libvio_imu_hip, straight over the resident tables.
// Offsets behind the open interval repeat the end, so an append moves them all.
//   k_aif_imu      one wavefront per item: the lanes stride over the copy of the run into the slot's region, lane 0 keeps the books
//   k_aif_image    one workgroup of AIF_NT threads per item: the ids go to LDS, every thread ranks its ids against all of them
//                  (csrc/vio_aif_math.h's aif_rank) and stores its points at their ranks; thread 0 keeps the books
//   k_aif_slide    one workgroup of AIF_NT threads per item: samples and points move down in chunks, read, barrier, write, barrier;
//                  thread j moves row j of the tables, read, barrier, write
//   k_aif_info     one thread per item: the result rows of vio_aif_propagate_batch
// Every kernel decides first, from what it read before any write, whether the item is refused, in all its threads alike.  No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vio_aif.h"
#include "vio_companion.h"
#include "vio_aif_math.h"
#include "vio_imu_body.inc"

#pragma clang fp contract(off)

#include "vio_sfm_math.h"
#include "vio_pnp_body.inc"

#define AIF_WAVE 64
#define AIF_NT 256                          // threads of k_aif_image's and k_aif_slide's workgroup: one chunk

static_assert(VIO_AIF_MAX_SLOTS == AIF_MAX_SLOTS && VIO_AIF_MAX_FRAMES == AIF_MAX_FRAMES && VIO_AIF_MAX_FRAME_POINTS == AIF_MAX_FRAME_POINTS &&
              VIO_AIF_MAX_POINTS == AIF_MAX_POINTS && VIO_AIF_MAX_SAMPLES == AIF_MAX_SAMPLES && VIO_AIF_OFFS == AIF_OFFS,
              "vio_aif.h and vio_aif_math.h agree");
static_assert(VIO_AIF_STATUS_POOL_FULL == AIF_STATUS_POOL_FULL && VIO_AIF_STATUS_FRAMES_FULL == AIF_STATUS_FRAMES_FULL &&
              VIO_AIF_STATUS_NO_FRAME == AIF_STATUS_NO_FRAME, "the statuses' numbers");
static_assert(VIO_AIF_STATUS_WALK == AIF_STATUS_WALK && VIO_AIF_MAX_KEY == AIF_MAX_KEY && VIO_AIF_MAX_TRACKS == AIF_MAX_TRACKS &&
              VIO_AIF_MAX_FRAMES == VIO_PNP_MAX_FRAMES && VIO_AIF_MAX_POINTS <= 2 * VIO_PNP_MAX_POINTS && VIO_AIF_MAX_FRAME_POINTS <= VIO_PNP_MAX_POINTS &&
              VIO_AIF_MAX_FRAMES <= WAVE, "the structure call's limits");
static_assert(sizeof(vio_aif_structure_item) == 176 && sizeof(vio_aif_structure_result) == 32 && sizeof(vio_pnp_frame_info) == 24, "... and its layouts");
static_assert(VIO_AIF_OFFS == VIO_AIF_MAX_FRAMES + 2 && VIO_AIF_OFFS <= AIF_NT, "one thread per table row");
static_assert(sizeof(vio_aif_slot) == 416 + 272 + 830 * 8 && sizeof(vio_aif_result) == 32 && sizeof(vio_aif_image_item) == 80 &&
              sizeof(vio_aif_propagate_item) == 64, "the layouts the binding mirrors");

struct AifTables {
    vio_aif_slot *slot;         // [VIO_AIF_MAX_SLOTS]
    int64_t *off;               // [VIO_AIF_MAX_SLOTS][VIO_AIF_OFFS], absolute
    double *first;              // [VIO_AIF_MAX_SLOTS][VIO_AIF_OFFS][6]
    double *dt, *acc, *gyr;     // [VIO_AIF_MAX_SLOTS * VIO_AIF_MAX_SAMPLES] (x 3)
    int64_t *ids;               // [VIO_AIF_MAX_SLOTS * VIO_AIF_MAX_POINTS]
    double *pts;                // [VIO_AIF_MAX_SLOTS * VIO_AIF_MAX_POINTS][2]
};

__device__ __forceinline__ void aif_result(vio_aif_result *r, int status, int n_frames, int n_points, int n_samples) {
    r->status = status; r->n_frames = n_frames; r->n_points = n_points; r->n_samples = n_samples;
    r->erased_frames = 0; r->erased_samples = 0; r->records = 0; r->reserved = 0;
}

struct AifImuArgs {
    AifTables t;
    const int32_t *slot;        // [count]
    const int64_t *in_off;      // [count + 1] into in_dt / in_acc / in_gyr
    const double *in_dt, *in_acc, *in_gyr;
    vio_aif_result *res;        // [count]
};

__global__ __launch_bounds__(AIF_WAVE) void k_aif_imu(AifImuArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const int slot = a.slot[i];
    vio_aif_slot *S = a.t.slot + slot;
    int64_t *o = a.t.off + (int64_t)AIF_OFFS * slot;
    const int64_t b = a.in_off[i];
    const int n = (int)(a.in_off[i + 1] - b);
    const int F = S->n_frames;
    const int open = S->exists[F];                  // the reference's frame_count != 0
    const int64_t end = o[AIF_OFFS - 1];
    const int held = (int)(end - o[0]);
    const int st = aif_imu_status(open, held, n);
    if (st == AIF_STATUS_OK && open)                // tmp_pre_integration->push_back (:122): the open interval is the last with samples
        for (int s = lane; s < n; s += AIF_WAVE) {
            a.t.dt[end + s] = a.in_dt[b + s];
            for (int c = 0; c < 3; ++c) {
                a.t.acc[3 * (end + s) + c] = a.in_acc[3 * (b + s) + c];
                a.t.gyr[3 * (end + s) + c] = a.in_gyr[3 * (b + s) + c];
            }
        }
    __syncthreads();
    if (lane != 0) return;
    vio_aif_result *r = a.res + i;
    aif_result(r, st, F, S->n_points, held);
    if (st != AIF_STATUS_OK || n == 0) return;
    S->first_imu = 1;                               // :107-112 (acc_0 / gyr_0 end as the last sample either way)
    if (open) {
        for (int j = F + 1; j < AIF_OFFS; ++j) o[j] += n;
        r->n_samples = held + n;
    }
    for (int c = 0; c < 3; ++c) {                   // :137-138
        S->acc_0[c] = a.in_acc[3 * (b + n - 1) + c];
        S->gyr_0[c] = a.in_gyr[3 * (b + n - 1) + c];
    }
}

struct AifImageArgs {
    AifTables t;
    const int32_t *slot;        // [count]
    const int64_t *in_off;      // [count + 1] into in_ids / in_pts
    const int64_t *in_ids;
    const double *in_pts;       // [.][2]
    const double *header;       // [count]
    const double *bias;         // [count][6] ba | bg
    vio_aif_result *res;
};

__global__ __launch_bounds__(AIF_NT) void k_aif_image(AifImageArgs a) {
    __shared__ int64_t sid[AIF_MAX_FRAME_POINTS];
    const int t = threadIdx.x, i = blockIdx.x;
    const int slot = a.slot[i];
    vio_aif_slot *S = a.t.slot + slot;
    const int64_t b = a.in_off[i];
    const int n = (int)(a.in_off[i + 1] - b);
    const int F = S->n_frames, held = S->n_points;
    const int64_t *o = a.t.off + (int64_t)AIF_OFFS * slot;
    const int samples = (int)(o[AIF_OFFS - 1] - o[0]);
    const int st = aif_image_status(F, held, n);
    if (st != AIF_STATUS_OK) {
        if (t == 0) aif_result(a.res + i, st, F, held, samples);
        return;
    }
    for (int e = t; e < n; e += AIF_NT) sid[e] = a.in_ids[b + e];
    __syncthreads();                                // (every thread has read the slot's books by now; thread 0 writes them below)
    const int64_t base = (int64_t)AIF_MAX_POINTS * slot + held;
    for (int e = t; e < n; e += AIF_NT) {
        const int r = aif_rank(sid, n, e);
        a.t.ids[base + r] = sid[e];
        a.t.pts[2 * (base + r)] = a.in_pts[2 * (b + e)];
        a.t.pts[2 * (base + r) + 1] = a.in_pts[2 * (b + e) + 1];
    }
    if (t != 0) return;
    S->t[F] = a.header[i];                          // ImageFrame(image, header): is_key_frame false, R and T unset (0 here)
    for (int c = 0; c < 9; ++c) S->R[F][c] = 0.0;
    for (int c = 0; c < 3; ++c) S->T[F][c] = 0.0;
    S->is_key[F] = 0;
    S->pt_off[F + 1] = held + n;
    S->n_points = held + n;
    S->n_frames = F + 1;                            // the frame keeps interval F as it stands (:157); interval F + 1 opens (:159)
    S->exists[F + 1] = 1;
    double *f = a.t.first + 6 * ((int64_t)AIF_OFFS * slot + F + 1);
    for (int c = 0; c < 3; ++c) { f[c] = S->acc_0[c]; f[3 + c] = S->gyr_0[c]; }
    for (int c = 0; c < 6; ++c) S->bias[F + 1][c] = a.bias[6 * i + c];
    aif_result(a.res + i, st, F + 1, held + n, samples);
}

struct AifSlideArgs {
    AifTables t;
    const int32_t *slot;
    const double *t_0;
    vio_aif_result *res;
};

__global__ __launch_bounds__(AIF_NT) void k_aif_slide(AifSlideArgs a) {
    const int t = threadIdx.x, i = blockIdx.x;
    const int slot = a.slot[i];
    vio_aif_slot *S = a.t.slot + slot;
    int64_t *o = a.t.off + (int64_t)AIF_OFFS * slot;
    double *first = a.t.first + 6 * (int64_t)AIF_OFFS * slot;
    const int F = S->n_frames, held = S->n_points;
    const int k = aif_find(S->t, F, a.t_0[i]);
    const int64_t o0 = o[0], oend = o[AIF_OFFS - 1];
    if (k < 0) {
        if (t == 0) aif_result(a.res + i, AIF_STATUS_NO_FRAME, F, held, (int)(oend - o0));
        return;
    }
    const int d = k + 1;                            // frames and intervals 0 .. k leave
    const int64_t oc = o[d];
    const int pc = S->pt_off[d];
    // the samples of intervals d .. open move down over the erased ones: a chunk is read, then written, so a chunk never reads what
    // an earlier one wrote (the destination lies below the source)
    const int64_t stail = oend - oc;
    if (oc != o0)
        for (int64_t base = 0; base < stail; base += AIF_NT) {
            const int64_t s = base + t;
            const bool on = s < stail;
            double v[7] = {0, 0, 0, 0, 0, 0, 0};
            if (on) {
                v[0] = a.t.dt[oc + s];
                for (int c = 0; c < 3; ++c) { v[1 + c] = a.t.acc[3 * (oc + s) + c]; v[4 + c] = a.t.gyr[3 * (oc + s) + c]; }
            }
            __syncthreads();
            if (on) {
                a.t.dt[o0 + s] = v[0];
                for (int c = 0; c < 3; ++c) { a.t.acc[3 * (o0 + s) + c] = v[1 + c]; a.t.gyr[3 * (o0 + s) + c] = v[4 + c]; }
            }
            __syncthreads();
        }
    const int64_t pbase = (int64_t)AIF_MAX_POINTS * slot;
    const int ptail = held - pc;
    if (pc != 0)
        for (int base = 0; base < ptail; base += AIF_NT) {
            const int s = base + t;
            const bool on = s < ptail;
            int64_t id = 0;
            double x = 0, y = 0;
            if (on) { id = a.t.ids[pbase + pc + s]; x = a.t.pts[2 * (pbase + pc + s)]; y = a.t.pts[2 * (pbase + pc + s) + 1]; }
            __syncthreads();
            if (on) { a.t.ids[pbase + s] = id; a.t.pts[2 * (pbase + s)] = x; a.t.pts[2 * (pbase + s) + 1] = y; }
            __syncthreads();
        }
    // row t of the tables takes row t + d: interval rows up to the open one (index F), frame rows below F.  Read, barrier, write.
    const int sj = t + d;
    const bool row = t < AIF_OFFS, ival = row && sj <= F, frame = row && sj < F;
    int64_t no = 0;
    int np = 0, ex = 0, key = 0;
    double H = 0, R[9], T[3], Fi[6], B[6];
    if (row) {
        no = aif_slid_off(o, AIF_OFFS - 1, k, t);
        np = S->pt_off[sj < F ? sj : F] - pc;
    }
    if (ival) {
        ex = S->exists[sj];
        for (int c = 0; c < 6; ++c) { Fi[c] = first[6 * sj + c]; B[c] = S->bias[sj][c]; }
    }
    if (frame) {
        H = S->t[sj];
        key = S->is_key[sj];
        for (int c = 0; c < 9; ++c) R[c] = S->R[sj][c];
        for (int c = 0; c < 3; ++c) T[c] = S->T[sj][c];
    }
    __syncthreads();
    if (row) {
        o[t] = no;
        S->pt_off[t] = np;
        S->exists[t] = ex;
    }
    if (ival)
        for (int c = 0; c < 6; ++c) { first[6 * t + c] = Fi[c]; S->bias[t][c] = B[c]; }
    if (frame) {
        S->t[t] = H;
        S->is_key[t] = key;
        for (int c = 0; c < 9; ++c) S->R[t][c] = R[c];
        for (int c = 0; c < 3; ++c) S->T[t][c] = T[c];
    }
    if (t == 0) {
        S->n_frames = F - d;
        S->n_points = ptail;
        vio_aif_result *r = a.res + i;
        aif_result(r, AIF_STATUS_OK, F - d, ptail, (int)stail);
        r->erased_frames = d;
        r->erased_samples = (int)(oc - o0);
    }
}

struct AifInfoArgs {
    AifTables t;
    const int32_t *slot;
    vio_aif_result *res;
    int count;
};

__global__ __launch_bounds__(AIF_WAVE) void k_aif_info(AifInfoArgs a) {
    const int i = blockIdx.x * AIF_WAVE + threadIdx.x;
    if (i >= a.count) return;
    const int slot = a.slot[i];
    const vio_aif_slot *S = a.t.slot + slot;
    const int64_t *o = a.t.off + (int64_t)AIF_OFFS * slot;
    vio_aif_result *r = a.res + i;
    aif_result(r, AIF_STATUS_OK, S->n_frames, S->n_points, (int)(o[AIF_OFFS - 1] - o[0]));
    r->records = S->n_frames > 1 ? S->n_frames - 1 : 0;
}

// ---- vio_aif_structure_batch ----
// Per item the staged tables have fixed strides: STR_OBS observations (a slot's point pool) and the SfM's tracks with one extra,
// invalid row behind them.  PnP row 32 i + j is frame j of item i; a keyframe, a frame that does not exist and every frame of an item
// whose walk failed is an empty row (nobs = 0), which k_pnp_frames ends at once.
struct AifStructArgs {
    AifTables t;
    const int32_t *slot, *n_key, *n_tracks;     // [count]
    const int64_t *tr_off;                      // [count + 1]: item i's tracks are rows tr_off[i] .. of the track arrays, n_tracks + 1 of them
    const int64_t *rec_off;                     // [count + 1]: item i's records
    const double *headers;                      // [count][AIF_MAX_KEY]
    const double *ric;                          // [count][9]
    const int64_t *track_ids;                   // [tr_off[count]]
    int64_t *sorted_id;                         // [tr_off[count]]
    int32_t *sorted_tr;                         // [tr_off[count]]
    const PnpWin *wins;                         // [count] (host-made)
    PnpFrame *frames;                           // [count][32]
    int32_t *ints;                              // PnpArgs::ints
    double *dd;                                 // PnpArgs::dd
    int64_t o_op, o_obs;                        // where item 0's obs_point / obs_pts start in ints / dd; item i's lie i * AIF_MAX_POINTS (x 2) on
    const double *rec;                          // [rec_off[count]][IMU_REC]
    const double *pnp_out;                      // [count][32][FO]
    int32_t *walk;                              // [count][2 + 64]: status, n_key found | is_key [32] | guess [32]
    vio_aif_structure_result *res;              // [count]
    double *R_out, *T_out;                      // [count][32][9], [count][32][3]
    int32_t *key_out;                           // [count][32]
    vio_pnp_frame_info *info;                   // [count][32]
};

__global__ __launch_bounds__(AIF_WAVE) void k_aif_bias(AifTables t, const int *which, double *bias, int nrec) {
    const int k = blockIdx.x * AIF_WAVE + threadIdx.x;
    if (k >= nrec) return;
    const int iv = which[k], slot = iv / AIF_OFFS, j = iv % AIF_OFFS;
    for (int c = 0; c < 6; ++c) bias[6 * k + c] = t.slot[slot].bias[j][c];
}

__global__ __launch_bounds__(AIF_NT) void k_aif_join(AifStructArgs a) {
    __shared__ int64_t sid[AIF_MAX_TRACKS];
    __shared__ int32_t s_key[AIF_MAX_FRAMES], s_guess[AIF_MAX_FRAMES], s_st[2];
    const int t = threadIdx.x, i = blockIdx.x;
    const int slot = a.slot[i], nk = a.n_key[i], ntr = a.n_tracks[i];
    vio_aif_slot *S = a.t.slot + slot;
    const int F = S->n_frames;
    const double *hd = a.headers + (int64_t)AIF_MAX_KEY * i, *ric = a.ric + 9 * i;
    const PnpWin W = a.wins[i];
    const int64_t tro = a.tr_off[i];
    if (t < AIF_MAX_FRAMES) { s_key[t] = 0; s_guess[t] = 0; }
    for (int e = t; e < ntr; e += AIF_NT) sid[e] = a.track_ids[tro + e];
    __syncthreads();
    if (t == 0) {                                   // the excitation check and the key walk: F <= 32, one thread
        const double var = aif_excitation(a.rec + (int64_t)IMU_REC * a.rec_off[i], IMU_REC, F > 0 ? F - 1 : 0);
        const int st = aif_walk(S->t, F, hd, nk, s_key, s_guess);       // (into LDS: a private array indexed by the walk would be scratch)
        int found = 0;
        for (int j = 0; j < AIF_MAX_FRAMES; ++j) {
            if (st != AIF_STATUS_OK || j >= F) { s_key[j] = 0; s_guess[j] = 0; }
            found += s_key[j];
        }
        s_st[0] = st; s_st[1] = found;
        vio_aif_structure_result *r = a.res + i;
        r->status = st; r->pnp_status = VIO_OK; r->fail_frame = -1; r->n_frames = F; r->n_key = found;
        r->low_excitation = var < 0.25 ? 1 : 0;
        r->var = var;
    }
    for (int e = t; e < ntr; e += AIF_NT) {         // the item's tracks sorted by id
        const int r = aif_rank(sid, ntr, e);
        a.sorted_id[tro + r] = sid[e];
        a.sorted_tr[tro + r] = e;
    }
    __syncthreads();
    const int st = s_st[0];
    int32_t *wk = a.walk + 66 * i;
    if (t < 2) wk[t] = s_st[t];
    if (t < AIF_MAX_FRAMES) {
        wk[2 + t] = s_key[t]; wk[34 + t] = s_guess[t];
        const bool solve = st == AIF_STATUS_OK && t < F && !s_key[t];
        const int p0 = t < F ? S->pt_off[t] : 0, p1 = t < F ? S->pt_off[t + 1] : 0;
        PnpFrame fr;
        fr.win = i; fr.guess = s_guess[t];
        fr.nobs = solve ? p1 - p0 : 0; fr.pad = 0;
        fr.o_op = a.o_op + (int64_t)AIF_MAX_POINTS * i + p0;
        fr.o_obs = a.o_obs + 2 * ((int64_t)AIF_MAX_POINTS * i + p0);
        fr.o_scr = PD * ((int64_t)AIF_MAX_POINTS * i + p0);
        a.frames[AIF_MAX_FRAMES * i + t] = fr;
        if (st == AIF_STATUS_OK && t < F && s_key[t]) {     // :316-320
            double Rq[9], R[9];
            aif_quat_to_rot(a.dd + W.o_key + 4 * s_guess[t], Rq);
            aif_mul_rict(Rq, ric, R);
            for (int c = 0; c < 9; ++c) { S->R[t][c] = R[c]; a.R_out[9 * (AIF_MAX_FRAMES * i + t) + c] = R[c]; }
            for (int c = 0; c < 3; ++c) {
                const double v = a.dd[W.o_keyT + 3 * s_guess[t] + c];
                S->T[t][c] = v; a.T_out[3 * (AIF_MAX_FRAMES * i + t) + c] = v;
            }
            S->is_key[t] = 1;
        }
    }
    if (st != AIF_STATUS_OK) return;
    // every observation of a non-keyframe: its id's track by bisection; a missing id or a track with state 0 is the extra row
    const int64_t pbase = (int64_t)AIF_MAX_POINTS * slot, obase = (int64_t)AIF_MAX_POINTS * i;
    const int32_t *valid = a.ints + W.o_valid;
    for (int j = 0; j < F; ++j) {
        if (s_key[j]) continue;
        const int p0 = S->pt_off[j], p1 = S->pt_off[j + 1];
        for (int e = p0 + t; e < p1; e += AIF_NT) {
            const int k = aif_bisect(a.sorted_id + tro, ntr, a.t.ids[pbase + e]);
            int tr = k >= 0 ? a.sorted_tr[tro + k] : ntr;
            if (tr < ntr && valid[tr] == 0) tr = ntr;
            a.ints[a.o_op + obase + e] = tr;
            a.dd[a.o_obs + 2 * (obase + e)] = a.t.pts[2 * (pbase + e)];
            a.dd[a.o_obs + 2 * (obase + e) + 1] = a.t.pts[2 * (pbase + e) + 1];
        }
    }
}

__global__ __launch_bounds__(AIF_WAVE) void k_aif_finish(AifStructArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const int slot = a.slot[i];
    vio_aif_slot *S = a.t.slot + slot;
    const int F = S->n_frames;
    const int32_t *wk = a.walk + 66 * i;
    const int st = wk[0];
    const int j = lane < AIF_MAX_FRAMES ? lane : 0;
    const bool frame = lane < AIF_MAX_FRAMES && lane < F, key = frame && wk[2 + j] != 0, solved = st == AIF_STATUS_OK && frame && !key;
    const double *o = a.pnp_out + (int64_t)FO * (AIF_MAX_FRAMES * i + j);
    const int fs = solved ? (int)o[0] : VIO_OK;
    const unsigned long long failed = __ballot(solved && fs != VIO_OK), nonfin = __ballot(solved && fs == VIO_ERR_NOT_FINITE);
    const bool bad = nonfin != 0ull;
    if (lane < AIF_MAX_FRAMES) {
        const int row = AIF_MAX_FRAMES * i + lane;
        vio_pnp_frame_info fi;
        fi.status = VIO_OK; fi.iterations = 0; fi.n_used = 0; fi.reserved = 0; fi.cost = 0.0;
        if (solved) {
            fi.status = bad ? VIO_ERR_NOT_FINITE : fs;
            fi.iterations = bad ? 0 : (int)o[1];
            fi.n_used = bad ? 0 : (int)o[2];
            fi.cost = bad ? NAN : o[3];
            double R[9], T[3];
            for (int c = 0; c < 9; ++c) R[c] = NAN;
            for (int c = 0; c < 3; ++c) T[c] = NAN;
            if (!bad && fs == VIO_OK) {             // :365-373
                double Rq[9];
                aif_quat_to_rot(o + 4, Rq);
                aif_mul_rict(Rq, a.ric + 9 * i, R);
                for (int c = 0; c < 3; ++c) T[c] = o[8 + c];
            }
            for (int c = 0; c < 9; ++c) { S->R[lane][c] = R[c]; a.R_out[9 * row + c] = R[c]; }
            for (int c = 0; c < 3; ++c) { S->T[lane][c] = T[c]; a.T_out[3 * row + c] = T[c]; }
            S->is_key[lane] = 0;
        } else if (!key || st != AIF_STATUS_OK) {   // nothing was solved: the caller's rows say so, the slot stays
            for (int c = 0; c < 9; ++c) a.R_out[9 * row + c] = NAN;
            for (int c = 0; c < 3; ++c) a.T_out[3 * row + c] = NAN;
        }
        a.key_out[row] = st == AIF_STATUS_OK && key ? 1 : 0;
        a.info[row] = fi;
    }
    if (lane == 0) {
        vio_aif_structure_result *r = a.res + i;
        if (bad) { r->pnp_status = VIO_ERR_NOT_FINITE; r->fail_frame = -1; }
        else if (failed != 0ull) {
            const int ff = __ffsll((long long)failed) - 1;
            r->fail_frame = ff;
            r->pnp_status = (int)a.pnp_out[(int64_t)FO * (AIF_MAX_FRAMES * i + ff)];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
struct vio_aif {
    int device = 0;
    StreamEvents<3> q;                              // the caller's stream or an owned one, and the timing events
    ErrText err = {0};
    vio_aif_config cfg;
    DevBuf<char> data;                              // slot | off | first | dt | acc | gyr | ids | pts
    AifTables t = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    Twin<char> in, out;
    DevBuf<char> work;                              // the structure call's device-only tables, the PnP's scratch and its rows
    int32_t n_frames[VIO_AIF_MAX_SLOTS];            // what the results of this handle's calls said: the slot's frames,
    double last_t[VIO_AIF_MAX_SLOTS];               // ... and its last header (valid where n_frames > 0)
    double timing[4] = {0, 0, 0, 0};
};

namespace {

constexpr size_t kNS = VIO_AIF_MAX_SLOTS, kSamples = (size_t)VIO_AIF_MAX_SLOTS * VIO_AIF_MAX_SAMPLES,
                 kPoints = (size_t)VIO_AIF_MAX_SLOTS * VIO_AIF_MAX_POINTS;

vio_aif_config default_config() {
    vio_aif_config c;
    std::memset(&c, 0, sizeof c);
    c.noise[0] = 0.2687; c.noise[1] = 0.2121; c.noise[2] = 7.07e-6; c.noise[3] = 7.07e-7;
    c.min_points = VIO_PNP_DEFAULT_MIN_POINTS;
    return c;
}

// clearState on a host image: acc_0 / gyr_0 stay
void reset_image(vio_aif_slot &s) {
    double acc[3], gyr[3];
    std::memcpy(acc, s.acc_0, sizeof acc);
    std::memcpy(gyr, s.gyr_0, sizeof gyr);
    std::memset(&s, 0, sizeof s);
    std::memcpy(s.acc_0, acc, sizeof acc);
    std::memcpy(s.gyr_0, gyr, sizeof gyr);
}

bool all_finite(const double *v, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// the checks every batched call shares: the count and the two arrays, then every item's slot
vio_status check_slots(vio_aif *h, int32_t count, const void *items, const void *results, const char *what) {
    if (count < 0 || count > VIO_AIF_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "%s: count %d outside [0, %d]", what, count, VIO_AIF_MAX_SLOTS);
    if (count > 0 && (!items || !results)) return fail(h->err, VIO_ERR_BAD_ARG, "%s: items / results is NULL", what);
    return VIO_OK;
}

template <class Item> vio_status check_distinct(vio_aif *h, int32_t count, const Item *items, const char *what) {
    bool seen[VIO_AIF_MAX_SLOTS] = {false};
    for (int32_t i = 0; i < count; ++i) {
        const int32_t s = items[i].slot;
        if (s < 0 || s >= VIO_AIF_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d outside [0, %d)", what, i, s, VIO_AIF_MAX_SLOTS);
        if (seen[s]) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d is listed twice", what, i, s);
        seen[s] = true;
    }
    return VIO_OK;
}

struct CallClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// the tail every batched call shares: results (and what lies behind them, nout bytes in all) down, one wait, the timing
vio_status finish(vio_aif *h, const CallClock &clk, double t_host, int32_t count, size_t nout, vio_aif_result *results, const char *what) {
    vio_status st;
    hipEventRecord(h->q.ev[1], h->q.stream);
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->out.h, h->out.d, nout, hipMemcpyDeviceToHost, h->q.stream), "read-back")) != VIO_OK) return st;
    hipEventRecord(h->q.ev[2], h->q.stream);
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), what)) != VIO_OK) return st;
    std::memcpy(results, h->out.h, sizeof(vio_aif_result) * (size_t)count);
    h->timing[0] = t_host;
    h->timing[1] = elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[2] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    h->timing[3] = clk.ms();
    return VIO_OK;
}

}  // namespace

extern "C" {

void vio_aif_destroy(vio_aif *h) { destroy_handle(h); }

vio_status vio_aif_create(int32_t device, void *stream, vio_aif **out) {
    return create_handle(device, stream, out, vio_aif_destroy, [](vio_aif *h) {
        h->cfg = default_config();
        std::memset(h->n_frames, 0, sizeof h->n_frames);
        std::memset(h->last_t, 0, sizeof h->last_t);
        const size_t oSlot = 0, oOff = align256(oSlot + sizeof(vio_aif_slot) * kNS), oFirst = align256(oOff + 8 * AIF_OFFS * kNS),
                     oDt = align256(oFirst + 48 * AIF_OFFS * kNS), oAcc = align256(oDt + 8 * kSamples), oGyr = align256(oAcc + 24 * kSamples),
                     oIds = align256(oGyr + 24 * kSamples), oPts = align256(oIds + 8 * kPoints), total = align256(oPts + 16 * kPoints);
        if (h->data.ensure(h->err, total) != VIO_OK) return false;
        if (hipMemsetAsync(h->data.d, 0, total, h->q.stream) != hipSuccess) return false;
        h->t.slot = (vio_aif_slot *)(h->data.d + oSlot);
        h->t.off = (int64_t *)(h->data.d + oOff);
        h->t.first = (double *)(h->data.d + oFirst);
        h->t.dt = (double *)(h->data.d + oDt);
        h->t.acc = (double *)(h->data.d + oAcc);
        h->t.gyr = (double *)(h->data.d + oGyr);
        h->t.ids = (int64_t *)(h->data.d + oIds);
        h->t.pts = (double *)(h->data.d + oPts);
        std::vector<int64_t> off(AIF_OFFS * kNS);
        for (size_t s = 0; s < kNS; ++s)
            for (int j = 0; j < AIF_OFFS; ++j) off[AIF_OFFS * s + j] = (int64_t)s * VIO_AIF_MAX_SAMPLES;
        if (hipMemcpyAsync(h->t.off, off.data(), 8 * off.size(), hipMemcpyHostToDevice, h->q.stream) != hipSuccess) return false;
        return hipStreamSynchronize(h->q.stream) == hipSuccess;
    });
}

const char *vio_aif_last_error(const vio_aif *h) { return h ? h->err : "NULL handle"; }

int32_t vio_aif_version(void) { return VIO_AIF_VERSION; }

vio_status vio_aif_set_config(vio_aif *h, const vio_aif_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg) return fail(h->err, VIO_ERR_BAD_ARG, "cfg is NULL");
    if (!all_finite(cfg->noise, 4)) return fail(h->err, VIO_ERR_BAD_ARG, "a non-finite entry in the config");
    if (cfg->min_points < 3 || cfg->min_points > VIO_PNP_MAX_POINTS)
        return fail(h->err, VIO_ERR_BAD_ARG, "min_points %d outside [3, %d]", cfg->min_points, VIO_PNP_MAX_POINTS);
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_aif_reset(vio_aif *h, int32_t slot) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_AIF_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "slot %d outside [0, %d)", slot, VIO_AIF_MAX_SLOTS);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    vio_aif_slot s;
    if ((st = hip_ck(h->err, hipMemcpyAsync(&s, h->t.slot + slot, sizeof s, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;
    reset_image(s);
    int64_t off[AIF_OFFS];
    for (int j = 0; j < AIF_OFFS; ++j) off[j] = (int64_t)slot * VIO_AIF_MAX_SAMPLES;
    double first[6 * AIF_OFFS] = {0};
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->t.slot + slot, &s, sizeof s, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->t.off + AIF_OFFS * slot, off, sizeof off, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->t.first + 6 * AIF_OFFS * slot, first, sizeof first, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;
    h->n_frames[slot] = 0;
    return VIO_OK;
}

vio_status vio_aif_frames_get(vio_aif *h, int32_t slot, vio_aif_slot *slot_out, int64_t cap_points, int64_t *ids, double *pts, int64_t cap_samples,
                              double *dt, double *acc, double *gyr) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_AIF_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "slot %d outside [0, %d)", slot, VIO_AIF_MAX_SLOTS);
    if (!slot_out || cap_points < 0 || cap_samples < 0) return fail(h->err, VIO_ERR_BAD_ARG, "slot_out is NULL, or a capacity below 0");
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    int64_t aoff[AIF_OFFS];
    if ((st = hip_ck(h->err, hipMemcpyAsync(slot_out, h->t.slot + slot, sizeof *slot_out, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK ||
        (st = hip_ck(h->err, hipMemcpyAsync(aoff, h->t.off + AIF_OFFS * slot, sizeof aoff, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK ||
        (st = hip_ck(h->err, hipMemcpyAsync(slot_out->first, h->t.first + 6 * AIF_OFFS * slot, sizeof slot_out->first, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK) {
        (void)hipStreamSynchronize(h->q.stream);
        return st;
    }
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;
    const int64_t sbase = (int64_t)slot * VIO_AIF_MAX_SAMPLES, pbase = (int64_t)slot * VIO_AIF_MAX_POINTS;
    for (int j = 0; j < AIF_OFFS; ++j) slot_out->samp_off[j] = aoff[j] - sbase;
    const int64_t S = slot_out->samp_off[AIF_OFFS - 1], P = slot_out->n_points;
    if (S > cap_samples || P > cap_points)
        return fail(h->err, VIO_ERR_BAD_ARG, "the slot holds %lld samples and %lld points, the capacities are %lld and %lld", (long long)S, (long long)P,
                    (long long)cap_samples, (long long)cap_points);
    if ((S > 0 && (!dt || !acc || !gyr)) || (P > 0 && (!ids || !pts))) return fail(h->err, VIO_ERR_BAD_ARG, "an array is NULL and its count is not 0");
    struct { void *d; const void *s; size_t b; } cp[5] = {{dt, h->t.dt + sbase, 8 * (size_t)S}, {acc, h->t.acc + 3 * sbase, 24 * (size_t)S},
                                                          {gyr, h->t.gyr + 3 * sbase, 24 * (size_t)S}, {ids, h->t.ids + pbase, 8 * (size_t)P},
                                                          {pts, h->t.pts + 2 * pbase, 16 * (size_t)P}};
    for (auto &c : cp)
        if (c.b && (st = hip_ck(h->err, hipMemcpyAsync(c.d, c.s, c.b, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK) {
            (void)hipStreamSynchronize(h->q.stream);
            return st;
        }
    return hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize");
}

vio_status vio_aif_imu_batch(vio_aif *h, int32_t count, const vio_aif_imu_item *items, vio_aif_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "imu_batch")) != VIO_OK || (st = check_distinct(h, count, items, "imu_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    size_t S = 0;
    for (int32_t i = 0; i < count; ++i) {
        const vio_aif_imu_item &it = items[i];
        if (it.n < 0 || it.n > VIO_AIF_MAX_SAMPLES) return fail(h->err, VIO_ERR_BAD_ARG, "imu_batch: item %d: n = %d outside [0, %d]", i, it.n, VIO_AIF_MAX_SAMPLES);
        if (it.n > 0 && (!it.dt || !it.acc || !it.gyr)) return fail(h->err, VIO_ERR_BAD_ARG, "imu_batch: item %d: dt / acc / gyr is NULL", i);
        if (!all_finite(it.dt, (size_t)it.n) || !all_finite(it.acc, 3 * (size_t)it.n) || !all_finite(it.gyr, 3 * (size_t)it.n))
            return fail(h->err, VIO_ERR_BAD_ARG, "imu_batch: item %d: a non-finite sample", i);
        S += (size_t)it.n;
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t oSlot = 0, oOff = align256(oSlot + 4 * (size_t)count), oDt = align256(oOff + 8 * ((size_t)count + 1)), oAcc = align256(oDt + 8 * S),
                 oGyr = align256(oAcc + 24 * S), nin = align256(oGyr + 24 * S), nout = sizeof(vio_aif_result) * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    int32_t *hs = (int32_t *)(h->in.h + oSlot);
    int64_t *ho = (int64_t *)(h->in.h + oOff);
    double *hdt = (double *)(h->in.h + oDt), *hacc = (double *)(h->in.h + oAcc), *hgyr = (double *)(h->in.h + oGyr);
    ho[0] = 0;
    for (int32_t i = 0; i < count; ++i) {
        const vio_aif_imu_item &it = items[i];
        hs[i] = it.slot;
        if (it.n > 0) {
            std::memcpy(hdt + ho[i], it.dt, 8 * (size_t)it.n);
            std::memcpy(hacc + 3 * ho[i], it.acc, 24 * (size_t)it.n);
            std::memcpy(hgyr + 3 * ho[i], it.gyr, 24 * (size_t)it.n);
        }
        ho[i + 1] = ho[i] + it.n;
    }
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    AifImuArgs a;
    a.t = h->t;
    a.slot = (const int32_t *)(h->in.d + oSlot); a.in_off = (const int64_t *)(h->in.d + oOff);
    a.in_dt = (const double *)(h->in.d + oDt); a.in_acc = (const double *)(h->in.d + oAcc); a.in_gyr = (const double *)(h->in.d + oGyr);
    a.res = (vio_aif_result *)h->out.d;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_aif_imu, dim3(count), dim3(AIF_WAVE), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_aif_imu launch");
    return finish(h, clk, t_host, count, nout, results, "k_aif_imu");
}

vio_status vio_aif_image_batch(vio_aif *h, int32_t count, const vio_aif_image_item *items, vio_aif_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "image_batch")) != VIO_OK || (st = check_distinct(h, count, items, "image_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    size_t P = 0;
    std::vector<int64_t> sorted;
    for (int32_t i = 0; i < count; ++i) {
        const vio_aif_image_item &it = items[i];
        if (it.n < 0 || it.n > VIO_AIF_MAX_FRAME_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "image_batch: item %d: n = %d outside [0, %d]", i, it.n, VIO_AIF_MAX_FRAME_POINTS);
        if (it.n > 0 && (!it.ids || !it.pts)) return fail(h->err, VIO_ERR_BAD_ARG, "image_batch: item %d: ids / pts is NULL", i);
        if (!std::isfinite(it.t) || !all_finite(it.ba, 3) || !all_finite(it.bg, 3) || !all_finite(it.pts, 2 * (size_t)it.n))
            return fail(h->err, VIO_ERR_BAD_ARG, "image_batch: item %d: a non-finite header, bias or point", i);
        if (h->n_frames[it.slot] > 0 && !(it.t > h->last_t[it.slot]))
            return fail(h->err, VIO_ERR_BAD_ARG, "image_batch: item %d: header %.17g is not greater than the slot's last one, %.17g", i, it.t, h->last_t[it.slot]);
        sorted.assign(it.ids, it.ids + it.n);
        std::sort(sorted.begin(), sorted.end());
        for (int32_t e = 1; e < it.n; ++e)
            if (sorted[e] == sorted[e - 1]) return fail(h->err, VIO_ERR_BAD_ARG, "image_batch: item %d: feature id %lld is listed twice", i, (long long)sorted[e]);
        P += (size_t)it.n;
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t oSlot = 0, oOff = align256(oSlot + 4 * (size_t)count), oHdr = align256(oOff + 8 * ((size_t)count + 1)), oBias = align256(oHdr + 8 * (size_t)count),
                 oIds = align256(oBias + 48 * (size_t)count), oPts = align256(oIds + 8 * P), nin = align256(oPts + 16 * P),
                 nout = sizeof(vio_aif_result) * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    int32_t *hs = (int32_t *)(h->in.h + oSlot);
    int64_t *ho = (int64_t *)(h->in.h + oOff), *hid = (int64_t *)(h->in.h + oIds);
    double *hh = (double *)(h->in.h + oHdr), *hb = (double *)(h->in.h + oBias), *hp = (double *)(h->in.h + oPts);
    ho[0] = 0;
    for (int32_t i = 0; i < count; ++i) {
        const vio_aif_image_item &it = items[i];
        hs[i] = it.slot;
        hh[i] = it.t;
        for (int c = 0; c < 3; ++c) { hb[6 * i + c] = it.ba[c]; hb[6 * i + 3 + c] = it.bg[c]; }
        if (it.n > 0) {
            std::memcpy(hid + ho[i], it.ids, 8 * (size_t)it.n);
            std::memcpy(hp + 2 * ho[i], it.pts, 16 * (size_t)it.n);
        }
        ho[i + 1] = ho[i] + it.n;
    }
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    AifImageArgs a;
    a.t = h->t;
    a.slot = (const int32_t *)(h->in.d + oSlot); a.in_off = (const int64_t *)(h->in.d + oOff); a.in_ids = (const int64_t *)(h->in.d + oIds);
    a.in_pts = (const double *)(h->in.d + oPts); a.header = (const double *)(h->in.d + oHdr); a.bias = (const double *)(h->in.d + oBias);
    a.res = (vio_aif_result *)h->out.d;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_aif_image, dim3(count), dim3(AIF_NT), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_aif_image launch");
    if ((st = finish(h, clk, t_host, count, nout, results, "k_aif_image")) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i) {
        h->n_frames[items[i].slot] = results[i].n_frames;
        if (results[i].status == VIO_AIF_STATUS_OK) h->last_t[items[i].slot] = items[i].t;
    }
    return VIO_OK;
}

vio_status vio_aif_slide_batch(vio_aif *h, int32_t count, const vio_aif_slide_item *items, vio_aif_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "slide_batch")) != VIO_OK || (st = check_distinct(h, count, items, "slide_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    for (int32_t i = 0; i < count; ++i)
        if (!std::isfinite(items[i].t_0)) return fail(h->err, VIO_ERR_BAD_ARG, "slide_batch: item %d: a non-finite t_0", i);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t oSlot = 0, oT = align256(oSlot + 4 * (size_t)count), nin = align256(oT + 8 * (size_t)count), nout = sizeof(vio_aif_result) * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i) {
        ((int32_t *)(h->in.h + oSlot))[i] = items[i].slot;
        ((double *)(h->in.h + oT))[i] = items[i].t_0;
    }
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    AifSlideArgs a;
    a.t = h->t;
    a.slot = (const int32_t *)(h->in.d + oSlot); a.t_0 = (const double *)(h->in.d + oT);
    a.res = (vio_aif_result *)h->out.d;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_aif_slide, dim3(count), dim3(AIF_NT), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_aif_slide launch");
    if ((st = finish(h, clk, t_host, count, nout, results, "k_aif_slide")) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i) h->n_frames[items[i].slot] = results[i].n_frames;      // (the last header stays the last)
    return VIO_OK;
}

vio_status vio_aif_propagate_batch(vio_aif *h, int32_t count, const vio_aif_propagate_item *items, vio_aif_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "propagate_batch")) != VIO_OK || (st = check_distinct(h, count, items, "propagate_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    size_t nrec = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int F = h->n_frames[items[i].slot];
        if (!all_finite(items[i].ba, 3) || !all_finite(items[i].bg, 3)) return fail(h->err, VIO_ERR_BAD_ARG, "propagate_batch: item %d: a non-finite bias", i);
        if (F > 1 && !items[i].pre) return fail(h->err, VIO_ERR_BAD_ARG, "propagate_batch: item %d: pre is NULL", i);
        nrec += F > 1 ? (size_t)(F - 1) : 0;
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t oSlot = 0, oBias = align256(oSlot + 4 * (size_t)count), oWhich = align256(oBias + 48 * nrec), nin = align256(oWhich + 4 * nrec);
    const size_t oRec = align256(sizeof(vio_aif_result) * (size_t)count), nout = oRec + 8 * IMU_REC * nrec;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    double *hb = (double *)(h->in.h + oBias);
    int *hw = (int *)(h->in.h + oWhich);
    size_t k = 0;
    for (int32_t i = 0; i < count; ++i) {
        ((int32_t *)(h->in.h + oSlot))[i] = items[i].slot;
        for (int j = 1; j < h->n_frames[items[i].slot]; ++j, ++k) {         // record k: interval j of the slot at the item's biases
            hw[k] = AIF_OFFS * items[i].slot + j;
            for (int c = 0; c < 3; ++c) { hb[6 * k + c] = items[i].ba[c]; hb[6 * k + 3 + c] = items[i].bg[c]; }
        }
    }
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    AifInfoArgs e;
    e.t = h->t;
    e.slot = (const int32_t *)(h->in.d + oSlot);
    e.res = (vio_aif_result *)h->out.d;
    e.count = count;
    ImuArgs a;
    a.off = h->t.off; a.first = h->t.first; a.dt = h->t.dt; a.acc = h->t.acc; a.gyr = h->t.gyr;
    a.bias = (const double *)(h->in.d + oBias); a.which = (const int *)(h->in.d + oWhich);
    a.out = (double *)(h->out.d + oRec);
    for (int c = 0; c < 4; ++c) a.sn[c] = h->cfg.noise[c];
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_aif_info, dim3((count + AIF_WAVE - 1) / AIF_WAVE), dim3(AIF_WAVE), 0, h->q.stream, e);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_aif_info launch");
    if (nrec > 0) {
        hipLaunchKernelGGL(k_imu_propagate, dim3((unsigned)nrec), dim3(IMU_NT), 0, h->q.stream, a);
        if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_imu_propagate launch");
    }
    if ((st = finish(h, clk, t_host, count, nout, results, "k_aif_info, k_imu_propagate")) != VIO_OK) return st;
    const double *rec = (const double *)(h->out.h + oRec);
    k = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int F = h->n_frames[items[i].slot];
        if (F > 1) {
            std::memcpy(items[i].pre, rec + (size_t)IMU_REC * k, sizeof(vio_preint) * (size_t)(F - 1));
            k += (size_t)(F - 1);
        }
    }
    h->timing[3] = clk.ms();
    return VIO_OK;
}

vio_status vio_aif_structure_batch(vio_aif *h, int32_t count, const vio_aif_structure_item *items, vio_aif_structure_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "structure_batch")) != VIO_OK || (st = check_distinct(h, count, items, "structure_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    size_t nrec = 0, ntrk = 0;
    std::vector<int64_t> sorted;
    for (int32_t i = 0; i < count; ++i) {
        const vio_aif_structure_item &it = items[i];
        const int F = h->n_frames[it.slot];
        if (it.n_key < 1 || it.n_key > VIO_AIF_MAX_KEY) return fail(h->err, VIO_ERR_BAD_ARG, "structure_batch: item %d: n_key = %d outside [1, %d]", i, it.n_key, VIO_AIF_MAX_KEY);
        if (it.n_tracks < 0 || it.n_tracks > VIO_AIF_MAX_TRACKS)
            return fail(h->err, VIO_ERR_BAD_ARG, "structure_batch: item %d: n_tracks = %d outside [0, %d]", i, it.n_tracks, VIO_AIF_MAX_TRACKS);
        if (!it.headers || !it.Q || !it.T || (it.n_tracks > 0 && (!it.track_ids || !it.points || !it.state)))
            return fail(h->err, VIO_ERR_BAD_ARG, "structure_batch: item %d: headers / Q / T / track_ids / points / state is NULL", i);
        if (F > 0 && (!it.R || !it.T_out || !it.is_key || (F > 1 && !it.pre))) return fail(h->err, VIO_ERR_BAD_ARG, "structure_batch: item %d: an out array is NULL", i);
        if (!all_finite(it.headers, (size_t)it.n_key) || !all_finite(it.ric, 9)) return fail(h->err, VIO_ERR_BAD_ARG, "structure_batch: item %d: a non-finite header or ric", i);
        if (!all_finite(it.Q, 4 * (size_t)it.n_key) || !all_finite(it.T, 3 * (size_t)it.n_key)) return fail(h->err, VIO_ERR_BAD_ARG, "structure_batch: item %d: a non-finite keyframe pose", i);
        sorted.assign(it.track_ids, it.track_ids + it.n_tracks);
        std::sort(sorted.begin(), sorted.end());
        for (int32_t e = 1; e < it.n_tracks; ++e)
            if (sorted[e] == sorted[e - 1]) return fail(h->err, VIO_ERR_BAD_ARG, "structure_batch: item %d: track id %lld is listed twice", i, (long long)sorted[e]);
        nrec += F > 1 ? (size_t)(F - 1) : 0;
        ntrk += (size_t)it.n_tracks + 1;
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t n = (size_t)count, nfr = n * VIO_AIF_MAX_FRAMES, nobs = n * VIO_AIF_MAX_POINTS;
    // uploaded: slot | n_key | n_tracks | tr_off | rec_off | headers | ric | which | track ids | wins | ints: valid | dd: points, Q, T
    const size_t oSlot = 0, oNk = align256(oSlot + 4 * n), oNt = align256(oNk + 4 * n), oTro = align256(oNt + 4 * n), oRco = align256(oTro + 8 * (n + 1)),
                 oHdr = align256(oRco + 8 * (n + 1)), oRic = align256(oHdr + 8 * AIF_MAX_KEY * n), oWhich = align256(oRic + 72 * n), oIds = align256(oWhich + 4 * nrec),
                 oWin = align256(oIds + 8 * ntrk), oInts = align256(oWin + sizeof(PnpWin) * n), oDd = align256(oInts + 4 * ntrk),
                 nup = align256(oDd + 8 * (3 * ntrk + 7 * AIF_MAX_KEY * n));
    const size_t oSid = 0, oStr = align256(oSid + 8 * ntrk), oFr = align256(oStr + 4 * ntrk), oBias = align256(oFr + sizeof(PnpFrame) * nfr),
                 oWalk = align256(oBias + 48 * nrec), oPnp = align256(oWalk + 4 * 66 * n), oScr = align256(oPnp + 8 * FO * nfr);
    // the PnP's arena, device only (no pinned twin): the uploaded ints and dd parts are copied to its front, and obs_point / obs_pts, which
    // k_aif_join writes, lie behind them so that the PnP's two bases reach both: obs_point from the ints base, obs_pts from the dd base
    const size_t aInts = align256(oScr + 8 * PD * nobs), aDd = aInts + (oDd - oInts), aOp = align256(aInts + (nup - oInts)), aObs = align256(aOp + 4 * nobs),
                 nwork = align256(aObs + 16 * nobs);
    const size_t oRes = 0, oR = align256(oRes + sizeof(vio_aif_structure_result) * n), oT = align256(oR + 72 * nfr), oKey = align256(oT + 24 * nfr),
                 oInfo = align256(oKey + 4 * nfr), oRec = align256(oInfo + sizeof(vio_pnp_frame_info) * nfr), nout = oRec + 8 * IMU_REC * nrec;
    if ((st = h->in.ensure(h->err, nup)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK || (st = h->work.ensure(h->err, nwork)) != VIO_OK) return st;
    char *H = h->in.h;
    int64_t *tro = (int64_t *)(H + oTro), *rco = (int64_t *)(H + oRco), *hid = (int64_t *)(H + oIds);
    int32_t *hv = (int32_t *)(H + oInts);
    int *hw = (int *)(H + oWhich);
    double *hd = (double *)(H + oDd);
    PnpWin *wins = (PnpWin *)(H + oWin);
    tro[0] = 0; rco[0] = 0;
    int64_t nd = 0;
    for (int32_t i = 0; i < count; ++i) {
        const vio_aif_structure_item &it = items[i];
        const int F = h->n_frames[it.slot];
        ((int32_t *)(H + oSlot))[i] = it.slot; ((int32_t *)(H + oNk))[i] = it.n_key; ((int32_t *)(H + oNt))[i] = it.n_tracks;
        double *hh = (double *)(H + oHdr) + (size_t)AIF_MAX_KEY * i;
        for (int k = 0; k < AIF_MAX_KEY; ++k) hh[k] = k < it.n_key ? it.headers[k] : 0.0;
        std::memcpy((double *)(H + oRic) + 9 * (size_t)i, it.ric, 72);
        for (int j = 1; j < F; ++j) hw[rco[i] + j - 1] = AIF_OFFS * it.slot + j;
        rco[i + 1] = rco[i] + (F > 1 ? F - 1 : 0);
        PnpWin &w = wins[i];
        std::memset(&w, 0, sizeof w);
        w.np = it.n_tracks + 1; w.has_valid = 1;
        w.o_valid = tro[i];
        for (int e = 0; e < it.n_tracks; ++e) { hid[tro[i] + e] = it.track_ids[e]; hv[tro[i] + e] = it.state[e] != 0; }
        hid[tro[i] + it.n_tracks] = 0; hv[tro[i] + it.n_tracks] = 0;       // the extra row: never valid
        w.o_pts = nd;
        if (it.n_tracks) std::memcpy(hd + nd, it.points, 24 * (size_t)it.n_tracks);
        nd += 3 * (int64_t)it.n_tracks;
        hd[nd] = hd[nd + 1] = hd[nd + 2] = 0.0; nd += 3;
        w.o_key = nd; std::memcpy(hd + nd, it.Q, 32 * (size_t)it.n_key); nd += 4 * (int64_t)it.n_key;
        w.o_keyT = nd; std::memcpy(hd + nd, it.T, 24 * (size_t)it.n_key); nd += 3 * (int64_t)it.n_key;
        tro[i + 1] = tro[i] + it.n_tracks + 1;
    }
    char *D = h->in.d, *Wk = h->work.d, *O = h->out.d;
    if ((st = hip_ck(h->err, hipMemcpyAsync(D, H, oInts, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipMemcpyAsync(Wk + aInts, H + oInts, nup - oInts, hipMemcpyHostToDevice, h->q.stream), "upload of the PnP's arena")) != VIO_OK) return st;
    const double t_host = clk.ms();
    AifStructArgs a;
    a.t = h->t;
    a.slot = (const int32_t *)(D + oSlot); a.n_key = (const int32_t *)(D + oNk); a.n_tracks = (const int32_t *)(D + oNt);
    a.tr_off = (const int64_t *)(D + oTro); a.rec_off = (const int64_t *)(D + oRco);
    a.headers = (const double *)(D + oHdr); a.ric = (const double *)(D + oRic);
    a.track_ids = (const int64_t *)(D + oIds);
    a.sorted_id = (int64_t *)(Wk + oSid); a.sorted_tr = (int32_t *)(Wk + oStr);
    a.wins = (const PnpWin *)(D + oWin); a.frames = (PnpFrame *)(Wk + oFr);
    a.ints = (int32_t *)(Wk + aInts); a.dd = (double *)(Wk + aDd);
    a.o_op = (int64_t)((aOp - aInts) / 4); a.o_obs = (int64_t)((aObs - aDd) / 8);
    a.rec = (const double *)(O + oRec);
    a.pnp_out = (const double *)(Wk + oPnp);
    a.walk = (int32_t *)(Wk + oWalk);
    a.res = (vio_aif_structure_result *)(O + oRes);
    a.R_out = (double *)(O + oR); a.T_out = (double *)(O + oT); a.key_out = (int32_t *)(O + oKey); a.info = (vio_pnp_frame_info *)(O + oInfo);
    ImuArgs m;
    m.off = h->t.off; m.first = h->t.first; m.dt = h->t.dt; m.acc = h->t.acc; m.gyr = h->t.gyr;
    m.bias = (const double *)(Wk + oBias); m.which = (const int *)(D + oWhich);
    m.out = (double *)(O + oRec);
    for (int c = 0; c < 4; ++c) m.sn[c] = h->cfg.noise[c];
    PnpArgs p;
    p.wins = a.wins; p.frames = a.frames; p.ints = a.ints; p.dd = a.dd;
    p.scr = (double *)(Wk + oScr); p.out = (double *)(Wk + oPnp);
    p.nframes = (int32_t)nfr; p.min_points = h->cfg.min_points;
    hipEventRecord(h->q.ev[0], h->q.stream);
    if (nrec > 0) {
        hipLaunchKernelGGL(k_aif_bias, dim3((unsigned)((nrec + AIF_WAVE - 1) / AIF_WAVE)), dim3(AIF_WAVE), 0, h->q.stream, h->t, m.which, (double *)(Wk + oBias), (int)nrec);
        if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_aif_bias launch");
        hipLaunchKernelGGL(k_imu_propagate, dim3((unsigned)nrec), dim3(IMU_NT), 0, h->q.stream, m);
        if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_imu_propagate launch");
    }
    hipLaunchKernelGGL(k_aif_join, dim3(count), dim3(AIF_NT), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_aif_join launch");
    hipLaunchKernelGGL(k_pnp_frames, dim3((unsigned)((nfr + WAVES - 1) / WAVES)), dim3(NT), 0, h->q.stream, p);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_pnp_frames launch");
    hipLaunchKernelGGL(k_aif_finish, dim3(count), dim3(AIF_WAVE), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_aif_finish launch");
    hipEventRecord(h->q.ev[1], h->q.stream);
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->out.h, h->out.d, nout, hipMemcpyDeviceToHost, h->q.stream), "read-back")) != VIO_OK) return st;
    hipEventRecord(h->q.ev[2], h->q.stream);
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "structure_batch")) != VIO_OK) return st;
    std::memcpy(results, h->out.h + oRes, sizeof(vio_aif_structure_result) * n);
    const double *rec = (const double *)(h->out.h + oRec);
    for (int32_t i = 0; i < count; ++i) {
        const vio_aif_structure_item &it = items[i];
        const size_t F = (size_t)h->n_frames[it.slot], row = (size_t)VIO_AIF_MAX_FRAMES * i;
        if (F == 0) continue;
        std::memcpy(it.R, (const double *)(h->out.h + oR) + 9 * row, 72 * F);
        std::memcpy(it.T_out, (const double *)(h->out.h + oT) + 3 * row, 24 * F);
        for (size_t j = 0; j < F; ++j) it.is_key[j] = (uint8_t)(((const int32_t *)(h->out.h + oKey))[row + j] != 0);
        if (it.frame_info) std::memcpy(it.frame_info, (const vio_pnp_frame_info *)(h->out.h + oInfo) + row, sizeof(vio_pnp_frame_info) * F);
        if (F > 1) std::memcpy(it.pre, rec + (size_t)IMU_REC * (size_t)rco[i], sizeof(vio_preint) * (F - 1));
    }
    h->timing[0] = t_host;
    h->timing[1] = elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[2] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    h->timing[3] = clk.ms();
    return VIO_OK;
}

vio_status vio_aif_timing(const vio_aif *h, double *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->timing, sizeof(h->timing));
    return VIO_OK;
}

}   // extern "C"
