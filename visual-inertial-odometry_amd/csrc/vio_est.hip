// vio_est.hip — the Estimator's window state and IMU buffers of many streams (include/vio_est.h).
//
// A handle keeps, for VIO_EST_MAX_SLOTS slots: one vio_est_state each (d_state), 12 absolute sample offsets each (d_off), the
// constructor samples of every interval (d_first, 12 rows of 6 per slot, row 11 unused) and one region of VIO_EST_MAX_SAMPLES samples
// each in d_dt / d_acc / d_gyr.  Interval (slot, j) is thereby CSR interval 12 slot + j of csrc/vio_imu_body.inc's ImuArgs, and
// vio_est_window_batch launches k_imu_propagate, the kernel of libvio_imu_hip, straight over the resident tables.
//   k_est_imu      one wavefront per item: the lanes stride over the copy of the run into the slot's region, lane 0 carries the
//                  serial recurrence (csrc/vio_est_math.h's est_imu_step) and the bookkeeping
//   k_est_image    one thread per item
//   k_est_export   one wavefront per item: lane i < 11 writes frame i's pose and speed-bias, lane 11 the extrinsic, lanes 0..9 the
//                  (interval, bias) rows k_imu_propagate reads
//   k_est_update   one wavefront per item: every lane computes rot_diff, lane i < 11 writes frame i and its vector2double, lane 10
//                  holds the verdict
//   k_est_slide    one workgroup of EST_NT threads per item: the samples move down in chunks, read, barrier, write, barrier
// csrc/vio_est_init_body.inc, included at the end, adds k_est_init_apply and k_est_relinearize (include/vio_est_init.h).
// No atomics; every sum has the order the header writes down, so a slot's bits depend neither on the batch nor on the slot index.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vio_est.h"
#include "vio_companion.h"
#include "vio_est_math.h"
#include "vio_imu_body.inc"

#pragma clang fp contract(off)

#define EST_WAVE 64
#define EST_NT 256                          // threads of k_est_slide's workgroup: one chunk of samples
#define EST_WIN 183                         // doubles of one window: poses 77 | speed_bias 99 | ext 7
#define EST_W_SB 77
#define EST_W_EXT 176

static_assert(VIO_EST_MAX_SLOTS == EST_MAX_SLOTS && VIO_EST_MAX_SAMPLES == EST_MAX_SAMPLES && VIO_EST_FRAMES == EST_FRAMES &&
              VIO_EST_WINDOW_SIZE == EST_WINDOW, "vio_est.h and vio_est_math.h agree");
static_assert(VIO_EST_GATE_BA == EST_GATE_BA && VIO_EST_GATE_BG == EST_GATE_BG && VIO_EST_GATE_TRANSLATION == EST_GATE_TRANSLATION &&
              VIO_EST_GATE_Z == EST_GATE_Z, "the gates' numbers");
static_assert(sizeof(vio_est_state) == 64 + 419 * 8 && sizeof(vio_est_result) == 32 + 24 * 8, "the layouts the binding mirrors");

struct EstTables {
    vio_est_state *state;       // [VIO_EST_MAX_SLOTS]
    int64_t *off;               // [VIO_EST_MAX_SLOTS][12], absolute
    double *first;              // [VIO_EST_MAX_SLOTS][12][6]
    double *dt, *acc, *gyr;     // [VIO_EST_MAX_SLOTS * VIO_EST_MAX_SAMPLES] (x 3)
};

struct EstImuArgs {
    EstTables t;
    const int32_t *slot;        // [count]
    const int64_t *in_off;      // [count + 1] into in_dt / in_acc / in_gyr
    const double *in_dt, *in_acc, *in_gyr;
    vio_est_result *res;        // [count]
};

__device__ __forceinline__ void est_result_clear(vio_est_result *r) {
    r->status = 0; r->frame_count = 0; r->n_samples = 0; r->failure = 0; r->gate = 0; r->singular = 0; r->slid = 0; r->shift_depth = 0;
    for (int c = 0; c < 9; ++c) { r->marg_R[c] = 0.0; r->new_R[c] = 0.0; }
    for (int c = 0; c < 3; ++c) { r->marg_P[c] = 0.0; r->new_P[c] = 0.0; }
}

__global__ __launch_bounds__(EST_WAVE) void k_est_imu(EstImuArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const int slot = a.slot[i];
    vio_est_state *S = a.t.state + slot;
    int64_t *o = a.t.off + (int64_t)EST_OFFS * slot;
    const int64_t b = a.in_off[i];
    const int n = (int)(a.in_off[i + 1] - b);
    const int fc = S->frame_count;
    const int64_t end = o[EST_OFFS - 1];
    const int total = (int)(end - o[0]);
    const bool full = fc != 0 && total + n > EST_MAX_SAMPLES;
    if (!full && n > 0 && fc != 0)                  // the append (:124-126); interval fc is the last one that holds samples
        for (int s = lane; s < n; s += EST_WAVE) {
            a.t.dt[end + s] = a.in_dt[b + s];
            for (int c = 0; c < 3; ++c) {
                a.t.acc[3 * (end + s) + c] = a.in_acc[3 * (b + s) + c];
                a.t.gyr[3 * (end + s) + c] = a.in_gyr[3 * (b + s) + c];
            }
        }
    if (lane != 0) return;
    vio_est_result *r = a.res + i;
    est_result_clear(r);
    r->status = full ? VIO_EST_STATUS_POOL_FULL : VIO_EST_STATUS_OK;
    r->frame_count = fc;
    r->n_samples = total;
    if (full || n == 0) return;
    double acc0[3], gyr0[3];
    for (int c = 0; c < 3; ++c) { acc0[c] = S->acc_0[c]; gyr0[c] = S->gyr_0[c]; }
    if (!S->first_imu) {                            // :107-112
        S->first_imu = 1;
        for (int c = 0; c < 3; ++c) { acc0[c] = a.in_acc[3 * b + c]; gyr0[c] = a.in_gyr[3 * b + c]; }
    }
    if (!S->exists[fc]) {                           // :114-117
        S->exists[fc] = 1;
        double *f = a.t.first + 6 * ((int64_t)EST_OFFS * slot + fc);
        for (int c = 0; c < 3; ++c) {
            f[c] = acc0[c]; f[3 + c] = gyr0[c];
            S->lin_bias[fc][c] = S->Bas[fc][c]; S->lin_bias[fc][3 + c] = S->Bgs[fc][c];
        }
    }
    if (fc != 0) {                                  // :118-136
        double Rs[9], Ps[3], Vs[3], Ba[3], Bg[3], g[3];
        for (int c = 0; c < 9; ++c) Rs[c] = S->Rs[fc][c];
        for (int c = 0; c < 3; ++c) { Ps[c] = S->Ps[fc][c]; Vs[c] = S->Vs[fc][c]; Ba[c] = S->Bas[fc][c]; Bg[c] = S->Bgs[fc][c]; g[c] = S->g[c]; }
        for (int s = 0; s < n; ++s) {
            const double dt = a.in_dt[b + s];
            double acc[3], gyr[3];
            for (int c = 0; c < 3; ++c) { acc[c] = a.in_acc[3 * (b + s) + c]; gyr[c] = a.in_gyr[3 * (b + s) + c]; }
            est_imu_step(Rs, Ps, Vs, Ba, Bg, g, acc0, gyr0, dt, acc, gyr);
            for (int c = 0; c < 3; ++c) { acc0[c] = acc[c]; gyr0[c] = gyr[c]; }
        }
        for (int c = 0; c < 9; ++c) S->Rs[fc][c] = Rs[c];
        for (int c = 0; c < 3; ++c) { S->Ps[fc][c] = Ps[c]; S->Vs[fc][c] = Vs[c]; }
        for (int j = fc + 1; j < EST_OFFS; ++j) o[j] += n;
        r->n_samples = total + n;
    } else {
        for (int c = 0; c < 3; ++c) { acc0[c] = a.in_acc[3 * (b + n - 1) + c]; gyr0[c] = a.in_gyr[3 * (b + n - 1) + c]; }
    }
    for (int c = 0; c < 3; ++c) { S->acc_0[c] = acc0[c]; S->gyr_0[c] = gyr0[c]; }       // :137-138
}

struct EstImageArgs {
    EstTables t;
    const int32_t *slot;
    const int32_t *advance;
    const double *header;
    vio_est_result *res;
    int count;
};

__global__ __launch_bounds__(EST_WAVE) void k_est_image(EstImageArgs a) {
    const int i = blockIdx.x * EST_WAVE + threadIdx.x;
    if (i >= a.count) return;
    vio_est_state *S = a.t.state + a.slot[i];
    int fc = S->frame_count;
    S->Headers[fc] = a.header[i];                   // :154
    if (a.advance[i] && fc < EST_WINDOW) S->frame_count = ++fc;     // :206-207
    vio_est_result *r = a.res + i;
    est_result_clear(r);
    r->frame_count = fc;
}

struct EstExportArgs {
    EstTables t;
    const int32_t *slot;
    double *win;                // [count][EST_WIN]
    double *bias;               // [count * 10][6]: ImuArgs::bias
    int *which;                 // [count * 10]: ImuArgs::which
    vio_est_result *res;
};

__global__ __launch_bounds__(EST_WAVE) void k_est_export(EstExportArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const int slot = a.slot[i];
    const vio_est_state *S = a.t.state + slot;
    double *w = a.win + (int64_t)EST_WIN * i;
    if (lane < EST_FRAMES) {                        // vector2double, frame `lane` (:507-529)
        double R[9], q[4];
        for (int c = 0; c < 9; ++c) R[c] = S->Rs[lane][c];
        est_rot_to_quat(R, q);
        for (int c = 0; c < 3; ++c) {
            w[7 * lane + c] = S->Ps[lane][c];
            w[EST_W_SB + 9 * lane + c] = S->Vs[lane][c];
            w[EST_W_SB + 9 * lane + 3 + c] = S->Bas[lane][c];
            w[EST_W_SB + 9 * lane + 6 + c] = S->Bgs[lane][c];
        }
        for (int c = 0; c < 4; ++c) w[7 * lane + 3 + c] = q[c];
    } else if (lane == EST_FRAMES) {                // (:530-540)
        double R[9], q[4];
        for (int c = 0; c < 9; ++c) R[c] = S->ric[c];
        est_rot_to_quat(R, q);
        for (int c = 0; c < 3; ++c) w[EST_W_EXT + c] = S->tic[c];
        for (int c = 0; c < 4; ++c) w[EST_W_EXT + 3 + c] = q[c];
    }
    if (lane < EST_WINDOW) {                        // interval lane + 1 at its own construction biases
        const int j = lane + 1, k = EST_WINDOW * i + lane;
        const bool ex = S->exists[j] != 0;
        a.which[k] = EST_OFFS * slot + j;
        for (int c = 0; c < 6; ++c) a.bias[6 * k + c] = ex ? S->lin_bias[j][c] : 0.0;
    }
    if (lane == 0) {
        vio_est_result *r = a.res + i;
        est_result_clear(r);
        r->frame_count = S->frame_count;
    }
}

struct EstUpdateArgs {
    EstTables t;
    const int32_t *slot;
    const int32_t *commit;
    const double *win;          // [count][EST_WIN]
    double *wout;               // [count][EST_WIN]: vector2double of the updated state
    vio_est_result *res;
};

__global__ __launch_bounds__(EST_WAVE) void k_est_update(EstUpdateArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x;
    vio_est_state *S = a.t.state + a.slot[i];
    const double *w = a.win + (int64_t)EST_WIN * i;
    double *wo = a.wout + (int64_t)EST_WIN * i;
    // every lane: origin_R0 / origin_P0 and rot_diff (:551-577), from the state as the call found it
    const int occur = S->failure_occur;
    double Rs0[9], Ro[9], P0[3], lastP[3], rot_diff[9];
    for (int c = 0; c < 9; ++c) { Rs0[c] = S->Rs[0][c]; Ro[c] = occur ? S->last_R0[c] : Rs0[c]; }
    for (int c = 0; c < 3; ++c) { P0[c] = occur ? S->last_P0[c] : S->Ps[0][c]; lastP[c] = S->last_P[c]; }
    const int singular = est_rot_diff(Ro, Rs0, w + 3, rot_diff);
    __syncthreads();                                // (one wavefront: every lane has read before any lane writes)
    double R[9], P[3], V[3], Ba[3], Bg[3];
    int gate = 0;
    if (lane < EST_FRAMES) {                        // :579-600
        est_update_frame(rot_diff, P0, w + 7 * lane, w, w + EST_W_SB + 9 * lane, R, P, V, Ba, Bg);
        for (int c = 0; c < 9; ++c) S->Rs[lane][c] = R[c];
        for (int c = 0; c < 3; ++c) { S->Ps[lane][c] = P[c]; S->Vs[lane][c] = V[c]; S->Bas[lane][c] = Ba[c]; S->Bgs[lane][c] = Bg[c]; }
        if (lane == EST_WINDOW) gate = est_gate(Ba, Bg, P, lastP);
        double q[4];                                // vector2double of the frame just written: what the marginalisation takes
        est_rot_to_quat(R, q);
        for (int c = 0; c < 3; ++c) {
            wo[7 * lane + c] = P[c];
            wo[EST_W_SB + 9 * lane + c] = V[c]; wo[EST_W_SB + 9 * lane + 3 + c] = Ba[c]; wo[EST_W_SB + 9 * lane + 6 + c] = Bg[c];
        }
        for (int c = 0; c < 4; ++c) wo[7 * lane + 3 + c] = q[c];
    } else if (lane == EST_FRAMES) {                // :602-612
        double M[9], q[4];
        est_quat_to_rot(w + EST_W_EXT + 3, M);
        est_rot_to_quat(M, q);
        for (int c = 0; c < 3; ++c) { S->tic[c] = w[EST_W_EXT + c]; wo[EST_W_EXT + c] = w[EST_W_EXT + c]; }
        for (int c = 0; c < 9; ++c) S->ric[c] = M[c];
        for (int c = 0; c < 4; ++c) wo[EST_W_EXT + 3 + c] = q[c];
    }
    gate = __shfl(gate, EST_WINDOW);
    const int failure = gate != 0;
    const bool commit = !failure && a.commit[i] != 0;
    if (lane == 0) {
        S->failure_occur = failure;                 // double2vector clears it (:558); processImage sets it on a failure (:218)
        if (commit)
            for (int c = 0; c < 9; ++c) { S->last_R0[c] = R[c]; if (c < 3) S->last_P0[c] = P[c]; }
        vio_est_result *r = a.res + i;
        est_result_clear(r);
        r->frame_count = S->frame_count;
        r->failure = failure;
        r->gate = gate;
        r->singular = singular;
    }
    if (lane == EST_WINDOW && commit)
        for (int c = 0; c < 9; ++c) { S->last_R[c] = R[c]; if (c < 3) S->last_P[c] = P[c]; }
}

struct EstSlideArgs {
    EstTables t;
    const int32_t *slot;
    const int32_t *kind;
    const int32_t *nonlinear;
    vio_est_result *res;
};

__global__ __launch_bounds__(EST_NT) void k_est_slide(EstSlideArgs a) {
    const int t = threadIdx.x, i = blockIdx.x;
    const int slot = a.slot[i];
    vio_est_state *S = a.t.state + slot;
    int64_t *o = a.t.off + (int64_t)EST_OFFS * slot;
    double *first = a.t.first + 6 * (int64_t)EST_OFFS * slot;
    vio_est_result *r = a.res + i;
    const int fc = S->frame_count, kind = a.kind[i];
    int64_t off[EST_OFFS];
    for (int j = 0; j < EST_OFFS; ++j) off[j] = o[j];
    if (fc != EST_WINDOW) {                         // the reference's rule (:1152, :1206)
        if (t == 0) {
            est_result_clear(r);
            r->frame_count = fc;
            r->n_samples = (int)(off[EST_OFFS - 1] - off[0]);
        }
        return;
    }
    if (kind == VIO_EST_MARG_OLD) {
        // the samples of intervals 1 .. 10 move down over interval 0's: a chunk is read, then written, so a chunk never reads what
        // an earlier one wrote (the destination lies below the source)
        const int64_t src = off[1], dst = off[0], tail = off[EST_OFFS - 1] - off[1];
        if (src != dst)
            for (int64_t base = 0; base < tail; base += EST_NT) {
                const int64_t s = base + t;
                const bool on = s < tail;
                double v[7] = {0, 0, 0, 0, 0, 0, 0};
                if (on) {
                    v[0] = a.t.dt[src + s];
                    for (int c = 0; c < 3; ++c) { v[1 + c] = a.t.acc[3 * (src + s) + c]; v[4 + c] = a.t.gyr[3 * (src + s) + c]; }
                }
                __syncthreads();
                if (on) {
                    a.t.dt[dst + s] = v[0];
                    for (int c = 0; c < 3; ++c) { a.t.acc[3 * (dst + s) + c] = v[1 + c]; a.t.gyr[3 * (dst + s) + c] = v[4 + c]; }
                }
                __syncthreads();
            }
        // frame t < 10 takes frame t + 1; frame 10 stays (it is the copy of the new frame 9, :1170-1175).  Read, barrier, write.
        double R[9], P[3], V[3], Ba[3], Bg[3], H = 0, F[6], L[6], bR[9], bP[3];
        int ex = 0;
        if (t < EST_WINDOW) {
            for (int c = 0; c < 9; ++c) R[c] = S->Rs[t + 1][c];
            for (int c = 0; c < 3; ++c) { P[c] = S->Ps[t + 1][c]; V[c] = S->Vs[t + 1][c]; Ba[c] = S->Bas[t + 1][c]; Bg[c] = S->Bgs[t + 1][c]; }
            H = S->Headers[t + 1];
            ex = S->exists[t + 1];
            for (int c = 0; c < 6; ++c) { F[c] = first[6 * (t + 1) + c]; L[c] = S->lin_bias[t + 1][c]; }
        }
        if (t == 0) {                               // back_R0, back_P0 (:1150-1151)
            for (int c = 0; c < 9; ++c) bR[c] = S->Rs[0][c];
            for (int c = 0; c < 3; ++c) bP[c] = S->Ps[0][c];
        }
        __syncthreads();
        if (t < EST_WINDOW) {
            for (int c = 0; c < 9; ++c) S->Rs[t][c] = R[c];
            for (int c = 0; c < 3; ++c) { S->Ps[t][c] = P[c]; S->Vs[t][c] = V[c]; S->Bas[t][c] = Ba[c]; S->Bgs[t][c] = Bg[c]; }
            S->Headers[t] = H;
            S->exists[t] = ex;
            for (int c = 0; c < 6; ++c) { first[6 * t + c] = F[c]; S->lin_bias[t][c] = L[c]; }
        }
        if (t == EST_WINDOW) {                      // new IntegrationBase{acc_0, gyr_0, Bas[10], Bgs[10]} (:1177-1182)
            S->exists[EST_WINDOW] = 1;
            for (int c = 0; c < 3; ++c) {
                first[6 * EST_WINDOW + c] = S->acc_0[c]; first[6 * EST_WINDOW + 3 + c] = S->gyr_0[c];
                S->lin_bias[EST_WINDOW][c] = S->Bas[EST_WINDOW][c]; S->lin_bias[EST_WINDOW][3 + c] = S->Bgs[EST_WINDOW][c];
            }
            const int64_t d = off[1] - off[0];
            for (int j = 0; j + 1 < EST_OFFS; ++j) o[j] = off[j + 1] - d;
            o[EST_OFFS - 1] = off[EST_OFFS - 1] - d;
        }
        if (t == 0) {                               // slideWindowOld (:1254-1259): R = the new Rs[0], in this thread's registers
            double ric[9], tic[3];
            for (int c = 0; c < 9; ++c) ric[c] = S->ric[c];
            for (int c = 0; c < 3; ++c) tic[c] = S->tic[c];
            est_result_clear(r);
            est_slide_mats(bR, bP, R, P, ric, tic, r->marg_R, r->marg_P, r->new_R, r->new_P);
            r->frame_count = fc;
            r->n_samples = (int)(off[EST_OFFS - 1] - off[1]);
            r->slid = 1;
            r->shift_depth = a.nonlinear[i] != 0;
        }
        return;
    }
    if (t == 0) {                                   // MARG_SECOND_NEW (:1206-1236)
        o[EST_WINDOW] = off[EST_OFFS - 1];          // interval 9 takes interval 10's samples: they lie behind its own
        for (int c = 0; c < 9; ++c) S->Rs[EST_WINDOW - 1][c] = S->Rs[EST_WINDOW][c];
        for (int c = 0; c < 3; ++c) {
            S->Ps[EST_WINDOW - 1][c] = S->Ps[EST_WINDOW][c]; S->Vs[EST_WINDOW - 1][c] = S->Vs[EST_WINDOW][c];
            S->Bas[EST_WINDOW - 1][c] = S->Bas[EST_WINDOW][c]; S->Bgs[EST_WINDOW - 1][c] = S->Bgs[EST_WINDOW][c];
        }
        S->Headers[EST_WINDOW - 1] = S->Headers[EST_WINDOW];
        S->exists[EST_WINDOW] = 1;
        for (int c = 0; c < 3; ++c) {
            first[6 * EST_WINDOW + c] = S->acc_0[c]; first[6 * EST_WINDOW + 3 + c] = S->gyr_0[c];
            S->lin_bias[EST_WINDOW][c] = S->Bas[EST_WINDOW][c]; S->lin_bias[EST_WINDOW][3 + c] = S->Bgs[EST_WINDOW][c];
        }
        est_result_clear(r);
        r->frame_count = fc;
        r->n_samples = (int)(off[EST_OFFS - 1] - off[0]);
        r->slid = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
struct vio_est {
    int device = 0;
    StreamEvents<3> q;                              // the caller's stream or an owned one, and the timing events
    ErrText err = {0};
    vio_est_config cfg;
    DevBuf<char> data;                              // state | off | first | dt | acc | gyr
    EstTables t = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    Twin<char> in, out;
    double timing[4] = {0, 0, 0, 0};
};

namespace {

constexpr size_t kNS = VIO_EST_MAX_SLOTS, kSamples = (size_t)VIO_EST_MAX_SLOTS * VIO_EST_MAX_SAMPLES;

vio_est_config default_config() {
    vio_est_config c;
    std::memset(&c, 0, sizeof c);
    c.ric[3] = 1.0;
    c.g[2] = 9.81;
    c.noise[0] = 0.2687; c.noise[1] = 0.2121; c.noise[2] = 7.07e-6; c.noise[3] = 7.07e-7;
    return c;
}

// clearState + setParameter on a host image: what clearState leaves alone stays
void reset_image(vio_est_state &s, const vio_est_config &c) {
    s.frame_count = 0; s.first_imu = 0; s.failure_occur = 0; s.reserved = 0;
    std::memset(s.exists, 0, sizeof s.exists);
    std::memset(s.Ps, 0, sizeof s.Ps); std::memset(s.Vs, 0, sizeof s.Vs); std::memset(s.Bas, 0, sizeof s.Bas);
    std::memset(s.Bgs, 0, sizeof s.Bgs); std::memset(s.Rs, 0, sizeof s.Rs);
    std::memset(s.first, 0, sizeof s.first); std::memset(s.lin_bias, 0, sizeof s.lin_bias);
    for (int i = 0; i < EST_FRAMES; ++i) s.Rs[i][0] = s.Rs[i][4] = s.Rs[i][8] = 1.0;
    for (int k = 0; k < 3; ++k) { s.tic[k] = c.tic[k]; s.g[k] = c.g[k]; }
    est_quat_to_rot(c.ric, s.ric);
}

bool all_finite(const double *v, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// the checks every batched call shares: the count and the two arrays, then every item's slot
vio_status check_slots(vio_est *h, int32_t count, const void *items, const void *results, const char *what) {
    if (count < 0 || count > VIO_EST_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "%s: count %d outside [0, %d]", what, count, VIO_EST_MAX_SLOTS);
    if (count > 0 && (!items || !results)) return fail(h->err, VIO_ERR_BAD_ARG, "%s: items / results is NULL", what);
    return VIO_OK;
}

template <class Item> vio_status check_distinct(vio_est *h, int32_t count, const Item *items, const char *what) {
    bool seen[VIO_EST_MAX_SLOTS] = {false};
    for (int32_t i = 0; i < count; ++i) {
        const int32_t s = items[i].slot;
        if (s < 0 || s >= VIO_EST_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d outside [0, %d)", what, i, s, VIO_EST_MAX_SLOTS);
        if (seen[s]) return fail(h->err, VIO_ERR_BAD_ARG, "%s: item %d: slot %d is listed twice", what, i, s);
        seen[s] = true;
    }
    return VIO_OK;
}

struct CallClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// the tail every batched call shares: results of result_size bytes each (and `extra` bytes behind them) down, one wait, the timing
vio_status finish(vio_est *h, const CallClock &clk, double t_host, int32_t count, size_t nout, void *results, const char *what,
                  size_t result_size = sizeof(vio_est_result)) {
    vio_status st;
    hipEventRecord(h->q.ev[1], h->q.stream);
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->out.h, h->out.d, nout, hipMemcpyDeviceToHost, h->q.stream), "read-back")) != VIO_OK) return st;
    hipEventRecord(h->q.ev[2], h->q.stream);
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), what)) != VIO_OK) return st;
    std::memcpy(results, h->out.h, result_size * (size_t)count);
    h->timing[0] = t_host;
    h->timing[1] = elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[2] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    h->timing[3] = clk.ms();
    return VIO_OK;
}

}  // namespace

extern "C" {

void vio_est_destroy(vio_est *h) { destroy_handle(h); }

vio_status vio_est_create(int32_t device, void *stream, vio_est **out) {
    return create_handle(device, stream, out, vio_est_destroy, [](vio_est *h) {
        h->cfg = default_config();
        const size_t oState = 0, oOff = align256(oState + sizeof(vio_est_state) * kNS), oFirst = align256(oOff + 8 * EST_OFFS * kNS),
                     oDt = align256(oFirst + 48 * EST_OFFS * kNS), oAcc = align256(oDt + 8 * kSamples), oGyr = align256(oAcc + 24 * kSamples),
                     total = align256(oGyr + 24 * kSamples);
        if (h->data.ensure(h->err, total) != VIO_OK) return false;
        if (hipMemsetAsync(h->data.d, 0, total, h->q.stream) != hipSuccess) return false;
        h->t.state = (vio_est_state *)(h->data.d + oState);
        h->t.off = (int64_t *)(h->data.d + oOff);
        h->t.first = (double *)(h->data.d + oFirst);
        h->t.dt = (double *)(h->data.d + oDt);
        h->t.acc = (double *)(h->data.d + oAcc);
        h->t.gyr = (double *)(h->data.d + oGyr);
        std::vector<vio_est_state> img(kNS);
        std::vector<int64_t> off(EST_OFFS * kNS);
        for (size_t s = 0; s < kNS; ++s) {
            std::memset(&img[s], 0, sizeof(vio_est_state));
            reset_image(img[s], h->cfg);
            for (int j = 0; j < EST_OFFS; ++j) off[EST_OFFS * s + j] = (int64_t)s * VIO_EST_MAX_SAMPLES;
        }
        if (hipMemcpyAsync(h->t.state, img.data(), sizeof(vio_est_state) * kNS, hipMemcpyHostToDevice, h->q.stream) != hipSuccess) return false;
        if (hipMemcpyAsync(h->t.off, off.data(), 8 * off.size(), hipMemcpyHostToDevice, h->q.stream) != hipSuccess) return false;
        return hipStreamSynchronize(h->q.stream) == hipSuccess;
    });
}

const char *vio_est_last_error(const vio_est *h) { return h ? h->err : "NULL handle"; }

int32_t vio_est_version(void) { return VIO_EST_VERSION; }

vio_status vio_est_set_config(vio_est *h, const vio_est_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg) return fail(h->err, VIO_ERR_BAD_ARG, "cfg is NULL");
    if (!all_finite(cfg->tic, 3) || !all_finite(cfg->ric, 4) || !all_finite(cfg->g, 3) || !all_finite(cfg->noise, 4))
        return fail(h->err, VIO_ERR_BAD_ARG, "a non-finite entry in the config");
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_est_reset(vio_est *h, int32_t slot) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_EST_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "slot %d outside [0, %d)", slot, VIO_EST_MAX_SLOTS);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    vio_est_state s;
    if ((st = hip_ck(h->err, hipMemcpyAsync(&s, h->t.state + slot, sizeof s, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;
    reset_image(s, h->cfg);
    int64_t off[EST_OFFS];
    for (int j = 0; j < EST_OFFS; ++j) off[j] = (int64_t)slot * VIO_EST_MAX_SAMPLES;
    double first[6 * EST_OFFS] = {0};
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->t.state + slot, &s, sizeof s, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->t.off + EST_OFFS * slot, off, sizeof off, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->t.first + 6 * EST_OFFS * slot, first, sizeof first, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    return hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize");
}

vio_status vio_est_state_set(vio_est *h, int32_t slot, const vio_est_state *state, const int64_t *off, const double *dt, const double *acc,
                             const double *gyr) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_EST_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "slot %d outside [0, %d)", slot, VIO_EST_MAX_SLOTS);
    if (!state || !off) return fail(h->err, VIO_ERR_BAD_ARG, "state / off is NULL");
    const vio_est_state &s = *state;
    if (s.frame_count < 0 || s.frame_count > EST_WINDOW) return fail(h->err, VIO_ERR_BAD_ARG, "frame_count %d outside [0, 10]", s.frame_count);
    if ((s.first_imu | 1) != 1 || (s.failure_occur | 1) != 1) return fail(h->err, VIO_ERR_BAD_ARG, "first_imu / failure_occur is neither 0 nor 1");
    for (int j = 0; j < EST_OFFS; ++j)
        if ((s.exists[j] | 1) != 1 || (j == EST_OFFS - 1 && s.exists[j])) return fail(h->err, VIO_ERR_BAD_ARG, "exists[%d] = %d", j, s.exists[j]);
    if (off[0] != 0) return fail(h->err, VIO_ERR_BAD_ARG, "off[0] = %lld, not 0", (long long)off[0]);
    for (int j = 0; j < EST_FRAMES; ++j) {
        const int64_t n = off[j + 1] - off[j];
        if (n < 0) return fail(h->err, VIO_ERR_BAD_ARG, "off decreases at interval %d", j);
        if (n > 0 && (j > s.frame_count || !s.exists[j]))
            return fail(h->err, VIO_ERR_BAD_ARG, "interval %d holds %lld samples but %s", j, (long long)n, j > s.frame_count ? "lies behind frame_count" : "does not exist");
    }
    const int64_t S = off[EST_OFFS - 1];
    if (S > VIO_EST_MAX_SAMPLES) return fail(h->err, VIO_ERR_BAD_ARG, "%lld samples, more than %d", (long long)S, VIO_EST_MAX_SAMPLES);
    if (S > 0 && (!dt || !acc || !gyr)) return fail(h->err, VIO_ERR_BAD_ARG, "%lld samples and dt / acc / gyr is NULL", (long long)S);
    if (!all_finite(&s.Ps[0][0], 419)) return fail(h->err, VIO_ERR_BAD_ARG, "a non-finite entry in the state");
    if (S > 0 && (!all_finite(dt, (size_t)S) || !all_finite(acc, 3 * (size_t)S) || !all_finite(gyr, 3 * (size_t)S)))
        return fail(h->err, VIO_ERR_BAD_ARG, "a non-finite sample");
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const int64_t base = (int64_t)slot * VIO_EST_MAX_SAMPLES;
    int64_t aoff[EST_OFFS];
    for (int j = 0; j < EST_OFFS; ++j) aoff[j] = base + off[j];
    double first[6 * EST_OFFS] = {0};
    std::memcpy(first, s.first, sizeof s.first);
    struct { void *d; const void *s; size_t b; } cp[6] = {{h->t.state + slot, state, sizeof(vio_est_state)}, {h->t.off + EST_OFFS * slot, aoff, sizeof aoff},
                                                          {h->t.first + 6 * EST_OFFS * slot, first, sizeof first}, {h->t.dt + base, dt, 8 * (size_t)S},
                                                          {h->t.acc + 3 * base, acc, 24 * (size_t)S}, {h->t.gyr + 3 * base, gyr, 24 * (size_t)S}};
    vio_status st;
    for (auto &c : cp)
        if (c.b && (st = hip_ck(h->err, hipMemcpyAsync(c.d, c.s, c.b, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) {
            (void)hipStreamSynchronize(h->q.stream);
            return st;
        }
    return hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize");
}

vio_status vio_est_state_get(vio_est *h, int32_t slot, vio_est_state *state, int64_t cap_samples, int64_t *off, double *dt, double *acc,
                             double *gyr) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (slot < 0 || slot >= VIO_EST_MAX_SLOTS) return fail(h->err, VIO_ERR_BAD_ARG, "slot %d outside [0, %d)", slot, VIO_EST_MAX_SLOTS);
    if (!state || !off || cap_samples < 0) return fail(h->err, VIO_ERR_BAD_ARG, "state / off is NULL, or cap_samples < 0");
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    vio_status st;
    int64_t aoff[EST_OFFS];
    double first[6 * EST_OFFS];
    vio_est_state s;
    if ((st = hip_ck(h->err, hipMemcpyAsync(&s, h->t.state + slot, sizeof s, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK ||
        (st = hip_ck(h->err, hipMemcpyAsync(aoff, h->t.off + EST_OFFS * slot, sizeof aoff, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK ||
        (st = hip_ck(h->err, hipMemcpyAsync(first, h->t.first + 6 * EST_OFFS * slot, sizeof first, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK) {
        (void)hipStreamSynchronize(h->q.stream);
        return st;
    }
    if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;
    const int64_t base = (int64_t)slot * VIO_EST_MAX_SAMPLES;
    for (int j = 0; j < EST_OFFS; ++j) off[j] = aoff[j] - base;
    const int64_t S = off[EST_OFFS - 1];
    if (S > cap_samples) return fail(h->err, VIO_ERR_BAD_ARG, "the slot holds %lld samples, cap_samples is %lld", (long long)S, (long long)cap_samples);
    if (S > 0 && (!dt || !acc || !gyr)) return fail(h->err, VIO_ERR_BAD_ARG, "%lld samples and dt / acc / gyr is NULL", (long long)S);
    std::memcpy(s.first, first, sizeof s.first);
    *state = s;
    if (S > 0) {
        if ((st = hip_ck(h->err, hipMemcpyAsync(dt, h->t.dt + base, 8 * (size_t)S, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK ||
            (st = hip_ck(h->err, hipMemcpyAsync(acc, h->t.acc + 3 * base, 24 * (size_t)S, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK ||
            (st = hip_ck(h->err, hipMemcpyAsync(gyr, h->t.gyr + 3 * base, 24 * (size_t)S, hipMemcpyDeviceToHost, h->q.stream), "download")) != VIO_OK) {
            (void)hipStreamSynchronize(h->q.stream);
            return st;
        }
        if ((st = hip_ck(h->err, hipStreamSynchronize(h->q.stream), "hipStreamSynchronize")) != VIO_OK) return st;
    }
    return VIO_OK;
}

vio_status vio_est_imu_batch(vio_est *h, int32_t count, const vio_est_imu_item *items, vio_est_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "imu_batch")) != VIO_OK || (st = check_distinct(h, count, items, "imu_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    size_t S = 0;
    for (int32_t i = 0; i < count; ++i) {
        const vio_est_imu_item &it = items[i];
        if (it.n < 0 || it.n > VIO_EST_MAX_SAMPLES) return fail(h->err, VIO_ERR_BAD_ARG, "imu_batch: item %d: n = %d outside [0, %d]", i, it.n, VIO_EST_MAX_SAMPLES);
        if (it.n > 0 && (!it.dt || !it.acc || !it.gyr)) return fail(h->err, VIO_ERR_BAD_ARG, "imu_batch: item %d: dt / acc / gyr is NULL", i);
        if (!all_finite(it.dt, (size_t)it.n) || !all_finite(it.acc, 3 * (size_t)it.n) || !all_finite(it.gyr, 3 * (size_t)it.n))
            return fail(h->err, VIO_ERR_BAD_ARG, "imu_batch: item %d: a non-finite sample", i);
        S += (size_t)it.n;
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t oSlot = 0, oOff = align256(oSlot + 4 * (size_t)count), oDt = align256(oOff + 8 * ((size_t)count + 1)), oAcc = align256(oDt + 8 * S),
                 oGyr = align256(oAcc + 24 * S), nin = align256(oGyr + 24 * S), nout = sizeof(vio_est_result) * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    int32_t *hs = (int32_t *)(h->in.h + oSlot);
    int64_t *ho = (int64_t *)(h->in.h + oOff);
    double *hdt = (double *)(h->in.h + oDt), *hacc = (double *)(h->in.h + oAcc), *hgyr = (double *)(h->in.h + oGyr);
    ho[0] = 0;
    for (int32_t i = 0; i < count; ++i) {
        const vio_est_imu_item &it = items[i];
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
    EstImuArgs a;
    a.t = h->t;
    a.slot = (const int32_t *)(h->in.d + oSlot); a.in_off = (const int64_t *)(h->in.d + oOff);
    a.in_dt = (const double *)(h->in.d + oDt); a.in_acc = (const double *)(h->in.d + oAcc); a.in_gyr = (const double *)(h->in.d + oGyr);
    a.res = (vio_est_result *)h->out.d;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_est_imu, dim3(count), dim3(EST_WAVE), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_est_imu launch");
    return finish(h, clk, t_host, count, nout, results, "k_est_imu");
}

vio_status vio_est_image_batch(vio_est *h, int32_t count, const vio_est_image_item *items, vio_est_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "image_batch")) != VIO_OK || (st = check_distinct(h, count, items, "image_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    for (int32_t i = 0; i < count; ++i)
        if (!std::isfinite(items[i].header)) return fail(h->err, VIO_ERR_BAD_ARG, "image_batch: item %d: a non-finite header", i);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t oSlot = 0, oAdv = align256(oSlot + 4 * (size_t)count), oHdr = align256(oAdv + 4 * (size_t)count), nin = align256(oHdr + 8 * (size_t)count),
                 nout = sizeof(vio_est_result) * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i) {
        ((int32_t *)(h->in.h + oSlot))[i] = items[i].slot;
        ((int32_t *)(h->in.h + oAdv))[i] = items[i].advance != 0;
        ((double *)(h->in.h + oHdr))[i] = items[i].header;
    }
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    EstImageArgs a;
    a.t = h->t;
    a.slot = (const int32_t *)(h->in.d + oSlot); a.advance = (const int32_t *)(h->in.d + oAdv); a.header = (const double *)(h->in.d + oHdr);
    a.res = (vio_est_result *)h->out.d;
    a.count = count;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_est_image, dim3((count + EST_WAVE - 1) / EST_WAVE), dim3(EST_WAVE), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_est_image launch");
    return finish(h, clk, t_host, count, nout, results, "k_est_image");
}

vio_status vio_est_window_batch(vio_est *h, int32_t count, const vio_est_window_item *items, vio_est_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "window_batch")) != VIO_OK || (st = check_distinct(h, count, items, "window_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    for (int32_t i = 0; i < count; ++i)
        if (!items[i].poses || !items[i].speed_bias || !items[i].ext || !items[i].preint)
            return fail(h->err, VIO_ERR_BAD_ARG, "window_batch: item %d: poses / speed_bias / ext / preint is NULL", i);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t nrec = (size_t)EST_WINDOW * count;
    const size_t oSlot = 0, oBias = align256(oSlot + 4 * (size_t)count), oWhich = align256(oBias + 48 * nrec), nin = align256(oWhich + 4 * nrec);
    const size_t oRes = 0, oWin = align256(oRes + sizeof(vio_est_result) * (size_t)count), oRec = align256(oWin + 8 * EST_WIN * (size_t)count),
                 nout = oRec + 8 * IMU_REC * nrec;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i) ((int32_t *)(h->in.h + oSlot))[i] = items[i].slot;
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, 4 * (size_t)count, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    EstExportArgs e;
    e.t = h->t;
    e.slot = (const int32_t *)(h->in.d + oSlot);
    e.win = (double *)(h->out.d + oWin);
    e.bias = (double *)(h->in.d + oBias);
    e.which = (int *)(h->in.d + oWhich);
    e.res = (vio_est_result *)(h->out.d + oRes);
    ImuArgs a;
    a.off = h->t.off; a.first = h->t.first; a.dt = h->t.dt; a.acc = h->t.acc; a.gyr = h->t.gyr;
    a.bias = e.bias; a.which = e.which;
    a.out = (double *)(h->out.d + oRec);
    for (int c = 0; c < 4; ++c) a.sn[c] = h->cfg.noise[c];
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_est_export, dim3(count), dim3(EST_WAVE), 0, h->q.stream, e);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_est_export launch");
    hipLaunchKernelGGL(k_imu_propagate, dim3((unsigned)nrec), dim3(IMU_NT), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_imu_propagate launch");
    if ((st = finish(h, clk, t_host, count, nout, results, "k_est_export, k_imu_propagate")) != VIO_OK) return st;
    const double *win = (const double *)(h->out.h + oWin), *rec = (const double *)(h->out.h + oRec);
    for (int32_t i = 0; i < count; ++i) {
        const double *w = win + (size_t)EST_WIN * i;
        std::memcpy(items[i].poses, w, 8 * 77);
        std::memcpy(items[i].speed_bias, w + EST_W_SB, 8 * 99);
        std::memcpy(items[i].ext, w + EST_W_EXT, 8 * 7);
        std::memcpy(items[i].preint, rec + (size_t)IMU_REC * EST_WINDOW * i, sizeof(vio_preint) * EST_WINDOW);
    }
    h->timing[3] = clk.ms();
    return VIO_OK;
}

vio_status vio_est_update_batch(vio_est *h, int32_t count, const vio_est_update_item *items, vio_est_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "update_batch")) != VIO_OK || (st = check_distinct(h, count, items, "update_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    for (int32_t i = 0; i < count; ++i) {
        if (!items[i].poses || !items[i].speed_bias || !items[i].ext) return fail(h->err, VIO_ERR_BAD_ARG, "update_batch: item %d: poses / speed_bias / ext is NULL", i);
        if (!all_finite(items[i].poses, 77) || !all_finite(items[i].speed_bias, 99) || !all_finite(items[i].ext, 7))
            return fail(h->err, VIO_ERR_BAD_ARG, "update_batch: item %d: a non-finite pose, speed-bias or extrinsic", i);
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t oSlot = 0, oCommit = align256(oSlot + 4 * (size_t)count), oWin = align256(oCommit + 4 * (size_t)count),
                 nin = align256(oWin + 8 * EST_WIN * (size_t)count), oOut = align256(sizeof(vio_est_result) * (size_t)count),
                 nout = oOut + 8 * EST_WIN * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i) {
        ((int32_t *)(h->in.h + oSlot))[i] = items[i].slot;
        ((int32_t *)(h->in.h + oCommit))[i] = items[i].commit_last != 0;
        double *w = (double *)(h->in.h + oWin) + (size_t)EST_WIN * i;
        std::memcpy(w, items[i].poses, 8 * 77);
        std::memcpy(w + EST_W_SB, items[i].speed_bias, 8 * 99);
        std::memcpy(w + EST_W_EXT, items[i].ext, 8 * 7);
    }
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    EstUpdateArgs a;
    a.t = h->t;
    a.slot = (const int32_t *)(h->in.d + oSlot); a.commit = (const int32_t *)(h->in.d + oCommit); a.win = (const double *)(h->in.d + oWin);
    a.res = (vio_est_result *)h->out.d;
    a.wout = (double *)(h->out.d + oOut);
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_est_update, dim3(count), dim3(EST_WAVE), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_est_update launch");
    if ((st = finish(h, clk, t_host, count, nout, results, "k_est_update")) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i) {
        const double *w = (const double *)(h->out.h + oOut) + (size_t)EST_WIN * i;
        if (items[i].poses_out) std::memcpy(items[i].poses_out, w, 8 * 77);
        if (items[i].speed_bias_out) std::memcpy(items[i].speed_bias_out, w + EST_W_SB, 8 * 99);
        if (items[i].ext_out) std::memcpy(items[i].ext_out, w + EST_W_EXT, 8 * 7);
    }
    h->timing[3] = clk.ms();
    return VIO_OK;
}

vio_status vio_est_slide_batch(vio_est *h, int32_t count, const vio_est_slide_item *items, vio_est_result *results) {
    CallClock clk;
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    vio_status st;
    if ((st = check_slots(h, count, items, results, "slide_batch")) != VIO_OK || (st = check_distinct(h, count, items, "slide_batch")) != VIO_OK) return st;
    if (count == 0) return VIO_OK;
    for (int32_t i = 0; i < count; ++i)
        if (items[i].kind != VIO_EST_MARG_OLD && items[i].kind != VIO_EST_MARG_SECOND_NEW)
            return fail(h->err, VIO_ERR_BAD_ARG, "slide_batch: item %d: kind %d", i, items[i].kind);
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t oSlot = 0, oKind = align256(oSlot + 4 * (size_t)count), oNl = align256(oKind + 4 * (size_t)count), nin = align256(oNl + 4 * (size_t)count),
                 nout = sizeof(vio_est_result) * (size_t)count;
    if ((st = h->in.ensure(h->err, nin)) != VIO_OK || (st = h->out.ensure(h->err, nout)) != VIO_OK) return st;
    for (int32_t i = 0; i < count; ++i) {
        ((int32_t *)(h->in.h + oSlot))[i] = items[i].slot;
        ((int32_t *)(h->in.h + oKind))[i] = items[i].kind;
        ((int32_t *)(h->in.h + oNl))[i] = items[i].nonlinear != 0;
    }
    if ((st = hip_ck(h->err, hipMemcpyAsync(h->in.d, h->in.h, nin, hipMemcpyHostToDevice, h->q.stream), "upload")) != VIO_OK) return st;
    const double t_host = clk.ms();
    EstSlideArgs a;
    a.t = h->t;
    a.slot = (const int32_t *)(h->in.d + oSlot); a.kind = (const int32_t *)(h->in.d + oKind); a.nonlinear = (const int32_t *)(h->in.d + oNl);
    a.res = (vio_est_result *)h->out.d;
    hipEventRecord(h->q.ev[0], h->q.stream);
    hipLaunchKernelGGL(k_est_slide, dim3(count), dim3(EST_NT), 0, h->q.stream, a);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "k_est_slide launch");
    return finish(h, clk, t_host, count, nout, results, "k_est_slide");
}

vio_status vio_est_timing(const vio_est *h, double *out4) {
    if (!h || !out4) return VIO_ERR_BAD_ARG;
    std::memcpy(out4, h->timing, sizeof(h->timing));
    return VIO_OK;
}

}   // extern "C"

#include "vio_est_init_body.inc"                    // include/vio_est_init.h: vio_est_init_apply_batch, vio_est_relinearize_batch
