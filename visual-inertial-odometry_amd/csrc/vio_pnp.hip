// vio_pnp.hip — libvio_pnp_hip.so: the PnP of the non-keyframes of many windows in one call (include/vio_pnp.h).
//
//   k_pnp_frames    one wavefront per frame, WAVES wavefronts per workgroup; the frames of every window of the call are one flat
//                   grid through the host-made descriptor table.  The wavefront lists the frame's usable points by a prefix count
//                   (64 observations at a time: a ballot of the valid ones, the set bits below each lane) into its own part of the
//                   HBM scratch, five doubles per point.  Then the Levenberg-Marquardt loop: lane j takes the usable points j,
//                   j + 64, ... in ascending order into 28 private accumulators (upper triangle of J^T J, J^T r, r^2), the butterfly
//                   v[i] += v[i ^ s], s = 1 .. 32, leaves the same 28 sums in every lane, and every lane runs the 6 x 6 damped
//                   Cholesky solve and the trust-region decision on them.
// Frames of one workgroup end after different iteration counts, so the kernel has no workgroup barrier anywhere: only wave-level
// operations (ballot, shuffle) and one workgroup-scope memory fence between the wavefront's writes of its point list and its reads.
// Every lane of a wavefront holds the same loop state, so the trip counts are uniform within the wavefront.
// Contraction is off: products and sums round as the host restatement's (tests/pnp_reference.py) do.  No floating-point atomics, so
// repeated calls are bitwise identical and a frame's result depends on nothing but its own inputs.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vio_pnp.h"
#include "vio_companion.h"

#pragma clang fp contract(off)

#include "vio_sfm_math.h"

#include "vio_pnp_body.inc"

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct vio_pnp {
    int device = 0;
    ErrText err = {0};
    vio_pnp_config cfg = {VIO_PNP_DEFAULT_MIN_POINTS, 0};
    Twin<char> staging;                                  // window descriptors | frame descriptors | int32 | doubles
    DevBuf<double> scr;
    Twin<double> out;
    StreamEvents<3> q;                                   // events: upload start, kernel start, end
    double timing[3] = {NAN, NAN, NAN};
};

namespace {

vio_status check_item(vio_pnp *h, int i, const vio_pnp_item &it) {
    if (it.n_frames < 0 || it.n_frames > VIO_PNP_MAX_FRAMES)
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: n_frames must be in [0, %d]", i, VIO_PNP_MAX_FRAMES);
    if (it.n_points < 0 || it.n_key < 0) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: n_points and n_key must not be negative", i);
    if (it.n_frames == 0) return VIO_OK;
    if (!it.guess_key || !it.obs_offset || !it.key_Q || !it.key_T)
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: key_Q, key_T, guess_key and obs_offset are required", i);
    if (it.obs_offset[0] != 0) return fail(h->err, VIO_ERR_BAD_ARG, "window %d: obs_offset[0] must be 0", i);
    for (int k = 0; k < it.n_frames; ++k) {
        if (it.guess_key[k] < 0 || it.guess_key[k] >= it.n_key)
            return fail(h->err, VIO_ERR_BAD_ARG, "window %d: guess_key[%d] is outside [0, n_key)", i, k);
        const int64_t len = it.obs_offset[k + 1] - it.obs_offset[k];
        if (len < 0 || len > VIO_PNP_MAX_POINTS)
            return fail(h->err, VIO_ERR_BAD_ARG, "window %d: frame %d must have between 0 and %d observations", i, k, VIO_PNP_MAX_POINTS);
    }
    const int64_t nobs = it.obs_offset[it.n_frames];
    if ((it.n_points > 0 && !it.points) || (nobs > 0 && (!it.obs_point || !it.obs_pts)))
        return fail(h->err, VIO_ERR_BAD_ARG, "window %d: points, obs_point and obs_pts are required", i);
    for (int64_t k = 0; k < nobs; ++k)
        if (it.obs_point[k] < 0 || it.obs_point[k] >= it.n_points)
            return fail(h->err, VIO_ERR_BAD_ARG, "window %d: obs_point[%lld] is outside [0, n_points)", i, (long long)k);
    return VIO_OK;
}

}  // namespace

extern "C" {

int32_t vio_pnp_version(void) { return VIO_PNP_VERSION; }

const char *vio_pnp_last_error(const vio_pnp *h) { return h ? h->err : "NULL handle"; }

vio_status vio_pnp_create(int32_t device, void *stream, vio_pnp **out) { return create_handle(device, stream, out, vio_pnp_destroy); }

void vio_pnp_destroy(vio_pnp *h) { destroy_handle(h); }

vio_status vio_pnp_set_config(vio_pnp *h, const vio_pnp_config *cfg) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (!cfg || cfg->min_points < 3 || cfg->min_points > VIO_PNP_MAX_POINTS)
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_pnp_set_config: min_points must be in [3, %d]", VIO_PNP_MAX_POINTS);
    h->cfg = *cfg;
    return VIO_OK;
}

vio_status vio_pnp_timing(const vio_pnp *h, double *out3) {
    if (!h || !out3) return VIO_ERR_BAD_ARG;
    std::memcpy(out3, h->timing, sizeof(h->timing));
    return VIO_OK;
}

vio_status vio_pnp_frames_batch(vio_pnp *h, int32_t count, const vio_pnp_item *items, vio_pnp_result *res, double *Q, double *T,
                                vio_pnp_frame_info *frame_info) {
    if (!h) return VIO_ERR_BAD_ARG;
    h->err[0] = 0;
    if (count < 0 || (count > 0 && (!items || !res || !Q || !T)))
        return fail(h->err, VIO_ERR_BAD_ARG, "vio_pnp_frames_batch: negative count or a NULL array");
    if (count == 0) return VIO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < count; ++i) {
        const vio_status st = check_item(h, i, items[i]);
        if (st != VIO_OK) return st;
    }
    // the descriptor table: every frame of every window, in the items' order
    int64_t ni = 0, nd = 0, nscr = 0;
    std::vector<PnpWin> wins((size_t)count);
    std::vector<PnpFrame> frames;
    for (int i = 0; i < count; ++i) {
        const vio_pnp_item &it = items[i];
        PnpWin &w = wins[(size_t)i];
        std::memset(&w, 0, sizeof(w));
        if (it.n_frames == 0) continue;                 // (nothing of it is staged)
        w.np = it.n_points;
        w.has_valid = it.valid != nullptr;
        w.o_valid = ni; ni += w.has_valid ? it.n_points : 0;
        w.o_pts = nd; nd += 3 * (int64_t)it.n_points;
        w.o_key = nd; nd += 4 * (int64_t)it.n_key;
        w.o_keyT = nd; nd += 3 * (int64_t)it.n_key;
        for (int k = 0; k < it.n_frames; ++k) {
            PnpFrame fr;
            std::memset(&fr, 0, sizeof(fr));
            fr.win = i; fr.guess = it.guess_key[k];
            fr.nobs = (int32_t)(it.obs_offset[k + 1] - it.obs_offset[k]);
            fr.o_op = ni; ni += fr.nobs;
            fr.o_obs = nd; nd += 2 * (int64_t)fr.nobs;
            fr.o_scr = nscr; nscr += PD * (int64_t)fr.nobs;
            frames.push_back(fr);
        }
    }
    const size_t nf = frames.size();
    if (nf == 0) {
        for (int i = 0; i < count; ++i) { res[i].status = VIO_OK; res[i].fail_frame = -1; }
        return VIO_OK;
    }
    DeviceScope dev(h->device);
    if (!dev.ok) return fail(h->err, VIO_ERR_HIP, "hipSetDevice(%d)", h->device);
    const size_t b_win = align256(sizeof(PnpWin) * (size_t)count), b_fr = align256(sizeof(PnpFrame) * nf);
    const size_t b_int = align256(sizeof(int32_t) * (size_t)ni), bytes = b_win + b_fr + b_int + sizeof(double) * (size_t)nd;
    const size_t outb = sizeof(double) * FO * nf;
    vio_status st;
    if ((st = h->staging.ensure(h->err, bytes)) != VIO_OK || (st = h->out.ensure(h->err, outb)) != VIO_OK ||
        (st = h->scr.ensure(h->err, sizeof(double) * (size_t)(nscr + 1))) != VIO_OK)
        return st;
    std::memcpy(h->staging.h, wins.data(), sizeof(PnpWin) * (size_t)count);
    std::memcpy(h->staging.h + b_win, frames.data(), sizeof(PnpFrame) * nf);
    int32_t *hi = (int32_t *)(h->staging.h + b_win + b_fr);
    double *hd = (double *)(h->staging.h + b_win + b_fr + b_int);
    size_t row = 0;
    for (int i = 0; i < count; ++i) {
        const vio_pnp_item &it = items[i];
        const PnpWin &w = wins[(size_t)i];
        if (it.n_frames == 0) continue;
        if (w.has_valid)
            for (int j = 0; j < it.n_points; ++j) hi[w.o_valid + j] = it.valid[j] != 0;
        if (it.n_points) std::memcpy(hd + w.o_pts, it.points, sizeof(double) * 3 * (size_t)it.n_points);
        std::memcpy(hd + w.o_key, it.key_Q, sizeof(double) * 4 * (size_t)it.n_key);
        std::memcpy(hd + w.o_keyT, it.key_T, sizeof(double) * 3 * (size_t)it.n_key);
        for (int k = 0; k < it.n_frames; ++k) {
            const PnpFrame &fr = frames[row + (size_t)k];
            if (!fr.nobs) continue;
            std::memcpy(hi + fr.o_op, it.obs_point + it.obs_offset[k], sizeof(int32_t) * (size_t)fr.nobs);
            std::memcpy(hd + fr.o_obs, it.obs_pts + 2 * it.obs_offset[k], sizeof(double) * 2 * (size_t)fr.nobs);
        }
        row += (size_t)it.n_frames;
    }
    PnpArgs a;
    a.wins = (const PnpWin *)h->staging.d;
    a.frames = (const PnpFrame *)(h->staging.d + b_win);
    a.ints = (const int32_t *)(h->staging.d + b_win + b_fr);
    a.dd = (const double *)(h->staging.d + b_win + b_fr + b_int);
    a.scr = h->scr.d; a.out = h->out.d;
    a.nframes = (int32_t)nf; a.min_points = h->cfg.min_points;
    const auto t1 = std::chrono::steady_clock::now();
    hipStream_t q = h->q.stream;
    (void)hipEventRecord(h->q.ev[0], q);
    if (hipMemcpyAsync(h->staging.d, h->staging.h, bytes, hipMemcpyHostToDevice, q) != hipSuccess) return fail_synced(h, "upload failed");
    (void)hipEventRecord(h->q.ev[1], q);
    hipLaunchKernelGGL(k_pnp_frames, dim3((unsigned)((nf + WAVES - 1) / WAVES)), dim3(NT), 0, q, a);
    (void)hipEventRecord(h->q.ev[2], q);
    if (hipGetLastError() != hipSuccess) return fail_synced(h, "kernel launch failed");
    if (hipMemcpyAsync(h->out.h, h->out.d, outb, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        return fail_synced(h, "kernel or read-back failed");
    vio_status ret = VIO_OK;
    row = 0;
    for (int i = 0; i < count; ++i) {
        const int wf = items[i].n_frames;
        vio_pnp_result &r = res[i];
        r.status = VIO_OK; r.fail_frame = -1;
        bool bad = false;
        for (int k = 0; k < wf; ++k) {
            const int32_t fs = (int32_t)h->out.h[(size_t)FO * (row + k)];
            bad = bad || fs == VIO_ERR_NOT_FINITE;
            if (fs != VIO_OK && r.fail_frame < 0) { r.status = fs; r.fail_frame = k; }
        }
        if (bad) { r.status = VIO_ERR_NOT_FINITE; r.fail_frame = -1; }
        for (int k = 0; k < wf; ++k) {
            const double *o = h->out.h + (size_t)FO * (row + k);
            for (int c = 0; c < 4; ++c) Q[4 * (row + k) + c] = bad ? NAN : o[4 + c];
            for (int c = 0; c < 3; ++c) T[3 * (row + k) + c] = bad ? NAN : o[8 + c];
            if (!frame_info) continue;
            vio_pnp_frame_info &fi = frame_info[row + k];
            fi.status = bad ? VIO_ERR_NOT_FINITE : (int32_t)o[0];
            fi.iterations = bad ? 0 : (int32_t)o[1];
            fi.n_used = bad ? 0 : (int32_t)o[2];
            fi.reserved = 0;
            fi.cost = bad ? NAN : o[3];
        }
        if (bad) {
            if (ret == VIO_OK) fail(h->err, VIO_ERR_NOT_FINITE, "window %d: non-finite input or result", i);
            ret = VIO_ERR_NOT_FINITE;
        }
        row += (size_t)wf;
    }
    const auto t2 = std::chrono::steady_clock::now();
    h->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count() + elapsed_ms(h->q.ev[0], h->q.ev[1]);
    h->timing[1] = elapsed_ms(h->q.ev[1], h->q.ev[2]);
    h->timing[2] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return ret;
}

}  // extern "C"
