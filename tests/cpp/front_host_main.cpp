// front_host_main.cpp — tests/test_front_host_cpu.py's driver: the host sides of the four front-end stages
// (csrc/vio_{clahe,flow,detect,reject}_host.h), built by a plain C++ compiler with no HIP header, each inside the namespace
// libvio_frame_hip gives it.  It reads one command per line and answers with one line; a text follows a '|'.
//
//   CC fn clip tiles_x tiles_y                     clahe_check_config     -> status | text
//   CF fn levels half_patch max_iter inverse border early_stop   flow_check_config
//   CD fn quality min_distance                     det_check_config
//   CR fn hypotheses f_threshold focal_length      rej_check_config
//   CM fn model fx fy cx cy k1 k2 p1 p2 w h        rej_check_camera
//   DF                                             the four checks on the four defaults -> four statuses
//   N fn n_tracked max_total                       det_check_counts of item 7
//   T fn n x y ...                                 det_check_tracked of item 7 on a 3 x 2 image -> status active | text
//   S count n_trk n_new                            det_sizes -> b_it b_tab b_res b_keep b_out b_key b_scratch
//   L width height levels                          flow_level_dims, flow_item -> ok then w h pitch per level, then frame_layout's w h
//   U n_tracked max_total active dev_kept dev_new  det_unpack of one item between guard bytes -> status item_status n_kept n_new guards
//                                                  | keep_order ...
// fn: a function name, or - for none (the stand-alone libraries' item texts).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/vio_clahe.h"
#include "../../include/vio_detect.h"
#include "../../include/vio_flow.h"
#include "../../include/vio_reject.h"
#include "vio_host_base.h"
#include "vio_clahe_math.h"
#include "vio_detect_math.h"
#include "vio_frame_slots.h"
#include "vio_reject_math.h"

namespace kc {
#include "vio_clahe_host.h"
}
namespace kf {
#include "vio_flow_host.h"
}
namespace kd {
#include "vio_detect_host.h"
}
namespace kr {
#include "vio_reject_host.h"
}

static const char *name(vio_status st) {
    static char other[32];
    if (st == VIO_OK) return "OK";
    if (st == VIO_ERR_BAD_ARG) return "BAD_ARG";
    if (st == VIO_ERR_NOT_FINITE) return "NOT_FINITE";
    snprintf(other, sizeof(other), "%d", (int)st);
    return other;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    char line[4096];
    while (fgets(line, sizeof(line), in)) {
        std::istringstream ss(line);
        std::string cmd, fn;
        ss >> cmd;
        ErrText err = {0};
        const auto num = [&]() { std::string t; ss >> t; return strtod(t.c_str(), nullptr); };
        const auto prefix = [&]() { ss >> fn; if (fn == "-") fn = ""; };
        const auto item_prefix = [&]() { prefix(); if (!fn.empty()) fn += ": "; };
        if (cmd == "CC") {
            prefix();
            vio_clahe_config c;
            c.clip_limit = num(); c.tiles_x = (int32_t)num(); c.tiles_y = (int32_t)num();
            fprintf(out, "%s |%s\n", name(kc::clahe_check_config(err, fn.c_str(), &c)), err);
        } else if (cmd == "CF") {
            prefix();
            vio_flow_config c;
            c.levels = (int32_t)num(); c.half_patch = (int32_t)num(); c.max_iter = (int32_t)num(); c.inverse = (int32_t)num();
            c.border = (int32_t)num(); c.early_stop = (int32_t)num();
            fprintf(out, "%s |%s\n", name(kf::flow_check_config(err, fn.c_str(), &c)), err);
        } else if (cmd == "CD") {
            prefix();
            vio_detect_config c;
            c.quality = num(); c.min_distance = (int32_t)num(); c.reserved = 0;
            fprintf(out, "%s |%s\n", name(kd::det_check_config(err, fn.c_str(), &c)), err);
        } else if (cmd == "CR") {
            prefix();
            vio_reject_config c;
            c.seed = 0; c.ransac_hypotheses = (int32_t)num(); c.f_threshold = num(); c.focal_length = num();
            fprintf(out, "%s |%s\n", name(kr::rej_check_config(err, fn.c_str(), &c)), err);
        } else if (cmd == "CM") {
            prefix();
            vio_reject_camera c;
            c.model = (int32_t)num();
            c.fx = num(); c.fy = num(); c.cx = num(); c.cy = num(); c.k1 = num(); c.k2 = num(); c.p1 = num(); c.p2 = num();
            c.width = (int32_t)num(); c.height = (int32_t)num(); c.reserved = 0;
            fprintf(out, "%s |%s\n", name(kr::rej_check_camera(err, fn.c_str(), &c)), err);
        } else if (cmd == "DF") {
            const vio_clahe_config c = kc::CLAHE_DEFAULTS;
            const vio_flow_config f = kf::FLOW_DEFAULTS;
            const vio_detect_config d = kd::DET_DEFAULTS;
            const vio_reject_config r = kr::REJ_DEFAULTS;
            fprintf(out, "%s ", name(kc::clahe_check_config(err, "", &c)));
            fprintf(out, "%s ", name(kf::flow_check_config(err, "", &f)));
            fprintf(out, "%s ", name(kd::det_check_config(err, "", &d)));
            fprintf(out, "%s |%s\n", name(kr::rej_check_config(err, "", &r)), err);
        } else if (cmd == "N") {
            item_prefix();
            const int n_tracked = (int)num(), max_total = (int)num();
            fprintf(out, "%s |%s\n", name(kd::det_check_counts(err, fn.c_str(), 7, n_tracked, max_total)), err);
        } else if (cmd == "T") {
            item_prefix();
            const int n = (int)num();
            std::vector<float> pts(2 * (size_t)n);          // (exactly n rows: a read past them is the sanitizer's to catch)
            for (float &v : pts) v = (float)num();
            int32_t active = -1;
            const vio_status st = kd::det_check_tracked(err, fn.c_str(), 7, pts.data(), n, 3, 2, &active);
            fprintf(out, "%s %d |%s\n", name(st), (int)active, err);
        } else if (cmd == "S") {
            const int count = (int)num();
            const int64_t n_trk = (int64_t)num(), n_new = (int64_t)num();
            const kd::DetSizes S = kd::det_sizes(count, n_trk, n_new);
            fprintf(out, "%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", S.b_it, S.b_tab, S.b_res, S.b_keep, S.b_out, S.b_key, S.b_scratch,
                    sizeof(kd::DetItemD), sizeof(kd::DetTrk), sizeof(kd::DetRes));
        } else if (cmd == "L") {
            const int width = (int)num(), height = (int)num(), levels = (int)num();
            kf::FlowItemD d;
            std::memset(&d, 0, sizeof(d));
            const bool ok = kf::flow_level_dims(width, height, levels, d.w, d.h);
            fprintf(out, "%d", ok ? 1 : 0);
            if (ok) {
                kf::flow_item(d, levels, d.w, d.h, d.w);
                FrameLayout Y;
                const bool lay = frame_layout(width, height, levels, Y);
                fprintf(out, " %d %d", (int)d.active, lay ? 1 : 0);
                for (int l = 0; l < levels; ++l) fprintf(out, " %d %d %d %d %d", d.w[l], d.h[l], d.pitch[l], Y.w[l], Y.h[l]);
            }
            fprintf(out, "\n");
        } else if (cmd == "U") {
            const int n_tracked = (int)num(), max_total = (int)num(), active = (int)num(), dev_kept = (int)num(), dev_new = (int)num();
            // one item whose rows start at 2 (trk) and 3 (newp) in the call's tables; the caller's arrays are exactly as long as stated,
            // each in a heap block of its own with guard bytes (0xA5) on both sides
            const int G = 64;
            const kd::DetSizes S = kd::det_sizes(1, 2 + n_tracked, 3 + max_total);
            std::vector<char> out_h(S.b_out + 1, 0);
            kd::DetRes *res = (kd::DetRes *)out_h.data();
            res->n_kept = dev_kept; res->n_new = dev_new; res->n_cand = 11;
            const double maxr = 2.5;
            std::memcpy(&res->maxbits, &maxr, sizeof(double));
            int32_t *keep = (int32_t *)(out_h.data() + S.b_res);
            float *newp = (float *)(out_h.data() + S.b_res + S.b_keep);
            for (int k = 0; k < 2 + n_tracked; ++k) keep[k] = 100 + k;
            for (int k = 0; k < 2 * (3 + max_total); ++k) newp[k] = (float)(1000 + k);
            std::vector<uint8_t> kb(2 * G + sizeof(int32_t) * (size_t)n_tracked, 0xA5), nb(2 * G + sizeof(float) * 2 * (size_t)max_total, 0xA5);
            vio_detect_item it;
            std::memset(&it, 0, sizeof(it));
            it.n_tracked = n_tracked; it.max_total = max_total;
            it.keep_order = (int32_t *)(kb.data() + G); it.new_pts = (float *)(nb.data() + G);
            kd::DetItemD d;
            std::memset(&d, 0, sizeof(d));
            d.active = active; d.trk = 2; d.newp = 3;
            vio_detect_result r;
            std::memset(&r, 0x7f, sizeof(r));
            const vio_status st = kd::det_unpack(err, out_h.data(), S, 1, &it, &d, &r);
            bool guards = true;
            for (int k = 0; k < G; ++k)
                guards = guards && kb[(size_t)k] == 0xA5 && kb[kb.size() - 1 - (size_t)k] == 0xA5 && nb[(size_t)k] == 0xA5 && nb[nb.size() - 1 - (size_t)k] == 0xA5;
            fprintf(out, "%s %s %d %d %d %.17g %d %g |", name(st), name((vio_status)r.status), r.n_kept, r.n_new, r.n_candidates, r.max_response,
                    guards ? 1 : 0, r.n_new > 0 ? (double)it.new_pts[0] : -1.0);
            for (int k = 0; k < n_tracked; ++k) fprintf(out, " %d", it.keep_order[k]);
            fprintf(out, " |%s\n", err);
        } else {
            fprintf(out, "?\n");
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
