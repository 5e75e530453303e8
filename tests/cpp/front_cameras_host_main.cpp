// front_cameras_host_main.cpp — tests/test_front_cameras_cpu.py's driver: the slot cameras of libvio_frame_hip
// (csrc/vio_frame_cameras.h), built by a plain C++ compiler with no HIP header.  It reads one command per line and answers with one
// line; a text follows a '|'.
//
//   H fx fy cx cy k1 k2 p1 p2 w h        rej_check_camera, then set_handle_camera        -> status | text
//   S slot model w h p0 .. p15           set (the slot's own camera)                     -> status | text
//   N slot                               set with a NULL camera                          -> status | text
//   C slot                               clear                                           -> status | text
//   P n slot ...                         path of a read of the listed slots              -> path bad
//   D                                    take_dirty                                      -> 0 or 1
//   Q                                    dirty, without taking it                        -> 0 or 1, n_own
//   T slot                               the table's entry                               -> own set model npow no_distortion half_w half_h c0 .. c15
//   G slot                               the slot's own camera as it was given           -> own model w h reserved p0 .. p15
//   E fx fy cx cy k1 k2 p1 p2 w h        the handle's CamDev against rej_camera's RejCam and rejectWithF's half sizes -> 1 if equal in every bit
//   I slot clamped bad                   lift_info_set                                   -> OK
//   J slot                               the slot's lift counts                          -> n_clamped n_bad
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "../../include/vio_camera.h"
#include "../../include/vio_reject.h"
#include "vio_host_base.h"
#include "vio_camera_math.h"

namespace kq {
#include "vio_camera_host.h"
}
#include "vio_frame_cameras.h"

static const char *name(vio_status st) {
    static char other[32];
    if (st == VIO_OK) return "OK";
    if (st == VIO_ERR_BAD_ARG) return "BAD_ARG";
    snprintf(other, sizeof(other), "%d", (int)st);
    return other;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    FrameCameras *cams = new FrameCameras();                // (on the heap: a read past the tables is the sanitizer's to catch)
    char line[4096];
    while (fgets(line, sizeof(line), in)) {
        std::istringstream ss(line);
        std::string cmd;
        ss >> cmd;
        ErrText err = {0};
        const auto num = [&]() { std::string t; ss >> t; return strtod(t.c_str(), nullptr); };
        const auto reject_camera = [&]() {
            vio_reject_camera c;
            std::memset(&c, 0, sizeof(c));
            c.fx = num(); c.fy = num(); c.cx = num(); c.cy = num(); c.k1 = num(); c.k2 = num(); c.p1 = num(); c.p2 = num();
            c.width = (int32_t)num(); c.height = (int32_t)num(); c.model = VIO_REJECT_MODEL_PINHOLE;
            return c;
        };
        if (cmd == "H") {
            const vio_reject_camera c = reject_camera();
            const vio_status st = kq::rej_check_camera(err, "vio_frame_set_camera", &c);
            if (st == VIO_OK) cams->set_handle_camera(c);
            fprintf(out, "%s |%s\n", name(st), err);
        } else if (cmd == "S") {
            const int slot = (int)num();
            vio_camera_model m;
            std::memset(&m, 0, sizeof(m));
            m.model = (int32_t)num(); m.width = (int32_t)num(); m.height = (int32_t)num(); m.reserved = 77;
            for (double &p : m.params) p = num();
            fprintf(out, "%s |%s\n", name(cams->set(err, slot, &m)), err);
        } else if (cmd == "N") {
            const int slot = (int)num();
            fprintf(out, "%s |%s\n", name(cams->set(err, slot, nullptr)), err);
        } else if (cmd == "C") {
            const int slot = (int)num();
            fprintf(out, "%s |%s\n", name(cams->clear(err, slot)), err);
        } else if (cmd == "P") {
            const int n = (int)num();
            int32_t *slots = new int32_t[(size_t)n];        // (exactly n entries)
            for (int i = 0; i < n; ++i) slots[i] = (int32_t)num();
            int32_t bad = -7;
            const FrameCamPath p = cams->path(n, slots, &bad);
            delete[] slots;
            fprintf(out, "%d %d\n", (int)p, (int)bad);
        } else if (cmd == "D") {
            fprintf(out, "%d\n", cams->take_dirty() ? 1 : 0);
        } else if (cmd == "Q") {
            fprintf(out, "%d %d\n", cams->dirty ? 1 : 0, (int)cams->n_own);
        } else if (cmd == "T") {
            const int slot = (int)num();
            const CamDev &d = cams->table[slot];
            fprintf(out, "%d %d %d %d %d %.17g %.17g", (int)cams->own[slot], d.set, d.model, d.npow, d.no_distortion, d.half_w, d.half_h);
            for (double c : d.c) fprintf(out, " %.17g", c);
            fprintf(out, "\n");
        } else if (cmd == "G") {
            const int slot = (int)num();
            const vio_camera_model &m = cams->model[slot];
            fprintf(out, "%d %d %d %d %d", (int)cams->own[slot], m.model, m.width, m.height, m.reserved);
            for (double p : m.params) fprintf(out, " %.17g", p);
            fprintf(out, "\n");
        } else if (cmd == "E") {
            const vio_reject_camera c = reject_camera();
            const RejCam r = rej_camera(c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2);
            const CamDev &d = cams->handle_dev;
            const double want[8] = {r.ik11, r.ik13, r.ik22, r.ik23, r.k1, r.k2, r.p1, r.p2};
            bool eq = d.set == 1 && d.model == VIO_CAMERA_MODEL_PINHOLE && d.no_distortion == r.no_distortion;
            for (int i = 0; i < 8; ++i) eq = eq && same_bits(d.c[i], want[i]);
            for (int i = 8; i < VIO_CAMERA_MAX_PARAMS; ++i) eq = eq && same_bits(d.c[i], 0.0);
            eq = eq && same_bits(d.half_w, c.width / 2.0) && same_bits(d.half_h, c.height / 2.0);
            fprintf(out, "%d\n", eq ? 1 : 0);
        } else if (cmd == "I") {
            const int slot = (int)num(), clamped = (int)num(), bad = (int)num();
            cams->lift_info_set(slot, clamped, bad);
            fprintf(out, "OK\n");
        } else if (cmd == "J") {
            const int slot = (int)num();
            fprintf(out, "%d %d\n", (int)cams->n_clamped[slot], (int)cams->n_bad[slot]);
        } else {
            fprintf(out, "?\n");
        }
    }
    delete cams;
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
