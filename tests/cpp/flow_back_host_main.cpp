// flow_back_host_main.cpp — tests/test_flow_back_host_cpu.py's program: the host side of the forward-backward check
// (csrc/vio_flow_host.h: flow_check_back, flow_back_levels, flow_back_args, flow_unpack_back; csrc/vio_flow_math.h: flow_back_verdict),
// built by a plain C++ compiler with no HIP header, with ASan and UBSan, and run directly.  It checks itself: every failed expectation
// prints its line and the program returns 1.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define __device__
#define __forceinline__ inline
#include "../../include/vio_flow.h"
#include "vio_host_base.h"
#include "vio_flow_math.h"

namespace kf {
#include "vio_flow_host.h"
}

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); failures += 1; } } while (0)

static vio_flow_back_config cfg(int enabled, int levels, double max_dist) {
    vio_flow_back_config c;
    c.enabled = enabled; c.levels = levels; c.max_dist = max_dist;
    return c;
}

static void check_configs() {
    ErrText err = {0};
    EXPECT(kf::flow_check_back(err, "f", nullptr, 4) == VIO_OK && err[0] == 0);
    const vio_flow_back_config good[] = {cfg(1, 0, 0.5), cfg(0, 0, 0.5), cfg(1, 4, 0.0), cfg(1, 1, 1e30), cfg(1, 2, DBL_MAX), cfg(0, 4, 0.5)};
    for (const vio_flow_back_config &c : good) {
        err[0] = 0;
        EXPECT(kf::flow_check_back(err, "f", &c, 4) == VIO_OK && err[0] == 0);
    }
    const vio_flow_back_config bad[] = {cfg(2, 0, 0.5), cfg(-1, 0, 0.5), cfg(1, -1, 0.5), cfg(1, 5, 0.5), cfg(0, 5, 0.5), cfg(1, 0, -1e-300),
                                        cfg(1, 0, NAN), cfg(1, 0, INFINITY), cfg(1, 0, -INFINITY)};
    for (const vio_flow_back_config &c : bad) {
        err[0] = 0;
        EXPECT(kf::flow_check_back(err, "vio_flow_set_back", &c, 4) == VIO_ERR_BAD_ARG);
        EXPECT(std::string(err) == "vio_flow_set_back: the check's enabled 0 or 1, its levels in [0, 4] (the flow levels), max_dist finite and >= 0");
    }
    // the levels are held to the flow levels they run under
    const vio_flow_back_config three = cfg(1, 3, 0.5);
    EXPECT(kf::flow_check_back(err, "f", &three, 3) == VIO_OK && kf::flow_check_back(err, "f", &three, 2) == VIO_ERR_BAD_ARG);
    EXPECT(kf::flow_back_levels(cfg(1, 0, 0.5), 4) == 4 && kf::flow_back_levels(cfg(1, 2, 0.5), 4) == 2 && kf::flow_back_levels(cfg(1, 4, 0.5), 4) == 4);
    EXPECT(kf::FLOW_BACK_DEFAULTS.enabled == 0 && kf::FLOW_BACK_DEFAULTS.levels == 0 && kf::FLOW_BACK_DEFAULTS.max_dist == 0.5);
}

static void check_args() {
    kf::FlowItemD items[1];
    kf::FlowPt pts[1];
    kf::FlowOut out[1];
    kf::FlowBackOut back[1];
    vio_flow_config c = kf::FLOW_DEFAULTS;
    c.half_patch = 5; c.max_iter = 7; c.border = 3; c.early_stop = 1; c.inverse = 1;
    const kf::FlowArgs f = kf::flow_args(items, pts, out, 140, 3, c);
    const kf::FlowBackArgs a = kf::flow_back_args(items, pts, out, back, 140, 3, c, cfg(1, 2, 0.3));
    EXPECT(a.f.items == f.items && a.f.pts == f.pts && a.f.out == f.out && a.f.npts == 140 && a.f.levels == 3 && a.f.half_patch == 5 &&
           a.f.max_iter == 7 && a.f.border == 3 && a.f.early_stop == 1);
    EXPECT(a.back == back && a.back_levels == 2 && a.pad == 0);
    const double d = 0.3;
    EXPECT(a.max_d2 == d * d);
    EXPECT(kf::flow_back_args(items, pts, out, back, 1, 3, c, cfg(1, 0, 0.0)).back_levels == 3);
    EXPECT(kf::flow_back_args(items, pts, out, back, 1, 3, c, cfg(1, 0, 0.0)).max_d2 == 0.0);
    EXPECT(std::isinf(kf::flow_back_args(items, pts, out, back, 1, 3, c, cfg(1, 0, 1e200)).max_d2));
    EXPECT(sizeof(kf::FlowBackOut) == 32 && sizeof(vio_flow_back_info) == 32 && sizeof(vio_flow_back_config) == 16 && sizeof(kf::FlowOut) == 24);
}

static void check_verdict() {
    double d2 = -1.0;
    EXPECT(flow_back_verdict(true, 1.f, 2.f, 1.f, 2.f, 0.0, d2) == VIO_OK && d2 == 0.0);
    EXPECT(flow_back_verdict(true, 1.f, 2.f, 4.f, 6.f, 25.0, d2) == VIO_OK && d2 == 25.0);
    EXPECT(flow_back_verdict(true, 1.f, 2.f, 4.f, 6.f, std::nextafter(25.0, 0.0), d2) == VIO_FLOW_FAIL_BACK_FAR && d2 == 25.0);
    EXPECT(flow_back_verdict(false, 1.f, 2.f, 1.f, 2.f, 25.0, d2) == VIO_FLOW_FAIL_BACK_LOST && d2 == 0.0);
    EXPECT(flow_back_verdict(true, 1.f, 2.f, NAN, 2.f, INFINITY, d2) == VIO_FLOW_FAIL_BACK_FAR && std::isnan(d2));
}

struct Item {
    int32_t n_pts;
};

// the unpacking of the backward rows over items of 0, 1 and 140 points, into arrays of exactly the rows there are
static void check_unpack() {
    const std::vector<Item> items = {{0}, {1}, {140}, {0}};
    const size_t total = 141;
    std::vector<kf::FlowBackOut> rows(total);
    for (size_t k = 0; k < total; ++k) {
        kf::FlowBackOut &o = rows[k];
        o.x = (float)k + 0.25f; o.y = -(float)k; o.status = (int32_t)(k % 3) - 1; o.iterations = (int32_t)k; o.cost = 2.0 * (double)k; o.d2 = k % 5 ? 0.125 * (double)k : NAN;
    }
    std::vector<vio_flow_back_info> back(total);            // (ASan watches both ends)
    std::memset(back.data(), 0xAB, sizeof(vio_flow_back_info) * total);
    kf::flow_unpack_back(rows.data(), (int)items.size(), items.data(), back.data());
    for (size_t k = 0; k < total; ++k) {
        const vio_flow_back_info &b = back[k];
        EXPECT(b.x == (float)k + 0.25f && b.y == -(float)k && b.status == (int32_t)(k % 3) - 1 && b.iterations == (int32_t)k && b.cost == 2.0 * (double)k);
        EXPECT(k % 5 ? b.d2 == 0.125 * (double)k : std::isnan(b.d2));
    }
    // a call without keypoints touches nothing
    const std::vector<Item> none = {{0}, {0}};
    kf::flow_unpack_back(rows.data(), 2, none.data(), (vio_flow_back_info *)nullptr);
    kf::flow_unpack_back(rows.data(), 0, none.data(), (vio_flow_back_info *)nullptr);
    // the forward rows of the same items still unpack as before beside them, the check's statuses passing through
    std::vector<kf::FlowOut> fw(total);
    for (size_t k = 0; k < total; ++k) { fw[k].x = (float)k; fw[k].y = 1.f; fw[k].status = (int32_t)(k % 5); fw[k].iterations = 1; fw[k].cost = 0.5; }
    std::vector<float> next(2 * total);
    std::vector<vio_flow_pt_info> info(total);
    ErrText err = {0};
    EXPECT(kf::flow_unpack(err, fw.data(), (int)items.size(), items.data(), next.data(), info.data()) == VIO_OK);
    for (size_t k = 0; k < total; ++k) EXPECT(info[k].status == (int32_t)(k % 5) && next[2 * k] == (float)k);
}

int main() {
    check_configs();
    check_args();
    check_verdict();
    check_unpack();
    if (failures) printf("FAILED %d\n", failures);
    else printf("ok\n");
    return failures ? 1 : 0;
}
