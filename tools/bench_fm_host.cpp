// bench_fm_host.cpp — the per-stream path of tools/bench_fm_batch.py: B host mirrors vio::FeatureManager (host/feature_manager.cpp),
// each with its waiting vio_triangulate on one shared context, looped over the streams in C++.  Built by the tool into a small shared
// object beside libvio_hip.so and called in the tool's process; the frame is timed here with the host clock, so nothing of Python is
// in it.  One frame of a stream: addFeatureCheckParallax, triangulate, getDepthVector, setDepth with the vector's magnitudes (every
// 50th negative), removeFailures, and at frame_count == WINDOW_SIZE the slide the keyframe decision asks for.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../visual-inertial-odometry_amd/host/feature_manager.h"

namespace {

struct Streams {
    vio_ctx *ctx = nullptr;
    std::vector<std::vector<vio::FeaturePerId>> tracks;
    std::vector<vio::FeatureManager> fm;
};

}  // namespace

extern "C" {

__attribute__((visibility("default"))) void *fmh_create(int32_t streams) {
    Streams *s = new Streams();
    vio_config cfg;
    vio_default_config(&cfg);
    if (vio_create(&cfg, &s->ctx) != VIO_OK) { delete s; return nullptr; }
    s->tracks.resize((size_t)streams);
    s->fm.reserve((size_t)streams);
    for (int i = 0; i < streams; ++i) s->fm.emplace_back(s->tracks[(size_t)i]);
    return s;
}

__attribute__((visibility("default"))) void fmh_destroy(void *h) {
    Streams *s = (Streams *)h;
    if (!s) return;
    vio_destroy(s->ctx);
    delete s;
}

// One frame of every stream; ids [streams][n], pts [streams][n][2], poses [11][7], ext [7], the four slide matrices.  Returns the ms
// the loop took, -1 on an error of vio_triangulate; keyframe [streams] and n_tracks [streams] are what each stream ended with.
__attribute__((visibility("default"))) double fmh_frame(void *h, int32_t frame_count, int32_t n, const int32_t *ids, const double *pts,
                                                         const double *poses, const double *ext, const double *marg_R, const double *marg_P,
                                                         const double *new_R, const double *new_P, int32_t *keyframe, int32_t *n_tracks) {
    Streams *s = (Streams *)h;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < s->fm.size(); ++i) {
        vio::FeatureManager &fm = s->fm[i];
        const bool key = fm.addFeatureCheckParallax(frame_count, n, ids + i * (size_t)n, pts + 2 * i * (size_t)n);
        if (!fm.triangulate(s->ctx, (const double(*)[7])poses, ext)) return -1.0;
        std::vector<double> x = fm.getDepthVector();
        for (size_t k = 0; k < x.size(); ++k) x[k] = k % 50 == 0 ? -std::fabs(x[k]) : std::fabs(x[k]);
        fm.setDepth(x);
        fm.removeFailures();
        if (frame_count == vio::WINDOW_SIZE) {
            if (key) fm.removeBackShiftDepth(marg_R, marg_P, new_R, new_P);
            else fm.removeFront(frame_count);
        }
        keyframe[i] = key ? 1 : 0;
        n_tracks[i] = (int32_t)fm.feature.size();
    }
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // extern "C"
