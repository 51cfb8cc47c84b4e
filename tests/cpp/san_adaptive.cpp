// tests/cpp/san_adaptive.cpp -- the host code of adaptive accumulations under AddressSanitizer + UBSan
// (CPU only, Makefile `san`): ort_debug_emulate_adaptive on the debug scene by brute force -- pass
// lists with thresholds 0, 0.05 and +inf, a band tile past the frame, every output alone, all in
// buffers of exactly the bytes the call covers -- against ort_debug_emulate_moments at each pixel's
// own count; ort_debug_adaptive_decision on stored states with NaN, +inf and huge sums; and the
// argument checks of the three calls, which must come back as codes with nothing written.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ort_internal.h"

namespace {

void check(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "san_adaptive: FAILED %s (%s)\n", what, ort_last_error(nullptr));
        std::exit(1);
    }
}

}  // namespace

int main() {
    int32_t ns = 0;
    check(ort_scene_debug(nullptr, nullptr, nullptr, &ns) == ORT_OK && ns > 0, "ort_scene_debug");
    std::vector<float> cr(4 * ns), ma(4 * ns), fr(4 * ns);
    check(ort_scene_debug(cr.data(), ma.data(), fr.data(), &ns) == ORT_OK, "ort_scene_debug arrays");
    ort_params p;
    std::memset(&p, 0, sizeof p);
    p.width = 13;
    p.height = 9;
    p.num_samples = 9;
    p.max_depth = 4;
    p.use_octree = 0;
    const float pos[3] = {0.0f, 1.0f, -4.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    check(ort_camera_view(pos, up, 90.0f, 0.0f, p.view) == ORT_OK, "ort_camera_view");
    std::memcpy(p.camera_position, pos, sizeof pos);
    p.camera_zoom = 45.0f;
    const int N = p.num_samples;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const ort_tile tiles[2] = {{0, 13, 0, 9, 0, 0}, {3, 7, 1, 6, 2, 4}};  // the second: rows 1-2, 5-6, 9-10 (past the frame)
    const float thresholds[3] = {0.0f, 0.05f, inf};
    const int splits[3][4] = {{1, 1, 1, 1}, {2, 3, 4, 7}, {5, 16, 1, 1}};
    int runs = 0;
    for (const ort_tile& t : tiles) {
        const size_t px = (size_t)t.width * t.rows;
        // the plain moments at every count
        std::vector<std::vector<float>> pm(N + 1), pv(N + 1);
        for (int k = 1; k <= N; ++k) {
            pm[k].resize(3 * px);
            pv[k].resize(px);
            check(ort_debug_emulate_moments(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                            nullptr, 0, ORT_LAYOUT_COMPACT, &p, &t, k, pm[k].data(), pv[k].data()) == ORT_OK,
                  "ort_debug_emulate_moments");
        }
        for (float thr : thresholds)
            for (const auto& split : splits)
                for (int min_samples : {0, 3}) {
                    ort_accum_adaptive passes[4];
                    int sum = 0;
                    for (int i = 0; i < 4; ++i) {
                        passes[i] = {split[i], min_samples, thr, 0.05f, {0, 0, 0, 0}};
                        sum += split[i];
                    }
                    std::vector<int32_t> counts(px);
                    std::vector<float> mean(3 * px), var(px);
                    check(ort_debug_emulate_adaptive(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                     0, nullptr, 0, ORT_LAYOUT_COMPACT, &p, &t, passes, 4, counts.data(), mean.data(),
                                                     var.data()) == ORT_OK,
                          "ort_debug_emulate_adaptive");
                    for (int j = 0; j < t.rows; ++j) {
                        const int y = t.band_height > 0 ? t.y0 + (j / t.band_height) * t.band_stride + j % t.band_height : t.y0 + j;
                        for (int c = 0; c < t.width; ++c) {
                            const size_t i = (size_t)j * t.width + c;
                            const int k = counts[i];
                            if (y >= p.height) {
                                check(k == 0 && mean[3 * i] == 0.0f && mean[3 * i + 1] == 0.0f && mean[3 * i + 2] == 0.0f && var[i] == -1.0f,
                                      "padding rows");
                                continue;
                            }
                            check(k >= 1 && k <= N, "a count in 1 .. N");
                            if (thr == 0.0f) check(k == (sum < N ? sum : N), "threshold 0 traces every pixel");
                            check(std::memcmp(&mean[3 * i], &pm[k][3 * i], 12) == 0 && std::memcmp(&var[i], &pv[k][i], 4) == 0,
                                  "a pixel's moments are the plain ones at its own count");
                        }
                    }
                    // one output at a time
                    std::vector<int32_t> c2(px);
                    std::vector<float> v2(px);
                    check(ort_debug_emulate_adaptive(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                     0, nullptr, 0, ORT_LAYOUT_COMPACT, &p, &t, passes, 4, c2.data(), nullptr, nullptr) == ORT_OK &&
                              c2 == counts,
                          "counts alone");
                    check(ort_debug_emulate_adaptive(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                     0, nullptr, 0, ORT_LAYOUT_COMPACT, &p, &t, passes, 4, nullptr, nullptr, v2.data()) == ORT_OK &&
                              std::memcmp(v2.data(), var.data(), 4 * px) == 0,
                          "variance alone");
                    ++runs;
                }
    }

    // the decision on stored states
    const ort_accum_adaptive crit = {1, 0, 0.05f, 0.05f, {0, 0, 0, 0}};
    const float grey[3] = {2.0f, 2.0f, 2.0f};
    check(ort_debug_adaptive_decision(4, 16, &crit, grey, 1.0f) == 0, "zero variance is held");
    check(ort_debug_adaptive_decision(16, 16, &crit, grey, 1.0f) == 0 && ort_debug_adaptive_decision(17, 16, &crit, grey, 1.0f) == 0,
          "k >= N is held");
    check(ort_debug_adaptive_decision(0, 16, &crit, grey, 0.0f) == 1 && ort_debug_adaptive_decision(1, 16, &crit, grey, 0.0f) == 1,
          "no estimate below two samples");
    int decisions = 5;
    for (float bad : {nan, inf, 3.0e38f})
        for (int ch = 0; ch < 4; ++ch) {
            float col[3] = {2.0f, 2.0f, 2.0f};
            float m2 = 1.0f;
            if (ch < 3)
                col[ch] = bad;
            else
                m2 = bad;
            for (float thr : {0.05f, 1.0e30f, inf}) {
                const ort_accum_adaptive c = {1, 0, thr, 0.05f, {0, 0, 0, 0}};
                const int d = ort_debug_adaptive_decision(4, 16, &c, col, m2);
                check(d == 0 || d == 1, "a decision");
                if (!std::isfinite(bad)) check(d == 1, "a non-finite sum is never held");
                ++decisions;
            }
        }

    // refusals: codes, nothing written
    std::vector<int32_t> keep(tiles[0].width * tiles[0].rows, -7);
    const ort_accum_adaptive bads[] = {{0, 0, 0.05f, 0.05f, {0, 0, 0, 0}},  {1, -1, 0.05f, 0.05f, {0, 0, 0, 0}}, {1, 0, -0.5f, 0.05f, {0, 0, 0, 0}},
                                       {1, 0, nan, 0.05f, {0, 0, 0, 0}},    {1, 0, 0.05f, 0.0f, {0, 0, 0, 0}},   {1, 0, 0.05f, inf, {0, 0, 0, 0}},
                                       {1, 0, 0.05f, nan, {0, 0, 0, 0}},    {1, 0, 0.05f, 0.05f, {0, 0, 0, 1}},  {1, 0, 0.05f, 0.05f, {1, 0, 0, 0}}};
    for (const ort_accum_adaptive& b : bads) {
        const ort_accum_adaptive two[2] = {crit, b};
        check(ort_debug_emulate_adaptive(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                         ORT_LAYOUT_COMPACT, &p, &tiles[0], two, 2, keep.data(), nullptr, nullptr) == ORT_ERR_INVALID_ARG,
              "a bad pass is refused");
        check(ort_debug_adaptive_decision(4, 16, &b, grey, 1.0f) == -1, "a bad criterion is refused");
    }
    check(ort_debug_emulate_adaptive(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                     ORT_LAYOUT_COMPACT, &p, &tiles[0], &crit, 1, nullptr, nullptr, nullptr) == ORT_ERR_INVALID_ARG,
          "no output refused");
    check(ort_debug_emulate_adaptive(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                     ORT_LAYOUT_COMPACT, &p, &tiles[0], nullptr, 1, keep.data(), nullptr, nullptr) == ORT_ERR_INVALID_ARG,
          "null passes refused");
    struct ort_accum_adaptive_stats st;
    std::memset(&st, 0x5a, sizeof st);
    const struct ort_accum_adaptive_stats st0 = st;
    check(ort_accum_render_adaptive(nullptr, nullptr, &crit, nullptr, nullptr) == ORT_ERR_INVALID_ARG, "render: null refused");
    check(ort_accum_read_counts(nullptr, nullptr, keep.data(), 0, nullptr) == ORT_ERR_INVALID_ARG, "read_counts: null refused");
    check(ort_accum_adaptive_stats(nullptr, nullptr, &crit, &st) == ORT_ERR_INVALID_ARG, "stats: null refused");
    check(std::memcmp(&st, &st0, sizeof st) == 0, "a refused stats call writes nothing");
    for (int32_t v : keep) check(v == -7, "a refused call writes nothing");
    std::printf("san_adaptive: %d adaptive emulations on 2 tiles, %d decisions, refusals: ok\n", runs, decisions);
    return 0;
}
