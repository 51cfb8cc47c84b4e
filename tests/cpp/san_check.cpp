// tests/cpp/san_check.cpp -- host ASan/UBSan run of the scene stage (scene.cpp: the
// reference's sphere generators), the octree builder (octree.cpp), the layout compilers
// (layout.cpp, via the emulation), the C ABI's host side (host_abi.cpp), the kernel's
// per-pixel code compiled for the host (ort_debug_emulate_render, render_core.h), the group
// partition/assembly (ort_debug_group_emulate) and the oracle (oracle/ort_oracle.c).
// Built by `make san` (every object instrumented, clang's runtime); no GPU is touched.
// Each case renders a small frame through the emulation (compact and explicit layouts) and
// through the oracle and requires identical bits, like tests/test_emulation.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ort_internal.h"

extern "C" {
#include "ort_oracle.h"
}

namespace {

struct Scene {
    std::vector<float> cr, ma, fr;
    int n = 0;
};

struct Tree {
    std::vector<float> mn, mx;
    std::vector<int32_t> co, oo, cnt, idx;
};

int failures = 0;

void check(bool ok, const char* what, const char* name) {
    if (!ok) {
        std::printf("FAIL %s: %s (%s)\n", name, what, ort_last_error(nullptr));
        ++failures;
    }
}

bool build(const Scene& s, int depth, int mspn, Tree& t) {
    ort_octree* o = nullptr;
    if (ort_octree_build(s.cr.data(), s.n, depth, mspn, &o) != ORT_OK) return false;
    int64_t nn = 0, ni = 0;
    double secs = 0;
    ort_octree_sizes(o, &nn, &ni, &secs);
    t.mn.resize(3 * nn);
    t.mx.resize(3 * nn);
    t.co.resize(nn);
    t.oo.resize(nn);
    t.cnt.resize(nn);
    t.idx.resize(ni > 0 ? ni : 1);
    const int rc = ort_octree_export(o, t.mn.data(), t.mx.data(), t.co.data(), t.oo.data(), t.cnt.data(), t.idx.data());
    t.idx.resize(ni);
    ort_octree_free(o);
    return rc == ORT_OK;
}

ort_params camera(int w, int h, int spp, int bounces, int use_octree) {
    ort_params p{};
    p.width = w;
    p.height = h;
    p.num_samples = spp;
    p.max_depth = bounces;
    p.use_octree = use_octree;
    const float pos[3] = {0.0f, 2.5f, -10.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    ort_camera_view(pos, up, -90.0f, 0.0f, p.view);
    std::memcpy(p.camera_position, pos, sizeof pos);
    p.camera_zoom = 45.0f;
    return p;
}

void render_case(const char* name, const Scene& s, int depth, int mspn, int w, int h, int spp, int bounces) {
    Tree t;
    if (!build(s, depth, mspn, t)) {
        check(false, "octree build", name);
        return;
    }
    const int nn = (int)t.co.size();
    const size_t px = (size_t)w * h;
    for (int use_octree = 1; use_octree >= 0; --use_octree) {
        const ort_params p = camera(w, h, spp, bounces, use_octree);
        oracle_scene os{s.cr.data(), s.ma.data(), s.fr.data(), s.n, t.mn.data(), t.mx.data(), t.co.data(),
                        t.oo.data(), t.cnt.data(), nn, t.idx.data(), (long long)t.idx.size()};
        oracle_params op;
        std::memcpy(&op, &p, sizeof op);
        std::vector<float> ref(3 * px);
        uint64_t rc[ORACLE_COUNT_N] = {0};
        check(oracle_render(&os, &op, 0, 0, w, h, 0, 0, ref.data(), rc, 1) == 0, "oracle render", name);
        const ort_tile tile{0, w, 0, h, 0, 0};
        for (int layout = 0; layout < (use_octree ? 2 : 1); ++layout) {
            std::vector<float> out(3 * px, -1.0f);
            uint64_t cnt[ORT_COUNT_N] = {0};
            const int e = ort_debug_emulate_render(s.cr.data(), s.ma.data(), s.fr.data(), s.n, t.mn.data(), t.mx.data(),
                                                   t.co.data(), t.oo.data(), t.cnt.data(), nn, t.idx.data(),
                                                   (int64_t)t.idx.size(), layout, &p, &tile, out.data(), cnt);
            check(e == ORT_OK, "emulated render", name);
            check(std::memcmp(out.data(), ref.data(), 4 * out.size()) == 0, "emulation != oracle bits", name);
            for (int k = 0; k < ORT_COUNT_N; ++k) check(cnt[k] == rc[k], "reference-walk work counters", name);
        }
        if (use_octree) {  // 3 band tiles, in-memory transport, assembled by the group's row map
            std::vector<float> g(3 * px, -1.0f);
            check(ort_debug_group_emulate(s.cr.data(), s.ma.data(), s.fr.data(), s.n, t.mn.data(), t.mx.data(),
                                          t.co.data(), t.oo.data(), t.cnt.data(), nn, t.idx.data(),
                                          (int64_t)t.idx.size(), 3, &p, g.data()) == ORT_OK,
                  "group emulation", name);
            check(std::memcmp(g.data(), ref.data(), 4 * g.size()) == 0, "group frame != oracle bits", name);
        }
    }
    std::printf("ok %s: %d nodes, %zu indices\n", name, nn, t.idx.size());
}

// The row limit (include/ort.h ort_tile) on a 48 x 32 frame: `refused` tiles, whose last row's pixel
// row passes 2^31 - 1, return an error from the emulation and the oracle and leave the output alone
// (before the limit the row arithmetic overflowed a signed int here); the largest accepted tiles lie
// wholly past the frame and are all zeros.
void limit_case(const char* name, const Scene& s, ort_tile tile, bool refused) {
    Tree t;
    if (!build(s, 3, 1, t)) {
        check(false, "octree build", name);
        return;
    }
    const int nn = (int)t.co.size();
    const ort_params p = camera(48, 32, 2, 2, 1);
    oracle_scene os{s.cr.data(), s.ma.data(), s.fr.data(), s.n, t.mn.data(), t.mx.data(), t.co.data(),
                    t.oo.data(), t.cnt.data(), nn, t.idx.data(), (long long)t.idx.size()};
    oracle_params op;
    std::memcpy(&op, &p, sizeof op);
    const size_t n = 3 * (size_t)tile.width * (size_t)tile.rows;
    std::vector<float> ref(n, -7.0f);
    const int orc = oracle_render(&os, &op, tile.x0, tile.y0, tile.width, tile.rows, tile.band_height, tile.band_stride,
                                  ref.data(), nullptr, 1);
    for (int layout = 0; layout < 2; ++layout) {
        std::vector<float> out(n, -7.0f);
        uint64_t cnt[ORT_COUNT_N] = {0};
        const int e = ort_debug_emulate_render(s.cr.data(), s.ma.data(), s.fr.data(), s.n, t.mn.data(), t.mx.data(),
                                               t.co.data(), t.oo.data(), t.cnt.data(), nn, t.idx.data(),
                                               (int64_t)t.idx.size(), layout, &p, &tile, out.data(), cnt);
        if (refused) {
            check(e == ORT_ERR_INVALID_ARG, "a tile past the row limit must be refused", name);
            for (float v : out) check(v == -7.0f, "a refused tile's output was written", name);
        } else {
            check(e == ORT_OK, "emulated render", name);
            for (float v : out) check(v == 0.0f && !std::signbit(v), "rows past the frame are zeros", name);
            check(cnt[ORT_COUNT_PIXELS] == 0, "no pixel of the tile is inside the frame", name);
        }
    }
    if (refused) {
        check(orc != 0, "the oracle must refuse a tile past the row limit", name);
        for (float v : ref) check(v == -7.0f, "the refusing oracle wrote its output", name);
    } else {
        check(orc == 0, "oracle render", name);
        for (float v : ref) check(v == 0.0f && !std::signbit(v), "oracle: rows past the frame are zeros", name);
    }
    std::printf("ok %s\n", name);
}

Scene random_scene(int n, uint32_t seed) {
    Scene s;
    s.n = n;
    s.cr.resize(4 * (size_t)n + 4);
    s.ma.resize(4 * (size_t)n + 4);
    s.fr.resize(4 * (size_t)n + 4);
    if (ort_scene_random(n, seed, s.cr.data(), s.ma.data(), s.fr.data()) != ORT_OK) ++failures;
    return s;
}

}  // namespace

int main() {
    render_case("c1 100 spheres d4 m0, 2 spp 3 bounces", random_scene(100, 42), 4, 0, 40, 30, 2, 3);
    render_case("1000 spheres d5 m1", random_scene(1000, 7), 5, 1, 48, 27, 1, 4);
    render_case("300 spheres d3 m2", random_scene(300, 3), 3, 2, 32, 24, 1, 2);
    render_case("depth 0", random_scene(50, 1), 0, 0, 24, 16, 1, 2);
    render_case("negative maxSpheresPerNode", random_scene(64, 9), 6, -1, 24, 16, 1, 2);
    render_case("depth 9 (96-bit walk)", random_scene(2000, 5), 9, 1, 32, 18, 1, 3);
    {
        Scene s;
        int32_t n = 0;
        ort_scene_prebuilt(nullptr, nullptr, nullptr, &n);
        s.n = n;
        s.cr.resize(4 * n);
        s.ma.resize(4 * n);
        s.fr.resize(4 * n);
        check(ort_scene_prebuilt(s.cr.data(), s.ma.data(), s.fr.data(), &n) == ORT_OK, "prebuilt", "prebuilt");
        render_case("prebuilt scene d5", s, 5, 0, 32, 24, 2, 4);
        check(ort_scene_debug(s.cr.data(), s.ma.data(), s.fr.data(), &n) == ORT_OK && n == 3, "debug scene", "debug");
        s.n = n;
        render_case("debug scene d3 m2", s, 3, 2, 24, 16, 1, 3);
    }
    {  // coincident and tangent spheres
        Scene s = random_scene(40, 11);
        for (int i = 1; i < 10; ++i) std::memcpy(&s.cr[4 * i], &s.cr[0], 4 * sizeof(float));
        s.cr[4 * 10 + 0] = s.cr[0] + 2.0f * s.cr[3];
        s.cr[4 * 10 + 1] = s.cr[1];
        s.cr[4 * 10 + 2] = s.cr[2];
        s.cr[4 * 10 + 3] = s.cr[3];
        render_case("coincident + tangent spheres d5 m1", s, 5, 1, 24, 16, 1, 3);
    }
    {  // frames at the kernels' unit sizes (tests/shape_sets.py groups A-D): below and around an 8 x 8 wave
       // block, a 16 x 16 tile and a tile pair; the group emulation's 3 ranks then outnumber the bands
        const Scene s = random_scene(100, 42);
        const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 5}, {7, 9}, {8, 8}, {9, 7}, {15, 17}, {16, 16}, {17, 15},
                                 {31, 1}, {32, 2}, {33, 3}};
        for (const auto& wh : shapes) {
            char name[64];
            std::snprintf(name, sizeof name, "unit size %d x %d, 2 spp 3 bounces", wh[0], wh[1]);
            render_case(name, s, 4, 1, wh[0], wh[1], 2, 3);
        }
        limit_case("refused: y0 + rows past INT_MAX", s, ort_tile{0, 8, 2147483640, 16, 0, 0}, true);
        limit_case("refused: band stride 2^30, row 2", s, ort_tile{0, 8, 0, 3, 1, 1 << 30}, true);
        limit_case("refused: band stride INT_MAX", s, ort_tile{0, 8, 40, 4, 2, 2147483647}, true);
        limit_case("refused: one row past INT_MAX", s, ort_tile{0, 8, 2147483647, 2, 0, 0}, true);
        limit_case("accepted: one row at INT_MAX", s, ort_tile{0, 8, 2147483647, 1, 0, 0}, false);
        limit_case("accepted: eight rows up to INT_MAX", s, ort_tile{0, 8, 2147483640, 8, 0, 0}, false);
        limit_case("accepted: a band tile whose last row is INT_MAX", s, ort_tile{0, 8, 40, 4, 2, 2147483606}, false);
    }
    {  // error paths of the host ABI
        ort_octree* o = nullptr;
        check(ort_octree_build(nullptr, 0, 3, 0, &o) != ORT_OK, "empty sphere list must fail", "errors");
        check(ort_scene_random(-1, 0, nullptr, nullptr, nullptr) != ORT_OK, "negative count must fail", "errors");
    }
    if (failures) {
        std::printf("san_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("san_check: all cases passed\n");
    return 0;
}
