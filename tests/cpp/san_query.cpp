// tests/cpp/san_query.cpp -- the ray queries' host code under AddressSanitizer + UBSan (CPU only,
// Makefile `san`): ort_debug_query_rays, the kernels' per-ray function (render_core.h query_ray)
// compiled for the host, over ordinary and degenerate rays on the compact layout (depth 5 and the
// 96-bit walk of depth 9), the explicit layout and brute force; the compact and the explicit walk
// must give the same records, and ort_trace_rays' argument errors must come back as codes.
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
        std::fprintf(stderr, "san_query: FAILED %s (%s)\n", what, ort_last_error(nullptr));
        std::exit(1);
    }
}

struct Tree {
    std::vector<float> nmin, nmax;
    std::vector<int32_t> co, oo, cnt, idx;
    int64_t n_nodes = 0, n_indices = 0;
};

Tree build(const std::vector<float>& cr, int32_t n, int depth, int per_node) {
    ort_octree* h = nullptr;
    check(ort_octree_build(cr.data(), n, depth, per_node, &h) == ORT_OK, "ort_octree_build");
    Tree t;
    double secs = 0.0;
    check(ort_octree_sizes(h, &t.n_nodes, &t.n_indices, &secs) == ORT_OK, "ort_octree_sizes");
    t.nmin.resize(3 * t.n_nodes);
    t.nmax.resize(3 * t.n_nodes);
    t.co.resize(t.n_nodes);
    t.oo.resize(t.n_nodes);
    t.cnt.resize(t.n_nodes);
    t.idx.resize(t.n_indices > 0 ? t.n_indices : 1);
    check(ort_octree_export(h, t.nmin.data(), t.nmax.data(), t.co.data(), t.oo.data(), t.cnt.data(), t.idx.data()) == ORT_OK,
          "ort_octree_export");
    ort_octree_free(h);
    return t;
}

// A deterministic ray set: origins in and around the root box, directions of mixed lengths, some
// with zero components, then the degenerate ones.
std::vector<float> make_rays(const Tree& t, int n) {
    std::vector<float> r;
    uint32_t x = 12345u;
    auto u = [&]() {
        x = x * 1664525u + 1013904223u;
        return (float)(x >> 8) / 16777216.0f;
    };
    for (int i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) r.push_back(t.nmin[a] + (t.nmax[a] - t.nmin[a]) * (1.1f * u() - 0.05f));
        float d[3] = {2.0f * u() - 1.0f, 2.0f * u() - 1.0f, 2.0f * u() - 1.0f};
        if (i % 7 == 0) d[i % 3] = (i & 8) ? 0.0f : -0.0f;
        const float scale = (i % 5 == 0) ? 1000.0f : ((i % 5 == 1) ? 0.001f : 1.0f);
        for (int a = 0; a < 3; ++a) r.push_back(d[a] * scale);
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float odd[][6] = {{0, 2.5f, -10, 0, 0, 0},      {0, 2.5f, -10, inf, 0, 1},   {0, 2.5f, -10, nan, 0, 1},
                            {nan, 2.5f, -10, 0, 0, 1},    {0, inf, -10, 0, 0, 1},      {0, 2.5f, -10, 0, 0, 1e-30f},
                            {1000, 1000, 1000, 0, 6e19f, 8e19f}, {inf, -inf, nan, nan, inf, -inf}};
    for (const auto& o : odd) r.insert(r.end(), o, o + 6);
    return r;
}

void query_case(const char* name, int32_t n, uint32_t seed, int depth, int per_node) {
    std::vector<float> cr(4 * (size_t)n), ma(4 * (size_t)n), fr(4 * (size_t)n);
    check(ort_scene_random(n, seed, cr.data(), ma.data(), fr.data()) == ORT_OK, "ort_scene_random");
    const Tree t = build(cr, n, depth, per_node);
    const std::vector<float> rays = make_rays(t, 1500);
    const int64_t nr = (int64_t)(rays.size() / 6);
    std::vector<ort_ray_hit> hc(nr), he(nr), hb(nr);
    std::vector<float> nc(3 * nr), ne(3 * nr), nb(3 * nr);
    auto run = [&](int layout, int use_octree, std::vector<ort_ray_hit>& h, float* nrm) {
        return ort_debug_query_rays(cr.data(), n, t.nmin.data(), t.nmax.data(), t.co.data(), t.oo.data(), t.cnt.data(),
                                    (int32_t)t.n_nodes, t.idx.data(), t.n_indices, layout, use_octree, rays.data(), nr, h.data(),
                                    nrm);
    };
    check(run(ORT_LAYOUT_COMPACT, 1, hc, nc.data()) == ORT_OK, "compact query");
    check(run(ORT_LAYOUT_EXPLICIT, 1, he, ne.data()) == ORT_OK, "explicit query");
    check(run(ORT_LAYOUT_COMPACT, 0, hb, nb.data()) == ORT_OK, "brute-force query");
    check(std::memcmp(hc.data(), he.data(), sizeof(ort_ray_hit) * nr) == 0, "compact records == explicit records");
    check(std::memcmp(nc.data(), ne.data(), sizeof(float) * 3 * nr) == 0, "compact normals == explicit normals");
    int64_t hits = 0;
    for (int64_t i = 0; i < nr; ++i) {
        if (hc[i].sphere >= 0) {
            ++hits;
            check(hc[i].sphere < n && hb[i].sphere >= 0 && hb[i].t <= hc[i].t, "brute force hits no later than the octree walk");
        } else {
            check(hc[i].t == 0.0f && nc[3 * i] == 0.0f && nc[3 * i + 1] == 0.0f && nc[3 * i + 2] == 0.0f, "miss record");
        }
    }
    for (int64_t i = nr - 8; i < nr; ++i) check(hc[i].sphere == -1 && hb[i].sphere == -1, "degenerate rays miss");
    check(hits * 20 > nr, "at least a twentieth of the rays hit");
    // without normals: a null pointer is never written
    std::vector<ort_ray_hit> h2(nr);
    check(run(ORT_LAYOUT_COMPACT, 1, h2, nullptr) == ORT_OK && std::memcmp(h2.data(), hc.data(), sizeof(ort_ray_hit) * nr) == 0,
          "records without normals");
    std::printf("ok %s: %lld rays, %lld hits\n", name, (long long)nr, (long long)hits);
}

}  // namespace

int main() {
    query_case("1000 spheres d5 m1", 1000, 7, 5, 1);
    query_case("2000 spheres d9 m1 (96-bit walk)", 2000, 5, 9, 1);
    query_case("100 spheres d4 m0", 100, 42, 4, 0);
    query_case("50 spheres depth 0", 50, 1, 0, 0);
    {  // the entry points' argument errors, as codes, without a context
        ort_ray_hit h;
        check(ort_trace_rays(nullptr, nullptr, nullptr) == ORT_ERR_INVALID_ARG, "ort_trace_rays(null ctx)");
        float ms;
        check(ort_last_query_ms(nullptr, &ms) == ORT_ERR_INVALID_ARG, "ort_last_query_ms(null ctx)");
        const float cr[4] = {0, 0, 0, 1};
        check(ort_debug_query_rays(cr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, ORT_LAYOUT_COMPACT, 1,
                                   cr, 0, &h, nullptr) == ORT_ERR_NO_SCENE, "octree query without a tree");
        check(ort_debug_query_rays(cr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, ORT_LAYOUT_COMPACT, 0,
                                   nullptr, 1, &h, nullptr) == ORT_ERR_INVALID_ARG, "null rays");
    }
    std::printf("san_query: all cases passed\n");
    return 0;
}
