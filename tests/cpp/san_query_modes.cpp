// tests/cpp/san_query_modes.cpp -- the query modes' host code under AddressSanitizer + UBSan (CPU
// only, Makefile `san`): ort_debug_query_rays_ex, the mode kernels' per-ray function (render_core.h
// query_ray_mode) compiled for the host, in ORT_QUERY_DRAWN, NEAREST and ANY over ordinary and
// degenerate rays and intervals on the compact layout (depth 5 and 9), the explicit layout and
// brute force.  NEAREST must give the same records on every walk, ANY the same flags, DRAWN the
// records of ort_debug_query_rays, and ort_trace_rays_ex' argument errors must come back as codes.
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
        std::fprintf(stderr, "san_query_modes: FAILED %s (%s)\n", what, ort_last_error(nullptr));
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

const float kInf = std::numeric_limits<float>::infinity(), kNan = std::numeric_limits<float>::quiet_NaN();
const float kMax = std::numeric_limits<float>::max();

// A deterministic ray set with intervals: origins in and around the root box (some exactly on a
// node's plane along a zero axis), directions of mixed lengths, then the degenerate rays; intervals
// ordinary, inverted, open-ended, starting at 0, NaN and negative.
void make_rays(const Tree& t, int n, std::vector<float>& r, std::vector<float>& range) {
    uint32_t x = 12345u;
    auto u = [&]() {
        x = x * 1664525u + 1013904223u;
        return (float)(x >> 8) / 16777216.0f;
    };
    for (int i = 0; i < n; ++i) {
        float o[3], d[3] = {2.0f * u() - 1.0f, 2.0f * u() - 1.0f, 2.0f * u() - 1.0f};
        for (int a = 0; a < 3; ++a) o[a] = t.nmin[a] + (t.nmax[a] - t.nmin[a]) * (1.1f * u() - 0.05f);
        if (i % 7 == 0) {
            d[i % 3] = (i & 8) ? 0.0f : -0.0f;
            if (i % 14 == 0) o[i % 3] = t.nmin[3 * (size_t)((uint32_t)i % (uint32_t)t.n_nodes) + i % 3];
        }
        const float scale = (i % 5 == 0) ? 1000.0f : ((i % 5 == 1) ? 0.001f : 1.0f);
        for (int a = 0; a < 3; ++a) r.push_back(o[a]);
        for (int a = 0; a < 3; ++a) r.push_back(d[a] * scale);
        const float lo = (i % 3 == 0) ? 0.001f : ((i % 3 == 1) ? 0.0f : 20.0f * u() / scale);
        const float hi = (i % 4 == 0) ? kMax : ((i % 4 == 1) ? kInf : 40.0f * u() / scale);
        range.push_back(i % 97 == 0 ? kNan : (i % 101 == 0 ? -1.0f : lo));
        range.push_back(i % 89 == 0 ? kNan : hi);
    }
    const float odd[][6] = {{0, 2.5f, -10, 0, 0, 0},      {0, 2.5f, -10, kInf, 0, 1},  {0, 2.5f, -10, kNan, 0, 1},
                            {kNan, 2.5f, -10, 0, 0, 1},   {0, kInf, -10, 0, 0, 1},     {0, 2.5f, -10, 0, 0, 1e-30f},
                            {1000, 1000, 1000, 0, 6e19f, 8e19f}, {kInf, -kInf, kNan, kNan, kInf, -kInf}};
    for (const auto& o : odd) {
        r.insert(r.end(), o, o + 6);
        range.push_back(0.0f);
        range.push_back(kInf);
    }
}

void mode_case(const char* name, int32_t n, uint32_t seed, int depth, int per_node) {
    std::vector<float> cr(4 * (size_t)n), ma(4 * (size_t)n), fr(4 * (size_t)n);
    check(ort_scene_random(n, seed, cr.data(), ma.data(), fr.data()) == ORT_OK, "ort_scene_random");
    const Tree t = build(cr, n, depth, per_node);
    std::vector<float> rays, range;
    make_rays(t, 1500, rays, range);
    const int64_t nr = (int64_t)(rays.size() / 6);
    auto run = [&](int layout, int use_octree, int mode, const float* tr, std::vector<ort_ray_hit>& h, float* nrm) {
        return ort_debug_query_rays_ex(cr.data(), n, t.nmin.data(), t.nmax.data(), t.co.data(), t.oo.data(), t.cnt.data(),
                                       (int32_t)t.n_nodes, t.idx.data(), t.n_indices, layout, use_octree, rays.data(), nr, mode, tr,
                                       h.data(), nrm);
    };
    long long hits = 0, any_hits = 0;
    for (const float* tr : {(const float*)nullptr, (const float*)range.data()}) {
        std::vector<ort_ray_hit> hc(nr), he(nr), hb(nr), ac(nr), ae(nr), ab(nr);
        std::vector<float> nc(3 * nr), ne(3 * nr), nb(3 * nr), na(3 * nr);
        check(run(ORT_LAYOUT_COMPACT, 1, ORT_QUERY_NEAREST, tr, hc, nc.data()) == ORT_OK, "compact nearest");
        check(run(ORT_LAYOUT_EXPLICIT, 1, ORT_QUERY_NEAREST, tr, he, ne.data()) == ORT_OK, "explicit nearest");
        check(run(ORT_LAYOUT_COMPACT, 0, ORT_QUERY_NEAREST, tr, hb, nb.data()) == ORT_OK, "brute-force nearest");
        check(std::memcmp(hc.data(), hb.data(), sizeof(ort_ray_hit) * nr) == 0, "compact nearest == brute-force nearest");
        check(std::memcmp(he.data(), hb.data(), sizeof(ort_ray_hit) * nr) == 0, "explicit nearest == brute-force nearest");
        check(std::memcmp(nc.data(), nb.data(), sizeof(float) * 3 * nr) == 0, "compact normals == brute-force normals");
        check(std::memcmp(ne.data(), nb.data(), sizeof(float) * 3 * nr) == 0, "explicit normals == brute-force normals");
        check(run(ORT_LAYOUT_COMPACT, 1, ORT_QUERY_ANY, tr, ac, na.data()) == ORT_OK, "compact any");
        check(run(ORT_LAYOUT_EXPLICIT, 1, ORT_QUERY_ANY, tr, ae, nullptr) == ORT_OK, "explicit any");
        check(run(ORT_LAYOUT_COMPACT, 0, ORT_QUERY_ANY, tr, ab, nullptr) == ORT_OK, "brute-force any");
        for (int64_t i = 0; i < nr; ++i) {
            const bool hit = hb[i].sphere >= 0;
            check((ac[i].sphere >= 0) == hit && (ae[i].sphere >= 0) == hit && (ab[i].sphere >= 0) == hit, "any-hit flag == nearest's");
            if (hit) {
                ++(tr ? any_hits : hits);
                check(hb[i].sphere < n && ac[i].t >= hb[i].t && ae[i].t >= hb[i].t && ab[i].t >= hb[i].t, "any hit no nearer than the nearest");
                if (tr) check(hb[i].t > tr[2 * i] && hb[i].t < tr[2 * i + 1], "nearest t inside the interval");
            } else {
                check(hc[i].t == 0.0f && nc[3 * i] == 0.0f && nc[3 * i + 1] == 0.0f && nc[3 * i + 2] == 0.0f, "miss record");
            }
            if (tr && !(tr[2 * i] >= 0.0f && tr[2 * i] < tr[2 * i + 1])) check(!hit, "an invalid interval misses");
        }
        for (int64_t i = nr - 8; i < nr; ++i) check(hc[i].sphere == -1 && ac[i].sphere == -1, "degenerate rays miss");
    }
    check(hits * 20 > nr && any_hits * 40 > nr, "enough rays hit");
    // DRAWN through the _ex entry point is the query of ort_debug_query_rays; it takes no interval
    std::vector<ort_ray_hit> d0(nr), d1(nr);
    check(run(ORT_LAYOUT_COMPACT, 1, ORT_QUERY_DRAWN, nullptr, d1, nullptr) == ORT_OK, "drawn");
    check(ort_debug_query_rays(cr.data(), n, t.nmin.data(), t.nmax.data(), t.co.data(), t.oo.data(), t.cnt.data(), (int32_t)t.n_nodes,
                               t.idx.data(), t.n_indices, ORT_LAYOUT_COMPACT, 1, rays.data(), nr, d0.data(), nullptr) == ORT_OK,
          "ort_debug_query_rays");
    check(std::memcmp(d0.data(), d1.data(), sizeof(ort_ray_hit) * nr) == 0, "drawn == ort_debug_query_rays");
    check(run(ORT_LAYOUT_COMPACT, 1, ORT_QUERY_DRAWN, range.data(), d1, nullptr) == ORT_ERR_INVALID_ARG, "drawn with a t_range");
    check(run(ORT_LAYOUT_COMPACT, 1, 3, nullptr, d1, nullptr) == ORT_ERR_INVALID_ARG, "unknown mode");
    std::printf("ok %s: %lld rays, %lld hits, %lld inside the intervals\n", name, (long long)nr, hits, any_hits);
}

}  // namespace

int main() {
    mode_case("1000 spheres d5 m1", 1000, 7, 5, 1);
    mode_case("2000 spheres d9 m1", 2000, 5, 9, 1);
    mode_case("100 spheres d4 m0", 100, 42, 4, 0);
    mode_case("50 spheres depth 0", 50, 1, 0, 0);
    {  // the entry point's argument errors, as codes, without a context
        check(ort_trace_rays_ex(nullptr, nullptr, nullptr) == ORT_ERR_INVALID_ARG, "ort_trace_rays_ex(null ctx)");
    }
    std::printf("san_query_modes: all cases passed\n");
    return 0;
}
