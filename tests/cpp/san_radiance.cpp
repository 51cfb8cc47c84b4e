// tests/cpp/san_radiance.cpp -- the radiance queries' host code under AddressSanitizer + UBSan (CPU
// only, Makefile `san`): ort_debug_radiance_rays, the kernels' per-bounce functions (render_core.h
// trace_ray, hit_record, shade_bounce) compiled for the host and chained per ray as
// ort_trace_radiance chains them, over ordinary and degenerate rays and valid and invalid states on
// the compact layout (depth 5 and 9) and brute force.  paths = 4 must equal four paths = 1 calls
// chained through states_out, an aliased states_out the separate one, an invalid state zeros and
// its echo, and the argument errors must come back as codes.
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
        std::fprintf(stderr, "san_radiance: FAILED %s (%s)\n", what, ort_last_error(nullptr));
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

// Rays from in and around the root box with unit directions (every 7th with a zero component, every
// 5th scaled), then the degenerate ones; states in [0, 1) from an LCG.
void make_rays(const Tree& t, int n, std::vector<float>& r, std::vector<float>& st) {
    uint32_t x = 2463534242u;
    auto u = [&]() {
        x = x * 1664525u + 1013904223u;
        return (float)(x >> 8) / 16777216.0f;
    };
    for (int i = 0; i < n; ++i) {
        float o[3], d[3] = {2.0f * u() - 1.0f, 2.0f * u() - 1.0f, 2.0f * u() - 1.0f};
        for (int a = 0; a < 3; ++a) o[a] = t.nmin[a] + (t.nmax[a] - t.nmin[a]) * (1.1f * u() - 0.05f);
        if (i % 7 == 0) d[i % 3] = (i & 8) ? 0.0f : -0.0f;
        const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const float scale = (i % 5 == 0 ? 100.0f : 1.0f) / (len > 0.0f ? len : 1.0f);
        for (int a = 0; a < 3; ++a) r.push_back(o[a]);
        for (int a = 0; a < 3; ++a) r.push_back(d[a] * scale);
    }
    const float odd[][6] = {{0, 2.5f, -10, 0, 0, 0},      {0, 2.5f, -10, kInf, 0, 1},  {0, 2.5f, -10, kNan, 0, 1},
                            {kNan, 2.5f, -10, 0, 0, 1},   {0, kInf, -10, 0, 0, 1},     {0, 2.5f, -10, 0, 0, 1e-30f},
                            {1000, 1000, 1000, 0, 6e19f, 8e19f}, {kInf, -kInf, kNan, kNan, kInf, -kInf}};
    for (const auto& o : odd) r.insert(r.end(), o, o + 6);
    for (size_t i = 0; i < r.size() / 6; ++i) {
        st.push_back(u());
        st.push_back(u());
    }
}

bool same(const std::vector<float>& a, const std::vector<float>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (std::memcmp(&a[i], &b[i], 4) != 0 && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
    return true;
}

void radiance_case(const char* name, int32_t n, uint32_t seed, int depth, int per_node, int use_octree) {
    std::vector<float> cr(4 * (size_t)n), ma(4 * (size_t)n), fr(4 * (size_t)n);
    check(ort_scene_random(n, seed, cr.data(), ma.data(), fr.data()) == ORT_OK, "ort_scene_random");
    const Tree t = build(cr, n, depth, per_node);
    std::vector<float> rays, states;
    make_rays(t, 600, rays, states);
    const int64_t nr = (int64_t)(rays.size() / 6);
    auto run = [&](const float* st, int64_t count, int max_depth, int paths, int flags, float* rad, float* out) {
        return ort_debug_radiance_rays(cr.data(), ma.data(), fr.data(), n, t.nmin.data(), t.nmax.data(), t.co.data(), t.oo.data(),
                                       t.cnt.data(), (int32_t)t.n_nodes, t.idx.data(), t.n_indices, ORT_LAYOUT_COMPACT, use_octree,
                                       rays.data(), st, count, max_depth, paths, flags, rad, out);
    };
    // paths = 4 == four single paths chained, summed in order and divided
    std::vector<float> rad4(3 * nr), st4(2 * nr), sum(3 * nr, 0.0f), one(3 * nr), st = states, next(2 * nr);
    check(run(states.data(), nr, 8, 4, 0, rad4.data(), st4.data()) == ORT_OK, "paths = 4");
    for (int k = 0; k < 4; ++k) {
        check(run(st.data(), nr, 8, 1, 0, one.data(), next.data()) == ORT_OK, "paths = 1");
        for (size_t i = 0; i < sum.size(); ++i) sum[i] += one[i];
        st = next;
    }
    for (float& v : sum) v /= 4.0f;
    check(same(sum, rad4) && same(st, st4), "paths = 4 == four chained paths");
    // states_out aliased to states; without states_out; sorted (accepted, no effect)
    std::vector<float> alias = states, rad(3 * nr);
    check(run(alias.data(), nr, 8, 4, ORT_QUERY_SORT, rad.data(), alias.data()) == ORT_OK, "aliased states_out");
    check(same(rad, rad4) && same(alias, st4), "aliased states_out == separate");
    check(run(states.data(), nr, 8, 4, 0, rad.data(), nullptr) == ORT_OK && same(rad, rad4), "no states_out");
    // gamma and normalize run; an invalid state gives zeros and its echo
    check(run(states.data(), nr, 3, 2, ORT_RADIANCE_GAMMA | ORT_RADIANCE_NORMALIZE, rad.data(), next.data()) == ORT_OK, "gamma + normalize");
    std::vector<float> bad = states;
    bad[0] = 1.0f;
    bad[3] = -0.25f;
    bad[4] = kNan;
    check(run(bad.data(), nr, 8, 4, 0, rad.data(), next.data()) == ORT_OK, "invalid states");
    for (int i = 0; i < 3; ++i) {
        check(rad[3 * i] == 0.0f && rad[3 * i + 1] == 0.0f && rad[3 * i + 2] == 0.0f, "an invalid state gives zeros");
        check(std::memcmp(&next[2 * i], &bad[2 * i], 8) == 0, "an invalid state is echoed");
    }
    check(same(std::vector<float>(rad.begin() + 9, rad.end()), std::vector<float>(rad4.begin() + 9, rad4.end())),
          "the other rays as ever");
    long long lit = 0;
    for (int64_t i = 0; i < nr; ++i) lit += rad4[3 * i] > 0.0f ? 1 : 0;
    check(lit * 2 > nr, "most rays see light");
    // the refusals, as codes, with the outputs untouched
    std::vector<float> keep(3 * nr, -7.0f), keep_st(2 * nr, -7.0f);
    const int inval = ORT_ERR_INVALID_ARG;
    check(run(states.data(), nr, 0, 1, 0, keep.data(), keep_st.data()) == inval, "max_depth 0");
    check(run(states.data(), nr, 1, 0, 0, keep.data(), keep_st.data()) == inval, "paths 0");
    check(run(states.data(), nr, 1, 65537, 0, keep.data(), keep_st.data()) == inval, "paths 65537");
    check(run(states.data(), nr, 1, 1, 8, keep.data(), keep_st.data()) == inval, "unknown flag");
    check(run(states.data(), -1, 1, 1, 0, keep.data(), keep_st.data()) == inval, "n_rays < 0");
    check(run(nullptr, nr, 1, 1, 0, keep.data(), keep_st.data()) == inval, "null states");
    check(run(states.data(), nr, 1, 1, 0, nullptr, keep_st.data()) == inval, "null radiance");
    check(run(states.data(), nr, 1, 1, 0, keep.data(), states.data() + 2) == inval, "states_out overlapping states");
    check(run((const float*)((const char*)states.data() + 1), nr, 1, 1, 0, keep.data(), nullptr) == inval, "misaligned states");
    for (float v : keep) check(v == -7.0f, "refused: radiance untouched");
    for (float v : keep_st) check(v == -7.0f, "refused: states_out untouched");
    check(run(states.data(), 0, 1, 1, 0, keep.data(), keep_st.data()) == ORT_OK && keep[0] == -7.0f, "n_rays == 0");
    std::printf("ok %s: %lld rays, %lld lit\n", name, (long long)nr, lit);
}

}  // namespace

int main() {
    radiance_case("1000 spheres d5 m1", 1000, 7, 5, 1, 1);
    radiance_case("2000 spheres d9 m1", 2000, 5, 9, 1, 1);
    radiance_case("100 spheres brute force", 100, 42, 4, 0, 0);
    radiance_case("50 spheres depth 0", 50, 1, 0, 0, 1);
    {  // the entry point's argument errors, as codes, without a context
        check(ort_trace_radiance(nullptr, nullptr, nullptr) == ORT_ERR_INVALID_ARG, "ort_trace_radiance(null ctx)");
    }
    std::printf("san_radiance: all cases passed\n");
    return 0;
}
