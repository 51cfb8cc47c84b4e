// tests/cpp/san_camera.cpp -- the camera queries' host code under AddressSanitizer + UBSan (CPU
// only, Makefile `san`): ort_debug_camera_query -- the kernels' per-pixel ray (camera_query.inc
// camera_query_ray) and per-ray walk compiled for the host -- over whole frames, a banded tile and a
// tile reaching past the frame, both kinds of ray, on the compact layout (depth 5 and the 96-bit
// walk of depth 9), the explicit layout and brute force; a tiling must give the frame's records,
// rows past the frame must be empty, and ort_trace_camera's argument errors must come back as codes.
// Also the layout export hooks (ort_debug_layout, ort_debug_lds_image_rev) on the same two trees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ort_internal.h"

namespace {

void check(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "san_camera: FAILED %s (%s)\n", what, ort_last_error(nullptr));
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

struct Records {
    std::vector<float> rays, normals;
    std::vector<ort_ray_hit> hits;
    explicit Records(size_t n) : rays(6 * n), normals(3 * n), hits(n) {}
};

ort_params frame(int w, int h, int ns, int use_octree) {
    ort_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = w;
    p.height = h;
    p.num_samples = ns;
    p.max_depth = 1;
    p.use_octree = use_octree;
    const float pos[3] = {0.0f, 2.5f, -10.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    check(ort_camera_view(pos, up, -90.0f, 0.0f, p.view) == ORT_OK, "ort_camera_view");
    std::memcpy(p.camera_position, pos, sizeof pos);
    p.camera_zoom = 45.0f;
    return p;
}

void camera_case(const char* name, int32_t n, uint32_t seed, int depth, int per_node) {
    std::vector<float> cr(4 * (size_t)n), ma(4 * (size_t)n), fr(4 * (size_t)n);
    check(ort_scene_random(n, seed, cr.data(), ma.data(), fr.data()) == ORT_OK, "ort_scene_random");
    const Tree t = build(cr, n, depth, per_node);
    {  // the layout export hooks (tests/layout_cases.py): every array into a buffer of exactly its size
        std::vector<uint32_t> planes;
        int tree_depth = -1;
        for (const char* what : {"node", "kid", "leaf_sph", "leaf_idx", "leaf16", "depth", "ordered", "planes"}) {
            int64_t bytes = -1;
            auto get = [&](void* out, int64_t cap) {
                return ort_debug_layout(cr.data(), n, t.nmin.data(), t.nmax.data(), t.co.data(), t.oo.data(), t.cnt.data(),
                                        (int32_t)t.n_nodes, t.idx.data(), t.n_indices, what, out, cap, &bytes);
            };
            check(get(nullptr, 0) == ORT_OK && bytes >= 0 && bytes % 4 == 0, what);
            planes.assign((size_t)bytes / 4, 0u);
            check(get(planes.data(), bytes) == ORT_OK, what);
            if (bytes > 4) check(get(planes.data(), bytes - 1) == ORT_ERR_INVALID_ARG, "a buffer too small is refused");
            if (!std::strcmp(what, "depth")) tree_depth = (int)planes[0];
        }
        check(tree_depth >= 0 && tree_depth <= depth && (int64_t)planes.size() == 3 * (((int64_t)1 << tree_depth) + 1),
              "planes of the tree's depth");
        for (int rev = 0; rev < 2; ++rev) {
            int32_t lay[7];
            check(ort_debug_lds_image_rev(tree_depth, (const float*)planes.data(), rev, nullptr, 0, lay) == ORT_OK, "image size");
            std::vector<uint32_t> img((size_t)lay[0] / 4);
            check(ort_debug_lds_image_rev(tree_depth, (const float*)planes.data(), rev, img.data(), (int64_t)img.size(), lay) == ORT_OK,
                  "LDS image");
        }
    }
    const int W = 37, H = 21;
    for (int which : {ORT_CAMERA_FIRST_SAMPLE, ORT_CAMERA_PIXEL_CENTRE}) {
        for (int mode = 0; mode < 3; ++mode) {  // compact, explicit, brute force
            const ort_params p = frame(W, H, 4, mode == 2 ? 0 : 1);
            const int layout = mode == 1 ? ORT_LAYOUT_EXPLICIT : ORT_LAYOUT_COMPACT;
            auto run = [&](const ort_tile& tile, Records& r) {
                return ort_debug_camera_query(cr.data(), n, t.nmin.data(), t.nmax.data(), t.co.data(), t.oo.data(),
                                              t.cnt.data(), (int32_t)t.n_nodes, t.idx.data(), t.n_indices, layout, &p, &tile,
                                              which, r.rays.data(), r.hits.data(), r.normals.data());
            };
            Records full((size_t)W * H);
            const ort_tile whole{0, W, 0, H, 0, 0};
            check(run(whole, full) == ORT_OK, name);
            size_t hit = 0;
            for (const ort_ray_hit& h : full.hits) hit += h.sphere >= 0;
            check(hit > 0 && hit < full.hits.size(), "some pixels hit and some miss");
            // a banded tile reaching past the frame: rows 12, 13, 14, 19, 20, 21 -- the last one empty
            const ort_tile band{5, 20, 12, 6, 3, 7};
            Records part((size_t)20 * 6);
            check(run(band, part) == ORT_OK, "banded tile");
            const int ys[6] = {12, 13, 14, 19, 20, 21};
            for (int j = 0; j < 6; ++j)
                for (int c = 0; c < 20; ++c) {
                    const size_t i = (size_t)j * 20 + c, k = (size_t)ys[j] * W + 5 + c;
                    if (ys[j] >= H) {
                        const float zero[6] = {0, 0, 0, 0, 0, 0};
                        check(part.hits[i].sphere == -1 && part.hits[i].t == 0.0f &&
                                  std::memcmp(&part.rays[6 * i], zero, 24) == 0 && std::memcmp(&part.normals[3 * i], zero, 12) == 0,
                              "a row past the frame is empty");
                    } else {
                        check(std::memcmp(&part.hits[i], &full.hits[k], sizeof(ort_ray_hit)) == 0 &&
                                  std::memcmp(&part.rays[6 * i], &full.rays[6 * k], 24) == 0 &&
                                  std::memcmp(&part.normals[3 * i], &full.normals[3 * k], 12) == 0,
                              "a tile gives the frame's records");
                    }
                }
            // rays only: no scene array is read
            Records only((size_t)W * H);
            check(ort_debug_camera_query(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, layout, &p, &whole,
                                         which, only.rays.data(), nullptr, nullptr) == ORT_OK, "rays only");
            check(std::memcmp(only.rays.data(), full.rays.data(), 4 * full.rays.size()) == 0, "rays only gives the same rays");
        }
    }
    std::printf("san_camera: %s ok\n", name);
}

}  // namespace

int main() {
    camera_case("2000 spheres, depth 5", 2000, 7, 5, 1);
    camera_case("3000 spheres, depth 9", 3000, 11, 9, 1);
    {  // the entry points' argument errors, as codes, without a context or a scene
        const ort_params p = frame(8, 4, 1, 1);
        ort_params p0 = p;
        p0.num_samples = 0;
        const ort_tile tile{0, 8, 0, 4, 0, 0}, outside{4, 8, 0, 4, 0, 0};
        std::vector<float> rays(6 * 32, 7.0f);
        ort_camera_query q;
        std::memset(&q, 0, sizeof(q));
        q.rays = (ort_ray*)rays.data();
        check(ort_trace_camera(nullptr, &p, &tile, &q, nullptr) == ORT_ERR_INVALID_ARG, "ort_trace_camera(null ctx)");
        auto gen = [&](const ort_params& pp, const ort_tile& tt, int which) {
            return ort_debug_camera_query(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, ORT_LAYOUT_COMPACT,
                                          &pp, &tt, which, rays.data(), nullptr, nullptr);
        };
        check(gen(p0, tile, 0) == ORT_ERR_INVALID_ARG, "num_samples < 1");
        check(gen(p, outside, 0) == ORT_ERR_INVALID_ARG, "tile outside the frame");
        check(gen(p, tile, 2) == ORT_ERR_INVALID_ARG, "unknown which");
        for (float v : rays) check(v == 7.0f, "a refused call leaves the output untouched");
        check(gen(p, tile, 1) == ORT_OK, "pixel centre rays");
    }
    std::printf("san_camera: all cases passed\n");
    return 0;
}
