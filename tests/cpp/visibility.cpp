// tests/cpp/visibility.cpp -- Raytracer::occluded and Raytracer::traceRays in the query modes on
// the DEBUG scene: prints, for a few fixed segments, one line "pair i occluded" and, for the rays
// from each segment's start towards its end, one line "nearest i sphere t-bits" (hex float bits;
// the DEBUG build's own chatter goes to the same stream), which tests/test_gpu_ray_modes.py
// compares with Renderer.occluded and Renderer.trace_rays(mode="nearest") on the same scene.
//   visibility [--brute]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "raytracer.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    RaytracerConfig cfg;
    cfg.debug = 1;
    cfg.useOctree = (argc > 1 && std::strcmp(argv[1], "--brute") == 0) ? 0 : 1;
    Raytracer rt(cfg);
    // the scene's three spheres have radius 3 and the centres below: from the DEBUG view's position
    // to each centre's far side (occluded), to a point short of it (visible), past its edge
    // (visible), between two spheres through the third's neighbourhood, and a pair of coincident
    // points
    const float eye[3] = {30.0f, 20.0f, -50.0f};
    const float centres[3][3] = {{-10.0f, -10.0f, -10.0f}, {10.0f, 10.0f, 10.0f}, {-10.0f, 10.0f, -10.0f}};
    std::vector<float> a, b;
    auto pair = [&](const float* p, float qx, float qy, float qz) {
        a.insert(a.end(), p, p + 3);
        b.push_back(qx);
        b.push_back(qy);
        b.push_back(qz);
    };
    for (int k = 0; k < 3; ++k) {
        const float* c = centres[k];
        pair(eye, c[0] + (c[0] - eye[0]) * 0.25f, c[1] + (c[1] - eye[1]) * 0.25f, c[2] + (c[2] - eye[2]) * 0.25f);
        pair(eye, eye[0] + (c[0] - eye[0]) * 0.5f, eye[1] + (c[1] - eye[1]) * 0.5f, eye[2] + (c[2] - eye[2]) * 0.5f);
        pair(eye, c[0] + 4.5f, c[1] + 4.5f, c[2]);
        pair(c, c[0], c[1] + 10.0f, c[2]);  // from inside the sphere out: its far root lies between
    }
    pair(centres[0], centres[2][0], centres[2][1], centres[2][2]);  // centre to centre, both surfaces between
    pair(eye, eye[0], eye[1], eye[2]);                              // coincident: not occluded
    const int64_t n = (int64_t)(a.size() / 3);
    std::vector<uint8_t> occ((size_t)n);
    int rc = rt.occluded(a.data(), b.data(), n, occ.data());
    if (rc != ORT_OK) {
        std::fprintf(stderr, "occluded failed (%d): %s\n", rc, rt.lastError());
        return 1;
    }
    for (int64_t i = 0; i < n; ++i) std::printf("pair %lld %d\n", (long long)i, (int)occ[(size_t)i]);
    // the nearest hit along b - a inside (0, 1): t in units of the segment
    std::vector<ort_ray> rays((size_t)n);
    std::vector<float> range(2 * (size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        rays[(size_t)i] = {{a[3 * i], a[3 * i + 1], a[3 * i + 2]}, {b[3 * i] - a[3 * i], b[3 * i + 1] - a[3 * i + 1], b[3 * i + 2] - a[3 * i + 2]}};
        range[2 * (size_t)i] = 0.0f;
        range[2 * (size_t)i + 1] = 1.0f;
    }
    std::vector<ort_ray_hit> hits((size_t)n);
    rc = rt.traceRays(rays.data(), n, hits.data(), nullptr, ORT_QUERY_NEAREST, range.data());
    if (rc != ORT_OK) {
        std::fprintf(stderr, "traceRays failed (%d): %s\n", rc, rt.lastError());
        return 1;
    }
    for (int64_t i = 0; i < n; ++i) std::printf("nearest %lld %d %08x\n", (long long)i, hits[(size_t)i].sphere, bits(hits[(size_t)i].t));
    return 0;
}
