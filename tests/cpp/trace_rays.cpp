// tests/cpp/trace_rays.cpp -- Raytracer::traceRays on the DEBUG scene: prints, for a few fixed
// rays, one line "ray i hit sphere t-bits nx-bits ny-bits nz-bits" (hex float bits; the DEBUG
// build's own chatter goes to the same stream), which
// tests/test_gpu_ray_query.py compares with Renderer.trace_rays on the same scene.
//   trace_rays [--brute]
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
    // from the DEBUG view's position (30, 20, -50): a 3 x 3 fan around the centre of each of the
    // scene's three spheres (radius 3: centre and edge rays hit, corner rays pass by), two rays
    // that look away, one straight down an axis from above
    const float centres[3][3] = {{-10.0f, -10.0f, -10.0f}, {10.0f, 10.0f, 10.0f}, {-10.0f, 10.0f, -10.0f}};
    std::vector<ort_ray> rays;
    for (int k = 0; k < 3; ++k)
        for (int j = -1; j <= 1; ++j)
            for (int i = -1; i <= 1; ++i)
                rays.push_back({{30.0f, 20.0f, -50.0f},
                                {(centres[k][0] + 2.5f * (float)i) - 30.0f, (centres[k][1] + 2.5f * (float)j) - 20.0f,
                                 centres[k][2] + 50.0f}});
    rays.push_back({{30.0f, 20.0f, -50.0f}, {0.0f, 0.0f, -1.0f}});
    rays.push_back({{30.0f, 20.0f, -50.0f}, {0.0f, 1.0f, 0.0f}});
    rays.push_back({{10.0f, 50.0f, 10.0f}, {0.0f, -1.0f, 0.0f}});
    std::vector<ort_ray_hit> hits(rays.size());
    std::vector<float> normals(3 * rays.size());
    const int rc = rt.traceRays(rays.data(), (int64_t)rays.size(), hits.data(), normals.data());
    if (rc != ORT_OK) {
        std::fprintf(stderr, "traceRays failed (%d): %s\n", rc, rt.lastError());
        return 1;
    }
    for (size_t i = 0; i < rays.size(); ++i)
        std::printf("ray %zu %d %d %08x %08x %08x %08x\n", i, hits[i].sphere >= 0 ? 1 : 0, hits[i].sphere, bits(hits[i].t),
                    bits(normals[3 * i]), bits(normals[3 * i + 1]), bits(normals[3 * i + 2]));
    return 0;
}
