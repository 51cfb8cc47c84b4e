// tests/cpp/radiance_probe.cpp -- Raytracer::traceRadiance on the prebuilt scene: a light probe at
// one point, the six axis directions, 64 paths of at most 8 bounces each.  Prints one line per ray
// "probe i" + 13 hex float bits: the ray (origin, direction), the RNG state it started from, the
// radiance, the state it ended with -- which tests/test_gpu_radiance_cpp.py compares with
// Renderer.trace_radiance on the same scene, rays and states -- and the mean over the six.
//   radiance_probe [--brute]
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
    cfg.usePrebuilt = 1;
    cfg.useOctree = (argc > 1 && std::strcmp(argv[1], "--brute") == 0) ? 0 : 1;
    Raytracer rt(cfg);
    const float at[3] = {2.0f, 1.0f, 0.0f};  // between two of the three large spheres, above the small ones
    std::vector<ort_ray> rays;
    std::vector<float> states;
    for (int axis = 0; axis < 3; ++axis)
        for (int sign = 0; sign < 2; ++sign) {
            ort_ray r = {{at[0], at[1], at[2]}, {0.0f, 0.0f, 0.0f}};
            r.direction[axis] = sign ? -1.0f : 1.0f;
            rays.push_back(r);
            const float i = (float)rays.size();  // one chain per ray: states exact in float32, in [0, 1)
            states.push_back(i * 0.125f);
            states.push_back(0.9375f - i * 0.0625f);
        }
    const int64_t n = (int64_t)rays.size();
    std::vector<float> radiance(3 * rays.size()), ends(2 * rays.size());
    const int rc = rt.traceRadiance(rays.data(), states.data(), n, 8, 64, radiance.data(), ends.data());
    if (rc != ORT_OK) {
        std::fprintf(stderr, "traceRadiance failed (%d): %s\n", rc, rt.lastError());
        return 1;
    }
    float mean[3] = {0.0f, 0.0f, 0.0f};
    for (int64_t i = 0; i < n; ++i) {
        const ort_ray& r = rays[(size_t)i];
        std::printf("probe %lld %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", (long long)i, bits(r.origin[0]),
                    bits(r.origin[1]), bits(r.origin[2]), bits(r.direction[0]), bits(r.direction[1]), bits(r.direction[2]),
                    bits(states[2 * i]), bits(states[2 * i + 1]), bits(radiance[3 * i]), bits(radiance[3 * i + 1]),
                    bits(radiance[3 * i + 2]), bits(ends[2 * i]), bits(ends[2 * i + 1]));
        for (int k = 0; k < 3; ++k) mean[k] += radiance[3 * i + k] / (float)n;
    }
    std::printf("mean %.4f %.4f %.4f\n", mean[0], mean[1], mean[2]);
    return 0;
}
