// tests/cpp/progressive.cpp -- Raytracer::renderProgressive against Raytracer::render on 100
// seeded spheres (64 x 48, 6 samples, 3 bounces): prints "step <name> rc done equals_render" lines
// that tests/test_gpu_accum_cpp.py reads.
//   same camera 3 x 2 samples      -> done 2, 4, 6; the last picture is render()'s
//   one more call when finished    -> done 6, render()'s picture again
//   a turned camera in between     -> the accumulation starts again: done 2, then 4, 6 = render(turned)
//   a zoomed camera                -> starts again as well
#include <cstdio>
#include <cstring>
#include <vector>

#include "raytracer.h"

int main() {
    RaytracerConfig cfg;
    cfg.numSpheres = 100;
    cfg.maxDepth = 4;
    cfg.numSamples = 6;
    cfg.maxRaysDepth = 3;
    cfg.width = 64;
    cfg.height = 48;
    Raytracer rt(cfg);
    const size_t n = (size_t)cfg.width * cfg.height * 3;
    std::vector<float> full(n), pic(n), fullTurned(n);
    Camera cam = rt.camera, turned = rt.camera, zoomed = rt.camera;
    turned.ProcessMouseMovement(4.0f, 1.0f);
    zoomed.ProcessMouseScroll(10.0f);
    if (rt.render(cam, full.data()) != ORT_OK || rt.render(turned, fullTurned.data()) != ORT_OK) {
        std::fprintf(stderr, "render failed: %s\n", rt.lastError());
        return 1;
    }
    if (std::memcmp(full.data(), fullTurned.data(), 4 * n) == 0) {
        std::fprintf(stderr, "the turned camera renders the same frame\n");
        return 1;
    }
    auto step = [&](const char* name, const Camera& c, int samples, const std::vector<float>& want) {
        int done = -1;
        const int rc = rt.renderProgressive(c, samples, pic.data(), &done);
        if (rc != ORT_OK) std::fprintf(stderr, "%s: renderProgressive failed (%d): %s\n", name, rc, rt.lastError());
        std::printf("step %s %d %d %d\n", name, rc, done, std::memcmp(pic.data(), want.data(), 4 * n) == 0 ? 1 : 0);
    };
    step("a1", cam, 2, full);
    step("a2", cam, 2, full);
    step("a3", cam, 2, full);
    step("a4", cam, 2, full);
    step("b1", turned, 2, fullTurned);
    step("c1", cam, 2, full);
    step("d1", turned, 2, fullTurned);
    step("d2", turned, 2, fullTurned);
    step("d3", turned, 5, fullTurned);
    step("e1", zoomed, 1, full);
    return 0;
}
