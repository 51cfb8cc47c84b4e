// tests/cpp/denoise.cpp -- Raytracer::denoise on the prebuilt scene (96 x 64, 8 bounces): one sample
// accumulated (renderProgressive), then denoised with the library's defaults.  Prints
//   hash <FNV-1a of the filtered picture's float bits>   (tests/test_gpu_denoise_cpp.py compares it
//                                                          with Renderer.denoise on the same frame)
//   mse <before> <after>                                   against the 64-sample frame
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "raytracer.h"

static double mse(const std::vector<float>& a, const std::vector<float>& b) {
    double s = 0.0;
    for (size_t i = 0; i < a.size(); ++i) s += ((double)a[i] - b[i]) * ((double)a[i] - b[i]);
    return s / (double)a.size();
}

int main() {
    RaytracerConfig cfg;
    cfg.usePrebuilt = 1;
    cfg.width = 96;
    cfg.height = 64;
    cfg.numSamples = 1;
    cfg.maxRaysDepth = 8;
    RaytracerConfig many = cfg;
    many.numSamples = 64;
    const size_t n = (size_t)cfg.width * cfg.height * 3;
    std::vector<float> noisy(n), filtered(n), ref(n);
    Raytracer rt(cfg), rtRef(many);
    if (rtRef.render(rtRef.camera, ref.data()) != ORT_OK) {
        std::fprintf(stderr, "render failed: %s\n", rtRef.lastError());
        return 1;
    }
    int done = 0;
    if (rt.renderProgressive(rt.camera, 1, noisy.data(), &done) != ORT_OK || done != 1) {
        std::fprintf(stderr, "renderProgressive failed: %s\n", rt.lastError());
        return 1;
    }
    const ort_tile tile{0, (int32_t)cfg.width, 0, (int32_t)cfg.height, 0, 0};
    const ort_output out = {filtered.data(), 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
    const int rc = rt.denoise(rt.camera, tile, noisy.data(), out);
    if (rc != ORT_OK) {
        std::fprintf(stderr, "denoise failed (%d): %s\n", rc, rt.lastError());
        return 1;
    }
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) {
        uint32_t u;
        std::memcpy(&u, &filtered[i], 4);
        for (int k = 0; k < 4; ++k) {
            h ^= (u >> (8 * k)) & 0xffu;
            h *= 1099511628211ull;
        }
    }
    std::printf("hash %016llx\n", (unsigned long long)h);
    std::printf("mse %.6f %.6f\n", mse(noisy, ref), mse(filtered, ref));
    return 0;
}
