// tests/cpp/denoise_variance.cpp -- the camera at rest, through Raytracer: the prebuilt scene (96 x 64,
// 8 bounces, 16 samples a pixel) refined in passes of 1, 1, 2 and 4 samples with the moments kept; after
// each pass from 2 samples on, the mean and its variance read back and a variance-guided denoise with
// gamma.  Prints, per such pass,
//   pass <samples done> hash <FNV-1a of the filtered picture's float bits> mse <preview> <filtered>
// (tests/test_gpu_variance_cpp.py compares the hashes with the Python path's; the errors are
// against the 256-sample frame).
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

static uint64_t fnv1a(const std::vector<float>& v) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < v.size(); ++i) {
        uint32_t u;
        std::memcpy(&u, &v[i], 4);
        for (int k = 0; k < 4; ++k) {
            h ^= (u >> (8 * k)) & 0xffu;
            h *= 1099511628211ull;
        }
    }
    return h;
}

int main() {
    RaytracerConfig cfg;
    cfg.usePrebuilt = 1;
    cfg.width = 96;
    cfg.height = 64;
    cfg.numSamples = 16;
    cfg.maxRaysDepth = 8;
    RaytracerConfig many = cfg;
    many.numSamples = 256;
    const size_t px = (size_t)cfg.width * cfg.height;
    std::vector<float> preview(3 * px), mean(3 * px), variance(px), filtered(3 * px), ref(3 * px);
    Raytracer rt(cfg), rtRef(many);
    if (rtRef.render(rtRef.camera, ref.data()) != ORT_OK) {
        std::fprintf(stderr, "render failed: %s\n", rtRef.lastError());
        return 1;
    }
    rt.setProgressiveMoments(true);
    const ort_tile tile{0, (int32_t)cfg.width, 0, (int32_t)cfg.height, 0, 0};
    const ort_output out = {filtered.data(), 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
    const int passes[] = {1, 1, 2, 4};
    for (int n : passes) {
        int done = 0;
        if (rt.renderProgressive(rt.camera, n, preview.data(), &done) != ORT_OK) {
            std::fprintf(stderr, "renderProgressive failed: %s\n", rt.lastError());
            return 1;
        }
        if (done < 2) continue;
        int rc = rt.readMoments(mean.data(), variance.data());
        if (rc == ORT_OK) rc = rt.denoise(rt.camera, tile, mean.data(), variance.data(), 4.0f, true, out);
        if (rc != ORT_OK) {
            std::fprintf(stderr, "moments or denoise failed (%d): %s\n", rc, rt.lastError());
            return 1;
        }
        std::printf("pass %d hash %016llx mse %.6f %.6f\n", done, (unsigned long long)fnv1a(filtered), mse(preview, ref),
                    mse(filtered, ref));
    }
    return 0;
}
