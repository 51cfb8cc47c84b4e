// tests/cpp/adaptive.cpp -- the camera at rest with adaptive sampling, through Raytracer: the prebuilt
// scene (96 x 64, 8 bounces, 16 samples a pixel) refined in adaptive passes of one sample (threshold
// 0.05, at least 4 samples, luminance floor 0.05) until no pixel is pending.  Prints, per pass,
//   pass <i> pending <pixels the pass traced> done <samples_done>
// and at the end
//   end passes <n> samples <sum of the counts> counts <hash> mean <hash> variance <hash> preview <hash>
// with FNV-1a hashes of the arrays' bytes (tests/test_gpu_adaptive_cpp.py compares them with the
// Python path's).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "raytracer.h"

static uint64_t fnv1a(const void* data, size_t bytes) {
    const unsigned char* b = (const unsigned char*)data;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
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
    const size_t px = (size_t)cfg.width * cfg.height;
    std::vector<float> preview(3 * px), mean(3 * px), variance(px);
    std::vector<int32_t> counts(px);
    Raytracer rt(cfg);
    rt.setProgressiveAdaptive(true, 0.05f, 4, 0.05f);
    if (rt.pendingPixels() != -1) {
        std::fprintf(stderr, "pendingPixels before the first pass must be -1\n");
        return 1;
    }
    int passes = 0;
    for (long long pending = (long long)px; pending != 0; pending = rt.pendingPixels()) {
        int done = 0;
        if (pending < 0 || passes > cfg.numSamples || rt.renderProgressive(rt.camera, 1, preview.data(), &done) != ORT_OK) {
            std::fprintf(stderr, "the rest loop failed at pass %d: %s\n", passes, rt.lastError());
            return 1;
        }
        std::printf("pass %d pending %lld done %d\n", passes, pending, done);
        ++passes;
    }
    int rc = rt.readSampleCounts(counts.data());
    if (rc == ORT_OK) rc = rt.readMoments(mean.data(), variance.data());
    if (rc != ORT_OK) {
        std::fprintf(stderr, "counts or moments failed (%d): %s\n", rc, rt.lastError());
        return 1;
    }
    long long samples = 0;
    for (int32_t c : counts) samples += c;
    std::printf("end passes %d samples %lld counts %016llx mean %016llx variance %016llx preview %016llx\n", passes, samples,
                (unsigned long long)fnv1a(counts.data(), 4 * px), (unsigned long long)fnv1a(mean.data(), 12 * px),
                (unsigned long long)fnv1a(variance.data(), 4 * px), (unsigned long long)fnv1a(preview.data(), 12 * px));
    return 0;
}
