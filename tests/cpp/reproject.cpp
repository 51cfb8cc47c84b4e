// tests/cpp/reproject.cpp -- Raytracer::reproject on the prebuilt scene (96 x 64, 8 bounces): a camera
// moved over four poses -- the start, a step sideways, a turn with a zoom change, another step -- and
// at each one a one-sample linear picture (renderProgressive with moments, readMoments' mean) blended
// into the history.  Prints per pose
//   pose <k> hash <FNV-1a of the integrated colour's and the variance's float bits>
// (tests/test_gpu_reproject_cpp.py compares them with History.update on the same pictures), then
//   mse <last one-sample picture> <last integrated colour>   against the 64-sample linear mean.
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

static uint64_t fnv1a(uint64_t h, const std::vector<float>& v) {
    for (float f : v) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        for (int k = 0; k < 4; ++k) {
            h ^= (u >> (8 * k)) & 0xffu;
            h *= 1099511628211ull;
        }
    }
    return h;
}

static void pose(Camera& cam, int k) {
    const float dx[4] = {0.0f, 0.05f, 0.05f, 0.1f}, yaw[4] = {0.0f, 0.0f, 2.0f, 2.0f}, zoom[4] = {45.0f, 45.0f, 47.0f, 47.0f};
    cam = Camera(ortm::vec3(0.0f + dx[k], 2.5f, -10.0f), ortm::vec3(0.0f, 1.0f, 0.0f), YAW + yaw[k], PITCH);
    cam.Zoom = zoom[k];
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
    const size_t px = (size_t)cfg.width * cfg.height;
    std::vector<float> preview(3 * px), sample(3 * px), color(3 * px), variance(px), ref(3 * px);
    Raytracer rt(cfg), rtRef(many);
    rt.setProgressiveMoments(true);
    rtRef.setProgressiveMoments(true);
    const ort_tile tile{0, (int32_t)cfg.width, 0, (int32_t)cfg.height, 0, 0};
    for (int k = 0; k < 4; ++k) {
        pose(rt.camera, k);
        int done = 0;
        int rc = rt.renderProgressive(rt.camera, 1, preview.data(), &done);
        if (rc == ORT_OK) rc = rt.readMoments(sample.data(), nullptr);
        if (rc == ORT_OK) rc = rt.reproject(rt.camera, tile, sample.data(), color.data(), variance.data());
        if (rc != ORT_OK) {
            std::fprintf(stderr, "pose %d failed (%d): %s\n", k, rc, rt.lastError());
            return 1;
        }
        std::printf("pose %d hash %016llx\n", k, (unsigned long long)fnv1a(fnv1a(1469598103934665603ull, color), variance));
    }
    pose(rtRef.camera, 3);
    int done = 0;
    if (rtRef.renderProgressive(rtRef.camera, 64, preview.data(), &done) != ORT_OK || rtRef.readMoments(ref.data(), nullptr) != ORT_OK) {
        std::fprintf(stderr, "reference failed: %s\n", rtRef.lastError());
        return 1;
    }
    std::printf("mse %.6f %.6f\n", mse(sample, ref), mse(color, ref));
    return 0;
}
