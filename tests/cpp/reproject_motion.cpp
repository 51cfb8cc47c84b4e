// tests/cpp/reproject_motion.cpp -- Raytracer::setHistoryMotion and moveSpheres on the prebuilt scene
// (96 x 64, 8 bounces) under a resting camera: over four steps the three large spheres (80, 81, 82 of
// getSpheres()) are moved -- 80 along x, 82 along y, 81 grows -- the scene is replaced by moveSpheres,
// and a one-sample linear picture (renderProgressive with moments, readMoments' mean) is blended into
// the history by reproject.  Prints per step
//   step <k> hash <FNV-1a of the integrated colour's and the variance's float bits>
// (tests/test_gpu_reproject_motion_cpp.py compares them with History.update(motion=True) on the same
// scenes and pictures), then
//   mse <last one-sample picture> <last integrated colour>   against the 64-sample linear mean of the
// last step's scene.
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

static const int kMoved[3] = {80, 81, 82};

// Where step k puts the three spheres, from where the scene has them at first.
static void placed(const std::vector<Sphere>& base, int k, float cr[12]) {
    for (int i = 0; i < 3; ++i) {
        const Sphere& s = base[(size_t)kMoved[i]];
        cr[4 * i] = s.center.x;
        cr[4 * i + 1] = s.center.y;
        cr[4 * i + 2] = s.center.z;
        cr[4 * i + 3] = s.radius;
    }
    cr[0] = cr[0] + 0.1f * (float)k;
    cr[7] = cr[7] * (1.0f + 0.02f * (float)k);
    cr[9] = cr[9] + 0.05f * (float)k;
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
    rt.setHistoryMotion(true);
    rt.camera = Camera(ortm::vec3(0.0f, 2.5f, -10.0f), ortm::vec3(0.0f, 1.0f, 0.0f), YAW, PITCH);
    rt.camera.Zoom = 45.0f;
    rtRef.camera = rt.camera;
    const ort_tile tile{0, (int32_t)cfg.width, 0, (int32_t)cfg.height, 0, 0};
    if (rt.moveSpheres(nullptr, nullptr, 0) != ORT_OK) {  // (builds the scene: getSpheres() is the first step's)
        std::fprintf(stderr, "scene failed: %s\n", rt.lastError());
        return 1;
    }
    const std::vector<Sphere> base = rt.getSpheres();
    if (base.size() != 83) {
        std::fprintf(stderr, "the prebuilt scene has %zu spheres\n", base.size());
        return 1;
    }
    float cr[12];
    for (int k = 0; k < 4; ++k) {
        placed(base, k, cr);
        int done = 0;
        int rc = rt.moveSpheres(kMoved, cr, 3);
        if (rc == ORT_OK) rc = rt.renderProgressive(rt.camera, 1, preview.data(), &done);
        if (rc == ORT_OK) rc = rt.readMoments(sample.data(), nullptr);
        if (rc == ORT_OK) rc = rt.reproject(rt.camera, tile, sample.data(), color.data(), variance.data());
        if (rc != ORT_OK) {
            std::fprintf(stderr, "step %d failed (%d): %s\n", k, rc, rt.lastError());
            return 1;
        }
        std::printf("step %d hash %016llx\n", k, (unsigned long long)fnv1a(fnv1a(1469598103934665603ull, color), variance));
    }
    int done = 0;
    if (rtRef.moveSpheres(kMoved, cr, 3) != ORT_OK || rtRef.renderProgressive(rtRef.camera, 64, preview.data(), &done) != ORT_OK ||
        rtRef.readMoments(ref.data(), nullptr) != ORT_OK) {
        std::fprintf(stderr, "reference failed: %s\n", rtRef.lastError());
        return 1;
    }
    std::printf("mse %.6f %.6f\n", mse(sample, ref), mse(color, ref));
    return 0;
}
