// tests/cpp/san_reproject_motion.cpp -- the moving-sphere reprojection's host code under
// AddressSanitizer + UBSan (CPU only, Makefile `san`): ort_debug_history_update_ex, the kernel's
// per-pixel function with motion (reproject.inc reproject_pixel<true>) compiled for the host, over a
// small seeded picture whose hit records name moved and unmoved spheres, misses and ids outside the
// scene (n, n + 5, INT_MAX, -1, -7, INT_MIN) -- a resting and a moved camera, with and without a
// snapshot, radii that make the scale infinite or NaN, a scene of no spheres -- with the sphere
// arrays in heap buffers of exactly n records, so that a read past them is reported.  History lengths
// must stay within 0 .. the updates made (and a few roundings); the state transitions (ort_debug_history_state) and the
// argument errors must come back as the header says, with nothing written.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "camera.h"
#include "ort_internal.h"

namespace {

void check(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "san_reproject_motion: FAILED %s (%s)\n", what, ort_last_error(nullptr));
        std::exit(1);
    }
}

uint32_t lcg = 2463534242u;
float u01() {
    lcg = lcg * 1664525u + 1013904223u;
    return (float)(lcg >> 8) / 16777216.0f;
}

ort_params frame_params(int W, int H, float px) {
    ort_params p;
    std::memset(&p, 0, sizeof p);
    p.width = W;
    p.height = H;
    p.num_samples = 1;
    p.max_depth = 1;
    p.use_octree = 1;
    Camera cam(ortm::vec3(px, 2.5f, -10.0f), ortm::vec3(0.0f, 1.0f, 0.0f), -90.0f, 0.0f);
    const ortm::mat4 v = cam.GetViewMatrix();
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) p.view[4 * c + r] = v[c][r];
    p.camera_position[0] = px;
    p.camera_position[1] = 2.5f;
    p.camera_position[2] = -10.0f;
    p.camera_zoom = 45.0f;
    return p;
}

}  // namespace

int main() {
    const int W = 37, H = 21, ROWS = 23, NS = 6;  // the tile's last two rows lie past the frame
    const size_t n = (size_t)W * ROWS;
    const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
    const ort_tile tile = {0, W, 0, ROWS, 0, 0};
    const ort_params cams[2] = {frame_params(W, H, 0.0f), frame_params(W, H, 0.2f)};
    const int32_t odd[6] = {NS, NS + 5, INT_MAX, -1, -7, INT_MIN};
    std::vector<float> pa(4 * n), pb(4 * n), na(4 * n), nb(4 * n);
    int calls = 0;
    for (int k = 0; k < 7; ++k) {
        const ort_params& p = cams[k == 3 || k == 4 ? 1 : 0];  // k = 1, 2, 4, 6: the camera rests bitwise
        const ort_params& prev = cams[k == 4 || k == 5 ? 1 : 0];
        const ort::CameraFrame c = ort::cameraFrameFromView(p.view, p.camera_position, p.camera_zoom, (float)W / (float)H);
        std::vector<float> color(3 * n);
        std::vector<ort_ray> rays(n);
        std::vector<ort_ray_hit> hits(n);
        for (int y = 0; y < ROWS; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = (size_t)y * W + x;
                for (int q = 0; q < 3; ++q) color[3 * i + q] = u01();
                const float a = ((float)x + 0.5f) / (float)W, b = ((float)y + 0.5f) / (float)H;
                float d[3], len = 0.0f;
                for (int q = 0; q < 3; ++q) {
                    d[q] = c.lowerLeft[q] + a * c.horizontal[q] + b * c.vertical[q] - c.origin[q];
                    len += d[q] * d[q];
                }
                len = std::sqrt(len);
                for (int q = 0; q < 3; ++q) {
                    rays[i].origin[q] = c.origin[q];
                    rays[i].direction[q] = d[q] / len;
                }
                const int32_t id = x < 30 ? (x / 5) % NS : -1;  // columns of spheres 0 .. 5, then the sky
                hits[i] = {id >= 0 ? 8.0f + 0.01f * (float)y : 0.0f, id};
            }
        for (int q = 0; q < 6; ++q) hits[(size_t)(2 + q) * W + 3 * q + 1].sphere = odd[q];
        // the spheres: exactly NS records each (k = 6: none at all); 1 and 4 move, 2 changes its radius,
        // 3 and 5 get radii that make the scale infinite and NaN
        const int ns = k == 6 ? 0 : NS;
        std::vector<float> now(4 * (size_t)ns), snap(4 * (size_t)ns);
        for (int s = 0; s < ns; ++s) {
            const float base[4] = {-3.0f + 1.2f * (float)s, 2.5f, -2.0f, 0.6f};
            for (int q = 0; q < 4; ++q) now[4 * s + q] = snap[4 * s + q] = base[q];
        }
        if (ns) {
            now[4 * 1 + 0] += 0.1f * (float)k;
            now[4 * 4 + 1] -= 0.05f * (float)k;
            now[4 * 2 + 3] *= 1.1f;
            now[4 * 3 + 3] = 0.0f;
            now[4 * 5 + 3] = k & 1 ? kNan : 0.0f;
            snap[4 * 5 + 3] = k & 1 ? 1.0f : 0.0f;
        }
        const bool with_snap = k != 2;
        std::vector<float> col(3 * n, -3.0f), var(n, -3.0f), len(n, -3.0f);
        ort_history_frame_ex f;
        std::memset(&f, 0, sizeof f);
        f.base.params = &p;
        f.base.tile = &tile;
        f.base.color = color.data();
        f.base.rays = rays.data();
        f.base.hits = hits.data();
        f.base.out_color = col.data();
        f.base.out_variance = var.data();
        f.base.out_length = len.data();
        f.base.alpha = 0.2f;
        f.base.depth_tolerance = k & 1 ? 0.1f : 0.0f;
        f.base.flags = ORT_HISTORY_MOTION;
        static const float none[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // (a scene of no spheres still has an address)
        check(ort_debug_history_update_ex(k ? &prev : nullptr, 0, 0, pa.data(), pb.data(), &f, ns ? now.data() : none,
                                          with_snap && ns ? snap.data() : nullptr, ns, na.data(), nb.data()) == ORT_OK,
              "a MOTION update");
        ++calls;
        for (size_t i = 0; i < n; ++i) {
            // (the taps' weighted mean of equal lengths is that length within its few roundings)
            check(len[i] >= 0.0f && len[i] <= (float)(k + 1) * (1.0f + 1e-6f), "a history length within the updates made");
            check(std::isfinite(col[3 * i]) && (var[i] == -1.0f || var[i] >= 0.0f), "finite outputs");
        }
        if (k == 1)  // the resting camera: a moved sphere's pixels were projected, the others took their own record
            check(len[(size_t)4 * W + 0] == 2.0f && len[(size_t)4 * W + 33] == 2.0f, "unmoved pixels keep their record");
        // the refusals: nothing written
        std::vector<float> na2(4 * n, -3.0f), nb2(4 * n, -3.0f);
        std::fill(col.begin(), col.end(), -3.0f);
        ort_history_frame_ex g = f;
        g.base.flags = 2;
        check(ort_debug_history_update_ex(&prev, 0, 0, pa.data(), pb.data(), &g, now.data(), snap.data(), ns, na2.data(),
                                          nb2.data()) == ORT_ERR_INVALID_ARG, "an unknown flag is refused");
        g = f;
        g.reserved[k % 4] = 1;
        check(ort_debug_history_update_ex(&prev, 0, 0, pa.data(), pb.data(), &g, now.data(), snap.data(), ns, na2.data(),
                                          nb2.data()) == ORT_ERR_INVALID_ARG, "reserved is refused");
        check(ort_debug_history_update_ex(&prev, 0, 0, pa.data(), pb.data(), &f, nullptr, nullptr, ns, na2.data(),
                                          nb2.data()) == ORT_ERR_NO_SCENE, "MOTION without a scene");
        check(ort_debug_history_update(&prev, 0, 0, pa.data(), pb.data(), &f.base, na2.data(), nb2.data()) == ORT_ERR_INVALID_ARG,
              "the plain call refuses the flag");
        for (size_t i = 0; i < 4 * n; ++i) check(na2[i] == -3.0f && nb2[i] == -3.0f, "a refusal writes no record");
        for (size_t i = 0; i < 3 * n; ++i) check(col[i] == -3.0f, "a refusal writes no output");
        pa = na;
        pb = nb;
    }
    // the state transitions: upload, MOTION, upload, upload, MOTION (revived), upload of another count, MOTION
    int64_t st[6] = {0, 0, 0, 0, 0, 0};
    int32_t reads = -1;
    const int ops[7] = {0, 3, 0, 0, 3, 0, 3}, counts[7] = {0, 6, 0, 0, 6, 0, 5};
    const int64_t updates[7] = {0, 1, 0, 0, 2, 0, 1};
    const int32_t read[7] = {0, 0, 0, 0, 1, 0, 0};
    for (int i = 0; i < 7; ++i) {
        check(ort_debug_history_state(st, ops[i], counts[i], &reads) == ORT_OK, "a state transition");
        check(st[0] == updates[i] && reads == read[i], "the updates value and the snapshot's use");
    }
    check(ort_debug_history_state(st, 4, 0, nullptr) == ORT_ERR_INVALID_ARG, "an unknown op is refused");
    check(ort_debug_history_state(nullptr, 0, 0, nullptr) == ORT_ERR_INVALID_ARG, "a null state is refused");
    std::printf("san_reproject_motion: ok (%d updates)\n", calls);
    return 0;
}
