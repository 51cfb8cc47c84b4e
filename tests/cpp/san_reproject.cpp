// tests/cpp/san_reproject.cpp -- temporal reprojection's host code under AddressSanitizer + UBSan
// (CPU only, Makefile `san`): ort_debug_history_update, the kernel's per-pixel function (reproject.inc
// reproject_pixel) compiled for the host, over a small seeded picture with hits, misses, non-finite
// samples and non-finite rays and distances -- five cameras (a first frame, a translation, a rotation
// with a zoom change, the same camera again, a jump), a colour pitch, outputs partly NULL, a tile
// reaching past the frame -- in buffers of exactly the bytes the frame covers, so that a read or
// write past them is reported.  Records and outputs must be finite where the samples are, history
// lengths within 0 .. the updates made; the argument errors must come back as codes with nothing
// written.
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
        std::fprintf(stderr, "san_reproject: FAILED %s (%s)\n", what, ort_last_error(nullptr));
        std::exit(1);
    }
}

uint32_t lcg = 2463534242u;
float u01() {
    lcg = lcg * 1664525u + 1013904223u;
    return (float)(lcg >> 8) / 16777216.0f;
}

ort_params frame_params(int W, int H, float px, float yaw, float zoom) {
    ort_params p;
    std::memset(&p, 0, sizeof p);
    p.width = W;
    p.height = H;
    p.num_samples = 1;
    p.max_depth = 1;
    p.use_octree = 1;
    Camera cam(ortm::vec3(px, 2.5f, -10.0f), ortm::vec3(0.0f, 1.0f, 0.0f), yaw, 0.0f);
    const ortm::mat4 v = cam.GetViewMatrix();
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) p.view[4 * c + r] = v[c][r];
    p.camera_position[0] = px;
    p.camera_position[1] = 2.5f;
    p.camera_position[2] = -10.0f;
    p.camera_zoom = zoom;
    return p;
}

}  // namespace

int main() {
    const int W = 37, H = 21, ROWS = 24;  // the tile's last three rows lie past the frame
    const size_t n = (size_t)W * ROWS;
    const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
    const ort_tile tile = {0, W, 0, ROWS, 0, 0};
    const ort_params cams[5] = {frame_params(W, H, 0.0f, -90.0f, 45.0f), frame_params(W, H, 0.3f, -90.0f, 45.0f),
                                frame_params(W, H, 0.3f, -87.0f, 49.0f), frame_params(W, H, 0.3f, -87.0f, 49.0f),
                                frame_params(W, H, 0.3f, 60.0f, 49.0f)};
    std::vector<float> pa(4 * n), pb(4 * n), na(4 * n), nb(4 * n);
    int calls = 0;
    for (int k = 0; k < 5; ++k) {
        const ort_params& p = cams[k];
        const ort::CameraFrame c = ort::cameraFrameFromView(p.view, p.camera_position, p.camera_zoom, (float)W / (float)H);
        const bool pitched = k & 1;
        const size_t pitch = pitched ? 12 * (size_t)W + 20 : 12 * (size_t)W;
        std::vector<unsigned char> color(pitch * (ROWS - 1) + 12 * (size_t)W);
        std::vector<ort_ray> rays(n);
        std::vector<ort_ray_hit> hits(n);
        for (int y = 0; y < ROWS; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = (size_t)y * W + x;
                float* s = reinterpret_cast<float*>(color.data() + y * pitch) + 3 * x;
                for (int q = 0; q < 3; ++q) s[q] = u01();
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
                const bool disc = (x - 12) * (x - 12) + (y - 10) * (y - 10) < 50, band = x > 25 && y > 4;
                hits[i] = {disc || band ? 8.0f + u01() : 0.0f, disc ? 3 : (band ? 5 : -1)};
            }
        // non-finite samples, a non-finite distance and a non-finite ray
        reinterpret_cast<float*>(color.data())[0] = kNan;
        reinterpret_cast<float*>(color.data() + 10 * pitch)[3 * 12 + 1] = kInf;
        hits[(size_t)10 * W + 13].t = kNan;
        hits[(size_t)11 * W + 13].t = kInf;
        rays[(size_t)12 * W + 13].direction[0] = kNan;
        rays[(size_t)5 * W + 30].origin[1] = -kInf;
        std::vector<float> col(k == 2 ? 0 : 3 * n, -3.0f), var(k == 3 ? 0 : n, -3.0f), len(k == 4 ? 0 : n, -3.0f);
        ort_history_frame f;
        std::memset(&f, 0, sizeof f);
        f.params = &p;
        f.tile = &tile;
        f.color = reinterpret_cast<const float*>(color.data());
        f.color_pitch_bytes = pitched ? (int64_t)pitch : 0;
        f.rays = rays.data();
        f.hits = hits.data();
        f.out_color = col.empty() ? nullptr : col.data();
        f.out_variance = var.empty() ? nullptr : var.data();
        f.out_length = len.empty() ? nullptr : len.data();
        f.alpha = k == 3 ? 0.0f : 0.2f;
        f.depth_tolerance = (k & 1) ? 0.1f : 0.0f;
        check(ort_debug_history_update(k ? &cams[k - 1] : nullptr, 0, 0, pa.data(), pb.data(), &f, na.data(), nb.data()) == ORT_OK,
              "ort_debug_history_update");
        ++calls;
        for (size_t i = 0; i < n; ++i) {
            const bool padding = i >= (size_t)W * H;
            const float cnt = na[4 * i + 3];
            check(cnt >= 0.0f && cnt <= (float)(k + 1), "history length within the updates made");
            if (padding) check(cnt == 0.0f && na[4 * i] == 0.0f, "a row past the frame holds zeros");
            for (int q = 0; q < 3; ++q) check(std::isfinite(na[4 * i + q]), "a finite integrated colour");
            if (!col.empty()) check(std::memcmp(&col[3 * i], &na[4 * i], 12) == 0, "out_color is the record's colour");
            if (!len.empty()) check(len[i] == cnt, "out_length is the record's n");
            if (!var.empty()) check(var[i] == -1.0f || (std::isfinite(var[i]) && var[i] >= 0.0f), "a variance or -1");
        }
        if (k == 3)  // the same camera: every pixel inside the frame with a finite sample grew by one
            check(na[4 * ((size_t)3 * W + 3) + 3] == pa[4 * ((size_t)3 * W + 3) + 3] + 1.0f, "the same camera keeps its history");
        pa.swap(na);
        pb.swap(nb);
    }
    // refusals: codes, nothing written
    const ort_params& p = cams[0];
    std::vector<float> color(3 * n, 0.5f), out(3 * n, -3.0f);
    std::vector<ort_ray> rays(n);
    std::vector<ort_ray_hit> hits(n);
    std::vector<float> keep_a(na), keep_b(nb);
    ort_history_frame f;
    std::memset(&f, 0, sizeof f);
    f.params = &p;
    f.tile = &tile;
    f.color = color.data();
    f.rays = rays.data();
    f.hits = hits.data();
    f.out_color = out.data();
    f.alpha = 0.2f;
    const auto refused = [&](const ort_history_frame& e, const char* what) {
        check(ort_debug_history_update(&p, 0, 0, pa.data(), pb.data(), &e, na.data(), nb.data()) == ORT_ERR_INVALID_ARG, what);
    };
    ort_history_frame e = f;
    e.alpha = 1.5f;
    refused(e, "alpha above 1 refused");
    e.alpha = kNan;
    refused(e, "NaN alpha refused");
    e = f;
    e.depth_tolerance = -0.1f;
    refused(e, "negative depth_tolerance refused");
    e = f;
    e.flags = 1;
    refused(e, "flags refused");
    e = f;
    e.reserved[3] = 1;
    refused(e, "reserved refused");
    e = f;
    e.color_pitch_bytes = 12 * W - 4;
    refused(e, "short colour pitch refused");
    e = f;
    e.color = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(color.data()) + 2);
    refused(e, "misaligned colour refused");
    e = f;
    e.rays = nullptr;
    refused(e, "null rays refused");
    e = f;
    e.params = nullptr;
    refused(e, "null params refused");
    const ort_tile banded = {0, W, 0, ROWS, 8, 16};
    e = f;
    e.tile = &banded;
    refused(e, "banded tile refused");
    const ort_tile wide = {0, W + 1, 0, ROWS, 0, 0};
    e = f;
    e.tile = &wide;
    refused(e, "a tile wider than the frame refused");
    ort_params zero = p;
    zero.num_samples = 0;
    e = f;
    e.params = &zero;
    refused(e, "params ort_render refuses are refused");
    check(ort_debug_history_update(&p, 0, 0, pa.data(), pb.data(), nullptr, na.data(), nb.data()) == ORT_ERR_INVALID_ARG, "null frame refused");
    for (float v : out) check(v == -3.0f, "a refused call writes no output");
    check(std::memcmp(na.data(), keep_a.data(), 16 * n) == 0 && std::memcmp(nb.data(), keep_b.data(), 16 * n) == 0,
          "a refused call writes no record");
    const ort_tile none = {0, 0, 0, ROWS, 0, 0};
    e = f;
    e.tile = &none;
    e.color = nullptr;
    e.rays = nullptr;
    e.hits = nullptr;
    check(ort_debug_history_update(nullptr, 0, 0, nullptr, nullptr, &e, nullptr, nullptr) == ORT_OK, "a history of no pixels is ORT_OK");
    std::printf("san_reproject: %d updates of %d x %d, refusals and the empty history: ok\n", calls, W, ROWS);
    return 0;
}
