// tests/cpp/san_denoise_var.cpp -- the host code of variance-guided denoising under AddressSanitizer
// + UBSan (CPU only, Makefile `san`): ort_debug_denoise_ex (the prefilter, denoise_pixel<true>, the
// gamma) over a small seeded image with a variance plane that holds zeros, -1, +inf, NaN and a huge
// value -- every iteration count, both formats, pitches, in place -- ort_debug_gamma, and
// ort_debug_emulate_moments on the debug scene at every sample count, a band tile past the frame among
// them, all in buffers of exactly the bytes the call covers.  The argument errors must come back as
// codes with nothing written.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ort_internal.h"

namespace {

void check(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "san_denoise_var: FAILED %s (%s)\n", what, ort_last_error(nullptr));
        std::exit(1);
    }
}

uint32_t lcg = 2463534242u;
float u01() {
    lcg = lcg * 1664525u + 1013904223u;
    return (float)(lcg >> 8) / 16777216.0f;
}

}  // namespace

int main() {
    const int W = 37, H = 21;
    const size_t n = (size_t)W * H;
    const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
    std::vector<ort_ray_hit> hits(n);
    std::vector<float> normals(3 * n), tight(3 * n), variance(n);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const bool disc = (x - 12) * (x - 12) + (y - 10) * (y - 10) < 50, band = x > 25 && y > 4;
            hits[i] = {disc || band ? 2.0f + u01() : 0.0f, disc ? 3 : (band ? 5 : -1)};
            float v[3] = {u01() - 0.5f, u01() - 0.5f, u01() + 0.1f};
            const float len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            for (int k = 0; k < 3; ++k) {
                normals[3 * i + k] = (disc || band) ? v[k] / len : 0.0f;
                tight[3 * i + k] = u01();
            }
            const float pick = u01();
            variance[i] = pick < 0.1f ? 0.0f : pick < 0.15f ? -1.0f : pick < 0.18f ? kInf : pick < 0.21f ? kNan
                          : pick < 0.23f ? 3.0e38f : 0.05f * u01();
        }
    variance[0] = kNan;  // the corners: the prefilter's in-image test
    variance[n - 1] = 3.0e38f;
    tight[3 * 5] = kNan;  // a pixel copied through
    int calls = 0;
    for (int iterations = 1; iterations <= 6; ++iterations)
        for (int variant = 0; variant < 8; ++variant) {
            const bool pitched = variant & 1, rgba8 = variant & 2, gamma = variant & 4;
            const size_t in_pitch = pitched ? 12 * (size_t)W + 20 : 12 * (size_t)W;
            std::vector<unsigned char> color(in_pitch * (H - 1) + 12 * (size_t)W);
            for (int y = 0; y < H; ++y) std::memcpy(color.data() + y * in_pitch, tight.data() + 3 * (size_t)y * W, 12 * (size_t)W);
            const size_t bpp = rgba8 ? 4 : 12, out_pitch = pitched ? bpp * W + 8 : bpp * W;
            std::vector<unsigned char> out(out_pitch * (H - 1) + bpp * W, 0xAB);
            ort_denoise_desc_ex x;
            std::memset(&x, 0, sizeof x);
            ort_denoise_desc& d = x.base;
            d.color = reinterpret_cast<const float*>(color.data());
            d.color_pitch_bytes = pitched ? (int64_t)in_pitch : 0;
            d.hits = hits.data();
            d.normals = normals.data();
            d.width = W;
            d.rows = H;
            d.iterations = iterations;
            d.sigma_color = (iterations & 1) ? 0.0f : 1.0f;
            d.sigma_depth = (iterations % 3) ? 0.5f : 0.0f;
            d.normal_power = iterations == 6 ? 0 : 5;
            d.flags = ((iterations & 2) ? 0 : ORT_DENOISE_SAME_SPHERE) | (gamma ? ORT_DENOISE_GAMMA : 0);
            x.variance = variance.data();
            x.sigma_variance = (float)(1 << (iterations % 4));
            const ort_output o = {out.data(), 0, rgba8 ? ORT_FORMAT_RGBA8 : ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0,
                                  pitched ? (int64_t)out_pitch : 0};
            check(ort_debug_denoise_ex(&x, &o) == ORT_OK, "ort_debug_denoise_ex");
            ++calls;
            for (int y = 0; pitched && y + 1 < H; ++y)
                for (size_t b = bpp * W; b < out_pitch; ++b) check(out[y * out_pitch + b] == 0xAB, "bytes between rows untouched");
            if (!rgba8 && !pitched) {  // in place gives the same picture; the gamma is ort_debug_gamma of the linear one
                std::vector<float> buf(tight);
                d.color = buf.data();
                const ort_output ip = {buf.data(), 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
                check(ort_debug_denoise_ex(&x, &ip) == ORT_OK, "in place");
                check(std::memcmp(buf.data(), out.data(), 12 * n) == 0, "in place equals out of place");
                ++calls;
                if (gamma) {
                    d.flags &= ~ORT_DENOISE_GAMMA;
                    d.color = tight.data();
                    check(ort_debug_denoise_ex(&x, &ip) == ORT_OK, "linear");
                    check(ort_debug_gamma(buf.data(), (int64_t)n, buf.data()) == ORT_OK, "ort_debug_gamma");
                    check(std::memcmp(buf.data(), out.data(), 12 * n) == 0, "the gamma output is the gamma of the linear one");
                    ++calls;
                }
            }
        }
    // refusals: codes, nothing written
    std::vector<float> out(3 * n, -3.0f);
    ort_denoise_desc_ex x;
    std::memset(&x, 0, sizeof x);
    x.base.color = tight.data();
    x.base.hits = hits.data();
    x.base.normals = normals.data();
    x.base.width = W;
    x.base.rows = H;
    x.base.iterations = 3;
    x.base.normal_power = 5;
    x.variance = variance.data();
    x.sigma_variance = 2.0f;
    ort_output o = {out.data(), 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
    ort_denoise_desc_ex e = x;
    e.sigma_variance = 0.0f;
    check(ort_debug_denoise_ex(&e, &o) == ORT_ERR_INVALID_ARG, "sigma_variance 0 with a variance refused");
    e.sigma_variance = kNan;
    check(ort_debug_denoise_ex(&e, &o) == ORT_ERR_INVALID_ARG, "NaN sigma_variance refused");
    e = x;
    e.variance = nullptr;
    check(ort_debug_denoise_ex(&e, &o) == ORT_ERR_INVALID_ARG, "sigma_variance without a variance refused");
    e = x;
    e.reserved[2] = 1;
    check(ort_debug_denoise_ex(&e, &o) == ORT_ERR_INVALID_ARG, "reserved refused");
    e = x;
    e.variance = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(variance.data()) + 2);
    check(ort_debug_denoise_ex(&e, &o) == ORT_ERR_INVALID_ARG, "a misaligned variance refused");
    e = x;
    e.base.flags = 4;
    check(ort_debug_denoise_ex(&e, &o) == ORT_ERR_INVALID_ARG, "unknown flags refused");
    e = x;
    e.base.flags = ORT_DENOISE_GAMMA;
    check(ort_debug_denoise(&e.base, &o) == ORT_ERR_INVALID_ARG, "ort_denoise refuses the gamma flag");
    check(ort_debug_denoise_ex(nullptr, &o) == ORT_ERR_INVALID_ARG && ort_debug_denoise_ex(&x, nullptr) == ORT_ERR_INVALID_ARG, "null refused");
    for (float v : out) check(v == -3.0f, "a refused call writes nothing");
    e = x;
    e.base.width = 0;
    check(ort_debug_denoise_ex(&e, &o) == ORT_OK, "an empty image is ORT_OK");

    // the moments emulation: the debug scene by brute force, 13 x 9, N = 5, every k, and a band tile past the frame
    int32_t ns = 0;
    check(ort_scene_debug(nullptr, nullptr, nullptr, &ns) == ORT_OK && ns > 0, "ort_scene_debug");
    std::vector<float> cr(4 * ns), ma(4 * ns), fr(4 * ns);
    check(ort_scene_debug(cr.data(), ma.data(), fr.data(), &ns) == ORT_OK, "ort_scene_debug arrays");
    ort_params p;
    std::memset(&p, 0, sizeof p);
    p.width = 13;
    p.height = 9;
    p.num_samples = 5;
    p.max_depth = 4;
    p.use_octree = 0;
    const float pos[3] = {0.0f, 1.0f, -4.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    check(ort_camera_view(pos, up, 90.0f, 0.0f, p.view) == ORT_OK, "ort_camera_view");
    std::memcpy(p.camera_position, pos, sizeof pos);
    p.camera_zoom = 45.0f;
    int moments = 0;
    const ort_tile tiles[2] = {{0, 13, 0, 9, 0, 0}, {3, 7, 1, 6, 2, 4}};  // the second: rows 1-2, 5-6, 9-10 (past the frame)
    for (const ort_tile& t : tiles)
        for (int k = 1; k <= p.num_samples; ++k) {
            const size_t px = (size_t)t.width * t.rows;
            std::vector<float> mean(3 * px), var(px), pic(3 * px), g(3 * px);
            check(ort_debug_emulate_moments(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                            nullptr, 0, ORT_LAYOUT_COMPACT, &p, &t, k, mean.data(), var.data()) == ORT_OK,
                  "ort_debug_emulate_moments");
            check(ort_debug_emulate_render_prefix(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                  0, nullptr, 0, ORT_LAYOUT_COMPACT, &p, &t, k, pic.data(), nullptr) == ORT_OK,
                  "ort_debug_emulate_render_prefix");
            check(ort_debug_gamma(mean.data(), (int64_t)px, g.data()) == ORT_OK, "ort_debug_gamma");
            for (int j = 0; j < t.rows; ++j) {
                const int y = t.band_height > 0 ? t.y0 + (j / t.band_height) * t.band_stride + j % t.band_height : t.y0 + j;
                for (int c = 0; c < t.width; ++c) {
                    const size_t i = (size_t)j * t.width + c;
                    if (y >= p.height) {
                        check(mean[3 * i] == 0.0f && mean[3 * i + 1] == 0.0f && mean[3 * i + 2] == 0.0f && var[i] == -1.0f, "padding rows");
                        continue;
                    }
                    check(std::memcmp(&g[3 * i], &pic[3 * i], 12) == 0, "the gamma of the mean is the preview");
                    check(k == 1 ? var[i] == -1.0f : (std::isfinite(var[i]) && var[i] >= 0.0f), "the variance");
                }
            }
            // one output at a time
            check(ort_debug_emulate_moments(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                            nullptr, 0, ORT_LAYOUT_COMPACT, &p, &t, k, nullptr, var.data()) == ORT_OK, "variance alone");
            ++moments;
        }
    check(ort_debug_emulate_moments(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                    ORT_LAYOUT_COMPACT, &p, &tiles[0], 6, out.data(), nullptr) == ORT_ERR_INVALID_ARG,
          "samples_done past num_samples refused");
    check(ort_debug_emulate_moments(cr.data(), ma.data(), fr.data(), ns, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                    ORT_LAYOUT_COMPACT, &p, &tiles[0], 2, nullptr, nullptr) == ORT_ERR_INVALID_ARG,
          "both outputs NULL refused");
    std::printf("san_denoise_var: %d denoises of %d x %d, %d moments emulations, refusals and the empty image: ok\n", calls, W, H,
                moments);
    return 0;
}
