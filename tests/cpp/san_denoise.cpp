// tests/cpp/san_denoise.cpp -- the denoiser's host code under AddressSanitizer + UBSan (CPU only,
// Makefile `san`): ort_debug_denoise, the kernels' per-pixel function (denoise.inc denoise_pixel)
// compiled for the host, over a small seeded image with hits, misses and non-finite pixels -- every
// iteration count, both formats, colour and output pitches, in place, every term -- in buffers
// of exactly the bytes the description covers, so that a read or write past them is reported.  A
// non-finite pixel must come through unchanged, the rest finite; the argument errors must come
// back as codes.
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
        std::fprintf(stderr, "san_denoise: FAILED %s (%s)\n", what, ort_last_error(nullptr));
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
    // a disc of sphere 3 and a band of sphere 5 over the sky, unit normals, depths 2 .. 3
    std::vector<ort_ray_hit> hits(n);
    std::vector<float> normals(3 * n), tight(3 * n);
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
        }
    const size_t bad[3] = {0, (size_t)10 * W + 12, n - 1};
    tight[3 * bad[0]] = kNan;
    tight[3 * bad[1] + 1] = kInf;
    tight[3 * bad[2] + 2] = -kInf;
    int calls = 0;
    for (int iterations = 1; iterations <= 6; ++iterations)
        for (int variant = 0; variant < 4; ++variant) {
            const bool pitched = variant & 1, rgba8 = variant & 2;
            // the colour rows a pitch apart, the last row ending with its pixels
            const size_t in_pitch = pitched ? 12 * (size_t)W + 20 : 12 * (size_t)W;
            std::vector<unsigned char> color(in_pitch * (H - 1) + 12 * (size_t)W);
            for (int y = 0; y < H; ++y) std::memcpy(color.data() + y * in_pitch, tight.data() + 3 * (size_t)y * W, 12 * (size_t)W);
            const size_t bpp = rgba8 ? 4 : 12, out_pitch = pitched ? bpp * W + 8 : bpp * W;
            std::vector<unsigned char> out(out_pitch * (H - 1) + bpp * W, 0xAB);
            ort_denoise_desc d;
            std::memset(&d, 0, sizeof d);
            d.color = reinterpret_cast<const float*>(color.data());
            d.color_pitch_bytes = pitched ? (int64_t)in_pitch : 0;
            d.hits = hits.data();
            d.normals = normals.data();
            d.width = W;
            d.rows = H;
            d.iterations = iterations;
            d.sigma_color = (iterations & 1) ? 0.0f : 1.0f;
            d.sigma_depth = (iterations % 3) ? 0.5f : 0.0f;
            d.normal_power = iterations == 6 ? 0 : (iterations == 5 ? 7 : 5);
            d.flags = (iterations & 2) ? 0 : ORT_DENOISE_SAME_SPHERE;
            const ort_output o = {out.data(), 0, rgba8 ? ORT_FORMAT_RGBA8 : ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0,
                                  pitched ? (int64_t)out_pitch : 0};
            check(ort_debug_denoise(&d, &o) == ORT_OK, "ort_debug_denoise");
            ++calls;
            for (int y = 0; y < H; ++y) {
                if (pitched && y + 1 < H)
                    for (size_t b = bpp * W; b < out_pitch; ++b) check(out[y * out_pitch + b] == 0xAB, "bytes between rows untouched");
                if (rgba8) continue;
                const float* row = reinterpret_cast<const float*>(out.data() + y * out_pitch);
                for (int x = 0; x < W; ++x) {
                    const size_t i = (size_t)y * W + x;
                    const bool through = i == bad[0] || i == bad[1] || i == bad[2];
                    if (through) check(std::memcmp(row + 3 * x, tight.data() + 3 * i, 12) == 0, "a non-finite pixel passes through");
                    else check(std::isfinite(row[3 * x]) && std::isfinite(row[3 * x + 1]) && std::isfinite(row[3 * x + 2]), "finite result");
                }
            }
            if (!rgba8 && !pitched) {  // in place gives the same picture
                std::vector<float> buf(tight);
                d.color = buf.data();
                const ort_output ip = {buf.data(), 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
                check(ort_debug_denoise(&d, &ip) == ORT_OK, "in place");
                check(std::memcmp(buf.data(), out.data(), 12 * n) == 0, "in place equals out of place");
                ++calls;
            }
        }
    // refusals: codes, nothing written
    std::vector<float> out(3 * n, -3.0f);
    ort_denoise_desc d;
    std::memset(&d, 0, sizeof d);
    d.color = tight.data();
    d.hits = hits.data();
    d.normals = normals.data();
    d.width = W;
    d.rows = H;
    d.iterations = 3;
    d.normal_power = 5;
    ort_output o = {out.data(), 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
    ort_denoise_desc e = d;
    e.iterations = 7;
    check(ort_debug_denoise(&e, &o) == ORT_ERR_INVALID_ARG, "iterations 7 refused");
    e = d;
    e.sigma_color = kNan;
    check(ort_debug_denoise(&e, &o) == ORT_ERR_INVALID_ARG, "NaN sigma refused");
    e = d;
    e.color_pitch_bytes = 12 * W - 4;
    check(ort_debug_denoise(&e, &o) == ORT_ERR_INVALID_ARG, "short colour pitch refused");
    o.placement = ORT_PLACE_FRAME;
    check(ort_debug_denoise(&d, &o) == ORT_ERR_INVALID_ARG, "frame placement refused");
    o.placement = ORT_PLACE_TILE;
    check(ort_debug_denoise(nullptr, &o) == ORT_ERR_INVALID_ARG && ort_debug_denoise(&d, nullptr) == ORT_ERR_INVALID_ARG, "null refused");
    for (float v : out) check(v == -3.0f, "a refused call writes nothing");
    e = d;
    e.width = 0;
    e.color = nullptr;
    check(ort_debug_denoise(&e, &o) == ORT_OK, "an empty image is ORT_OK");
    std::printf("san_denoise: %d denoises of %d x %d, refusals and the empty image: ok\n", calls, W, H);
    return 0;
}
