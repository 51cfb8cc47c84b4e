// tests/cpp/pick.cpp -- Raytracer::traceCamera and Raytracer::pick on the DEBUG scene (a 64 x 48
// frame of one sample per pixel from the DEBUG view): prints, for every pixel of a tile and both kinds of camera ray, one
// line "rec which i hit sphere t nx ny nz ox oy oz dx dy dz" (hex float bits from t on; the
// DEBUG build's own chatter goes to the same stream), then for the tile's first pixel one line
// "pick x y sphere t px py pz", which tests/test_gpu_camera_query.py compares with
// Renderer.trace_camera and Renderer.pick on the same scene.
//   pick [--brute] [x0 y0 width rows]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "raytracer.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    RaytracerConfig cfg;
    cfg.debug = 1;
    cfg.width = 64;
    cfg.height = 48;
    cfg.numSamples = 1;  // the first-sample ray is the one sample's: what a one-sample frame draws
    cfg.maxRaysDepth = 1;
    int at = 1;
    if (argc > at && std::strcmp(argv[at], "--brute") == 0) {
        cfg.useOctree = 0;
        ++at;
    }
    ort_tile tile{0, (int32_t)cfg.width, 0, (int32_t)cfg.height, 0, 0};
    if (argc >= at + 4) {
        tile.x0 = std::atoi(argv[at]);
        tile.y0 = std::atoi(argv[at + 1]);
        tile.width = std::atoi(argv[at + 2]);
        tile.rows = std::atoi(argv[at + 3]);
    }
    Raytracer rt(cfg);
    const size_t n = (size_t)tile.width * (size_t)tile.rows;
    std::vector<ort_ray> rays(n);
    std::vector<ort_ray_hit> hits(n);
    std::vector<float> normals(3 * n);
    for (int which : {ORT_CAMERA_FIRST_SAMPLE, ORT_CAMERA_PIXEL_CENTRE}) {
        const ort_camera_query q = {rays.data(), hits.data(), normals.data(), 0, which, {0, 0}};
        const int rc = rt.traceCamera(rt.camera, tile, q);
        if (rc != ORT_OK) {
            std::fprintf(stderr, "traceCamera failed (%d): %s\n", rc, rt.lastError());
            return 1;
        }
        for (size_t i = 0; i < n; ++i)
            std::printf("rec %d %zu %d %d %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", which, i,
                        hits[i].sphere >= 0 ? 1 : 0, hits[i].sphere, bits(hits[i].t), bits(normals[3 * i]),
                        bits(normals[3 * i + 1]), bits(normals[3 * i + 2]), bits(rays[i].origin[0]), bits(rays[i].origin[1]),
                        bits(rays[i].origin[2]), bits(rays[i].direction[0]), bits(rays[i].direction[1]),
                        bits(rays[i].direction[2]));
    }
    ort_ray_hit h;
    float point[3];
    const int rc = rt.pick(rt.camera, tile.x0, tile.y0, &h, point);
    if (rc != ORT_OK) {
        std::fprintf(stderr, "pick failed (%d): %s\n", rc, rt.lastError());
        return 1;
    }
    std::printf("pick %d %d %d %08x %08x %08x %08x\n", tile.x0, tile.y0, h.sphere, bits(h.t), bits(point[0]), bits(point[1]),
                bits(point[2]));
    return 0;
}
