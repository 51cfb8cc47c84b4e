// raytracer.cpp -- Raytracer on the gfx950 kernel (see raytracer.h).
#include "raytracer.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include <sched.h>

#include <hip/hip_runtime_api.h>

#include "scene.h"

Raytracer::Raytracer() : Raytracer(RaytracerConfig()) {}

Raytracer::Raytracer(const RaytracerConfig& c)
    : camera(ortm::vec3(0.0f, 8.0f, 30.0f)),
      cfg(c),
      width((int)c.width),
      height((int)c.height),
      ctx(nullptr),
      sceneReady(false),
      octree(c.debug ? c.debugDepth : c.maxDepth, c.debug ? c.debugSpheresPerNode : c.maxSpheresPerNode),
      statsFilename(c.outputFile),
      frameCount(0) {
    // camera pose of main() (src/main.cpp:29-40)
    if (cfg.debug) camera.Position = ortm::vec3(30.0f, 20.0f, -50.0f);
    else camera.Position = ortm::vec3(0.0f, 2.5f, -10.0f);
    camera.updateCameraVectors();
}

Raytracer::~Raytracer() { cleanupBuffers(); }

bool Raytracer::initialize() {
    if (ctx || group) return true;
    if (cfg.devices.size() > 1) {  // several GPUs: one context each inside an ort_group
        // RCCL over distinct devices; a device listed twice (testing on one GPU) gathers by copies
        bool distinct = true;
        for (size_t i = 0; i < cfg.devices.size(); ++i)
            for (size_t j = 0; j < i; ++j) distinct = distinct && cfg.devices[i] != cfg.devices[j];
        const int32_t transport = distinct ? ORT_GROUP_TRANSPORT_RCCL : ORT_GROUP_TRANSPORT_COPY;
        if (ort_group_create(cfg.devices.data(), (int32_t)cfg.devices.size(), transport, &group) != ORT_OK) {
            std::cerr << "Failed to create the MI355X device group: " << ort_group_last_error(nullptr) << std::endl;
            group = nullptr;
            return false;
        }
        return true;
    }
    if (ort_create(cfg.device, &ctx) != ORT_OK) {
        std::cerr << "Failed to create the MI355X context: " << ort_last_error(nullptr) << std::endl;
        ctx = nullptr;
        return false;
    }
    return true;
}

const char* Raytracer::lastError() const { return group ? ort_group_last_error(group) : ort_last_error(ctx); }

std::vector<Sphere> Raytracer::generatePreBuiltSpheres() { return ort::generatePreBuiltSpheres(); }
std::vector<Sphere> Raytracer::generateRandomSpheres() { return ort::generateRandomSpheres(cfg.numSpheres, cfg.seed); }

std::vector<Sphere> Raytracer::generateSpheres() {
    if (cfg.debug) return ort::generateDebugSpheres();
    if (cfg.usePrebuilt) return generatePreBuiltSpheres();
    return generateRandomSpheres();
}

void Raytracer::setupScene() {
    spheres = generateSpheres();
    const int maxDepth = cfg.debug ? cfg.debugDepth : cfg.maxDepth;
    const int maxSpheresPerNode = cfg.debug ? cfg.debugSpheresPerNode : cfg.maxSpheresPerNode;
    octree = Octree(maxDepth, maxSpheresPerNode);
    if (cfg.gpuBuild && !cfg.debug) return;  // setupBuffers builds it on the device
    octree.build(spheres, cfg.debug);
    if (cfg.debug) octree.printFlattenedTree();
}

void Raytracer::setupBuffers() {
    // SoA packing of src/raytracer.cpp:87-101, then one upload (replaces 7x glBufferData)
    std::vector<float> cr(4 * spheres.size()), ma(4 * spheres.size()), fr(4 * spheres.size());
    ort::packSpheres(spheres, cr.data(), ma.data(), fr.data());
    int rc = ORT_OK;
    const int ranks = group ? ort_group_size(group) : 1;
    for (int r = 0; r < ranks && rc == ORT_OK; ++r) {  // every device holds the whole scene
        ort_ctx* c = ctx;
        if (group) ort_group_context(group, r, &c);
        if (cfg.gpuBuild && !cfg.debug) {
            rc = ort_build_scene(c, cr.data(), ma.data(), fr.data(), (int32_t)spheres.size(), octree.getMaxDepth(),
                                 octree.getMaxSpheresPerNode(), 0);
            float ms = 0.0f;
            if (rc == ORT_OK) ort_last_build_ms(c, &ms);
            gpuBuildSeconds = ms * 1e-3;
        } else {
            rc = ort_upload_octree_nodes(c, cr.data(), ma.data(), fr.data(), (int32_t)spheres.size(),
                                         octree.flattenedTree.data(), (int32_t)octree.flattenedTree.size(),
                                         octree.objectIndices.data(), (int64_t)octree.objectIndices.size());
        }
        if (rc != ORT_OK) std::cerr << "scene upload failed: " << ort_last_error(c) << std::endl;
    }
    sceneReady = rc == ORT_OK;
}

void Raytracer::cleanupBuffers() {
    if (dframe) (void)hipFree(dframe);
    dframe = nullptr;
    if (dguides) (void)hipFree(dguides);
    dguides = nullptr;
    dguidesBytes = 0;
    accum = nullptr;  // (ort_destroy frees it)
    history = nullptr;
    if (ctx) ort_destroy(ctx);
    if (group) ort_group_destroy(group);
    ctx = nullptr;
    group = nullptr;
    sceneReady = false;
}

ort_params Raytracer::frameParams(const Camera& cam) const {
    ort_params p;
    p.width = width;
    p.height = height;
    p.num_samples = cfg.numSamples;
    p.max_depth = cfg.maxRaysDepth;
    p.use_octree = cfg.useOctree;
    const ortm::mat4 v = cam.GetViewMatrix();
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) p.view[4 * c + r] = v[c][r];
    p.camera_position[0] = cam.Position.x;
    p.camera_position[1] = cam.Position.y;
    p.camera_position[2] = cam.Position.z;
    p.camera_zoom = cam.Zoom;
    return p;
}

int Raytracer::render(const Camera& cam, const ort_tile& tile, float* out, bool outIsDevice, void* stream) {
    const ort_output o = {out, outIsDevice ? 1 : 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
    return render(cam, tile, o, stream);
}

int Raytracer::render(const Camera& cam, const ort_tile& tile, const ort_output& output, void* stream) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // a group renders whole frames (render(cam, rgb))
    if (!sceneReady) {
        setupScene();
        setupBuffers();
        if (!sceneReady) return ORT_ERR_INVALID_ARG;
    }
    const ort_params p = frameParams(cam);
    return ort_render_ex(ctx, &p, &tile, &output, stream);
}

int Raytracer::traceRays(const ort_ray* rays, int64_t n, ort_ray_hit* hits, float* normals) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // queries run on one context
    if (!sceneReady) {
        setupScene();
        setupBuffers();
        if (!sceneReady) return ORT_ERR_INVALID_ARG;
    }
    const ort_ray_query q = {rays, n, hits, normals, 0, cfg.useOctree, 0, 0};
    return ort_trace_rays(ctx, &q, nullptr);
}

int Raytracer::traceRays(const ort_ray* rays, int64_t n, ort_ray_hit* hits, float* normals, int mode, const float* t_range) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // queries run on one context
    if (!sceneReady) {
        setupScene();
        setupBuffers();
        if (!sceneReady) return ORT_ERR_INVALID_ARG;
    }
    const ort_ray_query_ex q = {{rays, n, hits, normals, 0, cfg.useOctree, 0, 0}, t_range, mode, {0, 0, 0}};
    return ort_trace_rays_ex(ctx, &q, nullptr);
}

int Raytracer::occluded(const float* a, const float* b, int64_t n, uint8_t* out, float eps) {
    if (n < 0 || (n > 0 && (!a || !b || !out)) || !(eps >= 0.0f)) return ORT_ERR_INVALID_ARG;
    std::vector<ort_ray> rays((size_t)n);
    std::vector<float> range(2 * (size_t)n);
    std::vector<ort_ray_hit> hits((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const float d[3] = {b[3 * i] - a[3 * i], b[3 * i + 1] - a[3 * i + 1], b[3 * i + 2] - a[3 * i + 2]};
        const float len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        const bool ok = len > 2.0f * eps;  // (NaN: not ok) -- else an empty interval: a miss
        rays[(size_t)i] = {{a[3 * i], a[3 * i + 1], a[3 * i + 2]},
                           {ok ? d[0] / len : 0.0f, ok ? d[1] / len : 0.0f, ok ? d[2] / len : 0.0f}};
        range[2 * (size_t)i] = eps;
        range[2 * (size_t)i + 1] = ok ? len - eps : 0.0f;
    }
    const int rc = traceRays(rays.data(), n, hits.data(), nullptr, ORT_QUERY_ANY, range.data());
    if (rc != ORT_OK) return rc;
    for (int64_t i = 0; i < n; ++i) out[i] = hits[(size_t)i].sphere >= 0 ? 1 : 0;
    return ORT_OK;
}

int Raytracer::traceCamera(const Camera& cam, const ort_tile& tile, const ort_camera_query& query) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // queries run on one context
    if (!sceneReady) {
        setupScene();
        setupBuffers();
        if (!sceneReady) return ORT_ERR_INVALID_ARG;
    }
    const ort_params p = frameParams(cam);
    return ort_trace_camera(ctx, &p, &tile, &query, nullptr);
}

int Raytracer::traceRadiance(const ort_ray* rays, const float* states, int64_t n, int maxDepth, int paths, float* radiance,
                             float* statesOut, int flags) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // queries run on one context
    if (!sceneReady) {
        setupScene();
        setupBuffers();
        if (!sceneReady) return ORT_ERR_INVALID_ARG;
    }
    const ort_radiance_query q = {rays, n, states, radiance, statesOut, 0, cfg.useOctree, maxDepth, paths, flags, 0};
    return ort_trace_radiance(ctx, &q, nullptr);
}

int Raytracer::pick(const Camera& cam, int x, int y, ort_ray_hit* hit, float point[3]) {
    ort_ray ray;
    ort_ray_hit h = {0.0f, -1};
    const ort_tile tile{x, 1, y, 1, 0, 0};
    const ort_camera_query q = {&ray, &h, nullptr, 0, ORT_CAMERA_PIXEL_CENTRE, {0, 0}};
    const int rc = traceCamera(cam, tile, q);
    if (rc != ORT_OK) return rc;
    if (hit) *hit = h;
    if (point)
        for (int k = 0; k < 3; ++k) point[k] = ray.origin[k] + h.t * ray.direction[k];
    return ORT_OK;
}

int Raytracer::renderProgressive(const Camera& cam, int samples, float* rgb, int* samplesDone) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // accumulations live on one context
    if (!sceneReady) {
        setupScene();
        setupBuffers();
        if (!sceneReady) return ORT_ERR_INVALID_ARG;
    }
    const ort_params p = frameParams(cam);
    int rc = ORT_OK;
    if (!accum) {
        const ort_tile t{0, width, 0, height, 0, 0};
        const int flags = accumAdaptive ? ORT_ACCUM_ADAPTIVE : (accumMoments ? ORT_ACCUM_MOMENTS : 0);
        if ((rc = ort_accum_begin_ex(ctx, &p, &t, flags, &accum)) != ORT_OK) return rc;
        accumParams = p;
    } else if (std::memcmp(p.view, accumParams.view, sizeof p.view) != 0 ||
               std::memcmp(p.camera_position, accumParams.camera_position, sizeof p.camera_position) != 0 ||
               p.camera_zoom != accumParams.camera_zoom) {  // the camera moved: the frame starts again
        if ((rc = ort_accum_restart(ctx, accum, &p)) != ORT_OK) return rc;
        accumParams = p;
    }
    const ort_output o = {rgb, 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
    if (accumAdaptive) {
        const ort_accum_adaptive a = adaptiveCriterion(samples);
        rc = ort_accum_render_adaptive(ctx, accum, &a, &o, nullptr);
    } else {
        rc = ort_accum_render(ctx, accum, samples, &o, nullptr);
    }
    ort_accum_info info{};
    if (samplesDone && ort_accum_get_info(accum, &info) == ORT_OK) *samplesDone = info.samples_done;
    return rc;
}

void Raytracer::setProgressiveMoments(bool on) {
    if (on == accumMoments) return;
    accumMoments = on;
    if (accum && ctx) (void)ort_accum_free(ctx, accum);  // the state has another shape: the frame starts again
    accum = nullptr;
}

ort_accum_adaptive Raytracer::adaptiveCriterion(int samples) const {
    return {samples, adaptiveMinSamples, adaptiveThreshold, adaptiveFloor, {0, 0, 0, 0}};
}

void Raytracer::setProgressiveAdaptive(bool on, float threshold, int minSamples, float luminanceFloor) {
    adaptiveThreshold = threshold;
    adaptiveMinSamples = minSamples;
    adaptiveFloor = luminanceFloor;
    if (on == accumAdaptive) return;  // (a new criterion alone applies from the next pass on)
    accumAdaptive = on;
    if (accum && ctx) (void)ort_accum_free(ctx, accum);  // the state has another shape: the frame starts again
    accum = nullptr;
}

int Raytracer::readSampleCounts(int32_t* counts, bool onDevice) {
    if (group) return ORT_ERR_UNSUPPORTED;
    if (!ctx || !accum) return ORT_ERR_INVALID_ARG;  // no renderProgressive yet
    return ort_accum_read_counts(ctx, accum, counts, onDevice ? 1 : 0, nullptr);
}

long long Raytracer::pendingPixels() {
    if (group || !ctx || !accum || !accumAdaptive) return -1;
    const ort_accum_adaptive a = adaptiveCriterion(1);
    struct ort_accum_adaptive_stats st;
    if (ort_accum_adaptive_stats(ctx, accum, &a, &st) != ORT_OK) return -1;
    return (long long)st.pending;
}

int Raytracer::readMoments(float* mean, float* variance, bool onDevice) {
    if (group) return ORT_ERR_UNSUPPORTED;
    if (!ctx || !accum) return ORT_ERR_INVALID_ARG;  // no renderProgressive yet
    const ort_accum_moments m = {mean, variance, onDevice ? 1 : 0, {0, 0, 0}};
    return ort_accum_read_moments(ctx, accum, &m, nullptr);
}

int Raytracer::denoise(const Camera& cam, const ort_tile& tile, const float* rgb, const ort_output& output,
                       const DenoiseOptions& options) {
    return denoise(cam, tile, rgb, nullptr, 0.0f, false, output, options);
}

int Raytracer::denoise(const Camera& cam, const ort_tile& tile, const float* rgb, const float* variance, float sigmaVariance,
                       bool gamma, const ort_output& output, const DenoiseOptions& options) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // the denoiser runs on one context
    if (tile.width < 0 || tile.rows < 0 || tile.y0 < 0 || (tile.band_height > 0 && tile.rows > tile.band_height))
        return ORT_ERR_INVALID_ARG;  // rows that are not neighbours in the frame
    // rows with y >= height are neither filtered nor used as taps (as Renderer.denoise)
    const int real = std::max(0, std::min(tile.rows, height - tile.y0));
    const size_t n = (size_t)tile.width * (size_t)tile.rows;
    std::vector<ort_ray_hit> hits;
    std::vector<float> normals;
    ort_camera_query q = {nullptr, nullptr, nullptr, output.is_device ? 1 : 0, ORT_CAMERA_PIXEL_CENTRE, {0, 0}};
    if (output.is_device) {
        if (dguidesBytes < 20 * n) {
            if (dguides) (void)hipFree(dguides);
            dguides = nullptr;
            dguidesBytes = 0;
            if (hipSetDevice(cfg.device) != hipSuccess || hipMalloc(&dguides, 20 * n) != hipSuccess) return ORT_ERR_OUT_OF_MEMORY;
            dguidesBytes = 20 * n;
        }
        q.hits = static_cast<ort_ray_hit*>(dguides);
        q.normals = reinterpret_cast<float*>(static_cast<unsigned char*>(dguides) + 8 * n);
    } else {
        hits.resize(n);
        normals.resize(3 * n);
        q.hits = hits.data();
        q.normals = normals.data();
    }
    if (n > 0) {
        const int rc = traceCamera(cam, tile, q);
        if (rc != ORT_OK) return rc;
    }
    ort_denoise_desc_ex x;
    std::memset(&x, 0, sizeof x);
    ort_denoise_desc& d = x.base;
    d.color = rgb;
    d.hits = q.hits;
    d.normals = q.normals;
    d.width = tile.width;
    d.rows = real;
    d.on_device = q.on_device;
    d.iterations = options.iterations;
    d.sigma_color = options.sigmaColor;
    d.sigma_depth = options.sigmaDepth;
    d.normal_power = options.normalPower;
    d.flags = options.sameSphere ? ORT_DENOISE_SAME_SPHERE : 0;
    int rc;
    if (!variance && !gamma && sigmaVariance == 0.0f) {
        rc = ort_denoise(ctx, &d, &output, nullptr);
    } else {
        if (gamma) d.flags |= ORT_DENOISE_GAMMA;
        x.variance = variance;
        x.sigma_variance = sigmaVariance;
        rc = ort_denoise_ex(ctx, &x, &output, nullptr);
    }
    if (rc != ORT_OK || real == tile.rows || !output.data) return rc;
    // the padding rows as render writes them: zero bytes
    const size_t rowBytes = (size_t)tile.width * (output.format == ORT_FORMAT_RGBA8 ? 4 : 12);
    const size_t pitch = output.row_pitch_bytes ? (size_t)output.row_pitch_bytes : rowBytes;
    unsigned char* first = static_cast<unsigned char*>(output.data) + (size_t)real * pitch;
    if (output.is_device) {
        if (hipMemset2D(first, pitch, 0, rowBytes, (size_t)(tile.rows - real)) != hipSuccess) return ORT_ERR_HIP;
    } else {
        for (int j = real; j < tile.rows; ++j) std::memset(first + (size_t)(j - real) * pitch, 0, rowBytes);
    }
    return ORT_OK;
}

int Raytracer::reproject(const Camera& cam, const ort_tile& tile, const float* rgb, float* outColor, float* outVariance,
                         float alpha, float depthTolerance) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // histories live on one context
    if (tile.width < 0 || tile.rows < 0) return ORT_ERR_INVALID_ARG;
    const size_t n = (size_t)tile.width * (size_t)tile.rows;
    std::vector<ort_ray> rays(n);
    std::vector<ort_ray_hit> hits(n);
    if (n > 0) {
        const ort_camera_query q = {rays.data(), hits.data(), nullptr, 0, ORT_CAMERA_PIXEL_CENTRE, {0, 0}};
        const int rc = traceCamera(cam, tile, q);
        if (rc != ORT_OK) return rc;
    }
    if (history && (historyWidth != tile.width || historyRows != tile.rows)) {
        (void)ort_history_free(ctx, history);
        history = nullptr;
    }
    if (!history) {
        const int rc = ort_history_begin(ctx, tile.width, tile.rows, &history);
        if (rc != ORT_OK) return rc;
        historyWidth = tile.width;
        historyRows = tile.rows;
    }
    const ort_params p = frameParams(cam);
    ort_history_frame f;
    std::memset(&f, 0, sizeof f);
    f.params = &p;
    f.tile = &tile;
    f.color = rgb;
    f.rays = rays.data();
    f.hits = hits.data();
    f.out_color = outColor;
    f.out_variance = outVariance;
    f.alpha = alpha;
    f.depth_tolerance = depthTolerance;
    if (!historyMotion) return ort_history_update(ctx, history, &f, nullptr);
    ort_history_frame_ex fx;
    std::memset(&fx, 0, sizeof fx);
    fx.base = f;
    fx.base.flags = ORT_HISTORY_MOTION;
    return ort_history_update_ex(ctx, history, &fx, nullptr);
}

void Raytracer::setHistoryMotion(bool on) { historyMotion = on; }

int Raytracer::moveSpheres(const int* indices, const float* centerRadius, int n) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) return ORT_ERR_UNSUPPORTED;  // histories live on one context
    if (n < 0 || (n > 0 && (!indices || !centerRadius))) return ORT_ERR_INVALID_ARG;
    if (!sceneReady) {
        setupScene();
        setupBuffers();
        if (!sceneReady) return ORT_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (indices[i] < 0 || (size_t)indices[i] >= spheres.size()) return ORT_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) {
        Sphere& s = spheres[(size_t)indices[i]];
        s.center = ortm::vec3(centerRadius[4 * i], centerRadius[4 * i + 1], centerRadius[4 * i + 2]);
        s.radius = centerRadius[4 * i + 3];
    }
    octree = Octree(octree.getMaxDepth(), octree.getMaxSpheresPerNode());
    if (!(cfg.gpuBuild && !cfg.debug)) octree.build(spheres, false);
    if (accum) (void)ort_accum_free(ctx, accum);  // begun on the scene that goes: the frame starts again
    accum = nullptr;
    setupBuffers();
    return sceneReady ? ORT_OK : ORT_ERR_INVALID_ARG;
}

void Raytracer::resetHistory() {
    if (history && ctx) (void)ort_history_reset(ctx, history);
}

int Raytracer::render(const Camera& cam, float* rgb) {
    if (!ctx && !group && !initialize()) return ORT_ERR_HIP;
    if (group) {
        if (!sceneReady) {
            setupScene();
            setupBuffers();
            if (!sceneReady) return ORT_ERR_INVALID_ARG;
        }
        const ort_params p = frameParams(cam);
        return ort_group_render(group, &p, rgb, 0);
    }
    ort_tile t{0, width, 0, height, 0, 0};
    return render(cam, t, rgb, false, nullptr);
}

void Raytracer::run() {
    if (!initialize()) return;
    setupScene();
    setupBuffers();
    if (!sceneReady) return;
    const size_t frameBytes = sizeof(float) * 3 * (size_t)width * height;
    if (cfg.readback) {
        frame.assign((size_t)width * height * 3, 0.0f);
    } else if (!dframe) {  // on the device that renders (a group: devices[0], where it assembles)
        const int dev = cfg.devices.size() > 1 ? cfg.devices[0] : cfg.device;
        if (hipSetDevice(dev) != hipSuccess || hipMalloc((void**)&dframe, frameBytes) != hipSuccess) {
            dframe = nullptr;
            std::cerr << "run: no device frame buffer of " << frameBytes << " bytes" << std::endl;
            return;
        }
    }
    for (int i = 0; i < cfg.warmupFrames; i++) renderRun();
    for (int i = 0; i < cfg.frames; i++) {
        const auto frameStart = std::chrono::steady_clock::now();
        if (renderRun() != ORT_OK) {
            std::cerr << "render failed: " << lastError() << std::endl;
            break;
        }
        const double frameTime = std::chrono::duration<double>(std::chrono::steady_clock::now() - frameStart).count();
        if (cfg.collectStats) {
            renderTimes.push_back(frameTime);
            frameCount++;
        }
    }
    if (cfg.collectStats) {
        if (cfg.extendedStats && !countWork()) std::cerr << "counting the frame's work failed: " << lastError() << std::endl;
        saveStats();
    }
}

// A synchronous frame either way (ort_render / ort_group_render on the context's own stream
// return once the frame is complete).
int Raytracer::renderRun() {
    if (!dframe) return render(camera, frame.data());
    if (group) {
        const ort_params p = frameParams(camera);
        return ort_group_render(group, &p, dframe, 1);
    }
    const ort_tile t{0, width, 0, height, 0, 0};
    return render(camera, t, dframe, true, nullptr);
}

// saveStats (src/raytracer.cpp:359-449): 2.5-sigma z-score filter, one ';' row.
std::string Raytracer::statsRow(const RaytracerConfig& cfg, const std::vector<double>& all, double buildSeconds,
                                const StatsWork* w) {
    if (all.empty()) return std::string();
    double sum = 0.0;
    for (double t : all) sum += t;
    const double mean = sum / all.size();
    double variance = 0.0;
    for (double t : all) variance += (t - mean) * (t - mean);
    const double stdDev = std::sqrt(variance / all.size());
    const double THRESHOLD = 2.5;
    std::vector<double> clean;
    int outliers = 0;
    for (double t : all) {
        const double z = std::abs(t - mean) / stdDev;
        if (z <= THRESHOLD) clean.push_back(t);
        else outliers++;
    }
    if (outliers > 0) std::cout << "Removed " << outliers << " outliers from " << all.size() << " samples" << std::endl;
    double total = 0.0, mn = clean.empty() ? 9999 : clean[0], mx = clean.empty() ? 0 : clean[0], fpsTotal = 0.0;
    for (double t : clean) {
        total += t;
        mn = std::min(mn, t);
        mx = std::max(mx, t);
        fpsTotal += 1.0 / t;
    }
    if (clean.empty()) {  // every sample an outlier (all equal: stdDev 0, z NaN): the unfiltered data
        clean = all;
        total = sum;
        for (double t : clean) {
            mn = std::min(mn, t);
            mx = std::max(mx, t);
            fpsTotal += 1.0 / t;
        }
    }
    const double avg = total / clean.size();
    const double fpsAvg = fpsTotal / clean.size();
    std::ostringstream row;
    row << cfg.useOctree << ";" << cfg.numSpheres << ";" << cfg.maxDepth << ";" << cfg.maxSpheresPerNode << ";"
        << cfg.numSamples << ";" << cfg.maxRaysDepth << ";" << cfg.width << ";" << cfg.height << ";" << mn << ";" << mx
        << ";" << avg << ";" << 1.0 / mx << ";" << 1.0 / mn << ";" << fpsAvg << ";" << buildSeconds;
    if (w) {
        const double mrays = (double)w->traversals / avg / 1e6;
        const double bytesPerRay = w->traversals ? w->algorithmicBytes / (double)w->traversals : 0.0;
        const double hbmPeakBytes = 8.0e12;  // MI355X HBM3E
        row << ";" << mrays << ";" << bytesPerRay << ";" << mrays * 1e6 * bytesPerRay / hbmPeakBytes << ";" << w->gpus
            << ";" << w->hostCores;
    }
    return row.str();
}

void Raytracer::saveStats() {
    if (renderTimes.empty()) {
        std::cout << "No render times recorded." << std::endl;
        return;
    }
    std::ofstream outFile(statsFilename, std::ios::out | std::ios::app);
    if (!outFile || !outFile.is_open()) {
        std::cerr << "Error opening file for writing: " << statsFilename << std::endl;
        return;
    }
    const double build = (cfg.gpuBuild && !cfg.debug) ? gpuBuildSeconds : octree.buildTime;
    outFile << statsRow(cfg, renderTimes, build, cfg.extendedStats ? &work : nullptr) << std::endl;
}

// The frame's work for the extended columns: the counting variant of the kernel over the
// full frame (untimed; on devices[0]'s context for a group, which holds the same scene).
bool Raytracer::countWork() {
    ort_ctx* c = ctx;
    if (group && ort_group_context(group, 0, &c) != ORT_OK) return false;
    const ort_params p = frameParams(camera);
    const ort_tile t{0, width, 0, height, 0, 0};
    uint64_t n[ORT_COUNT_N] = {0};
    if (ort_count_traffic(c, &p, &t, n) != ORT_OK) return false;
    work.traversals = n[ORT_COUNT_TRAVERSALS];
    work.algorithmicBytes = 36.0 * n[ORT_COUNT_NODES_POPPED] + 32.0 * n[ORT_COUNT_CHILD_RECORDS] +
                            20.0 * n[ORT_COUNT_LEAF_OBJECTS] + 32.0 * n[ORT_COUNT_ACCEPTED_HITS] +
                            12.0 * n[ORT_COUNT_PIXELS];
    work.gpus = group ? ort_group_size(group) : 1;
    cpu_set_t set;
    work.hostCores = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 1;
    return true;
}
