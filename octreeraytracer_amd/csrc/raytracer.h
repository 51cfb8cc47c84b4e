// raytracer.h -- the reference's Raytracer class (src/raytracer.h:13-60) on the MI355X
// kernel instead of OpenGL.
//
// Kept: Raytracer(), ~Raytracer(), initialize(), run(), and the private stages
// setupScene / setupBuffers / cleanupBuffers / generateSpheres / generatePreBuiltSpheres /
// generateRandomSpheres / saveStats with the reference's semantics and CSV schema.
// New: render() -- one frame into a caller buffer (the reference has no readback,
// SURVEY.md F3/F4) -- and RaytracerConfig, the runtime form of src/config.h.
// No window: initialize() creates the device context (the reference's GLFW/GLAD/shader
// setup, src/raytracer.cpp:32-60); run() renders warm-up + timed frames headless.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ort.h"
#include "camera.h"
#include "octree.h"
#include "sphere.h"

// src/config.h as a runtime struct; defaults equal the reference's constants.
struct RaytracerConfig {
    int debug = 0;                 // DEBUG
    int useOctree = 1;             // USEOCTREE
    int usePrebuilt = 0;           // USEPREBUILT
    int numSpheres = 100;          // NUMSPHERES
    int maxDepth = 3;              // MAXDEPTH
    int debugDepth = 3;            // DEBUGDEPTH
    int maxSpheresPerNode = 0;     // MAXSPHERESPERNODE
    int debugSpheresPerNode = 2;   // DEBUGSPHERESPERNODE
    int numSamples = 16;           // NUMSAMPLES
    int maxRaysDepth = 8;          // MAXRAYSDEPTH
    unsigned width = 800;          // SCR_WIDTH
    unsigned height = 600;         // SCR_HEIGHT
    bool collectStats = false;     // COLLECTSTATS
    std::string outputFile = "stats.csv";  // OUTPUTFILE
    // new knobs
    uint32_t seed = 42;            // replaces std::random_device in generateRandomSpheres
    int device = 0;                // HIP device of the context
    std::vector<int> devices;      // several GPUs: an ort_group over these (bands dealt round-robin,
                                   // RCCL gather to devices[0]; a device listed twice
                                   // gathers by device copies instead); empty = `device` only
    int frames = 50;               // frames of run() (the reference stops after 50 with stats)
    int warmupFrames = 15;         // src/raytracer.cpp:455
    bool gpuBuild = false;         // build the octree on the GPU (ort_build_scene, same tree) instead
                                   // of Octree::build on the host; getOctree() then stays empty
    bool extendedStats = false;    // saveStats appends 5 throughput columns to the reference's 15
                                   // (see StatsWork / Raytracer::statsRow)
    bool readback = false;         // run(): copy every frame to host memory; default off: the frames
                                   // stay in a device buffer, as the reference's stay in its GL
                                   // framebuffer (src/raytracer.cpp:476-519 never reads them back)
};

// Work of one frame for the extended stats columns: ort_count_traffic over the full frame
// (reference-layout counters), plus the device and host-core counts.
struct StatsWork {
    uint64_t traversals = 0;       // octree walks per frame (all samples and bounces)
    double algorithmicBytes = 0;   // 36/node popped + 32/child record + 20/leaf object + 32/hit + 12/pixel
    int gpus = 1;
    int hostCores = 1;
};

// Raytracer::denoise's parameters (include/ort.h ort_denoise_desc): the library's defaults.
struct DenoiseOptions {
    int iterations = 3;        // 1 .. 6: steps 1, 2, 4, ...
    float sigmaColor = 0.0f;   // 0: the colour term off
    float sigmaDepth = 0.0f;   // 0: the depth term off
    int normalPower = 5;       // squarings of the clamped dot product of the normals, 0 .. 7
    bool sameSphere = true;    // taps never cross from one sphere (or the sky) to another
};

class Raytracer {
public:
    Raytracer();
    explicit Raytracer(const RaytracerConfig& cfg);
    ~Raytracer();
    Raytracer(const Raytracer&) = delete;
    Raytracer& operator=(const Raytracer&) = delete;

    bool initialize();
    void run();

    // One full frame of the current scene seen from `cam` into rgb (width*height*3
    // floats, row 0 = bottom row, as the GL framebuffer).  Builds and uploads the scene on
    // first use.  Returns ORT_OK or an ORT_ERR_* code (message: lastError()).
    int render(const Camera& cam, float* rgb);
    // A tile (see ort_tile in include/ort.h) into host or device memory, optionally
    // stream-ordered on a caller hipStream_t.  Single-device configurations only (a group
    // renders whole frames: ORT_ERR_UNSUPPORTED).
    int render(const Camera& cam, const ort_tile& tile, float* out, bool outIsDevice, void* stream);
    // The same with the output described by an ort_output (include/ort.h ort_render_ex): RGBA8
    // as the GL default framebuffer holds it, a row pitch, the tile placed into a whole frame.
    int render(const Camera& cam, const ort_tile& tile, const ort_output& output, void* stream);
    // Ray queries (include/ort.h ort_trace_rays): what each of n rays hits in the current scene
    // -- hits[i] = {t, sphere index in getSpheres()} ({0, -1}: a miss), normals (nullptr, or 3
    // floats per ray) the surface normals -- by the walk the frames are drawn with (cfg.useOctree).
    // Host pointers; builds and uploads the scene on first use, like render.  Single-device
    // configurations only (a group: ORT_ERR_UNSUPPORTED).
    int traceRays(const ort_ray* rays, int64_t n, ort_ray_hit* hits, float* normals = nullptr);
    // The same in a query mode (include/ort.h ort_trace_rays_ex): ORT_QUERY_NEAREST -- the nearest
    // hit inside the ray's interval, the same with and without the octree -- or ORT_QUERY_ANY -- the
    // first hit found inside it; t_range nullptr ((0.001, MAXFLOAT) for every ray) or 2 floats per
    // ray {t_min, t_max} in units of the direction's length.  ORT_QUERY_DRAWN is the call above and
    // takes no t_range.
    int traceRays(const ort_ray* rays, int64_t n, ort_ray_hit* hits, float* normals, int mode, const float* t_range);
    // Segment visibility: out[i] = 1 when a sphere lies strictly between the points a[3 i ..] and
    // b[3 i ..], else 0 -- one ORT_QUERY_ANY ray per pair from a along the unit direction with the
    // interval (eps, |b - a| - eps), formed in float32; a pair no further apart than 2 eps is not
    // occluded.
    int occluded(const float* a, const float* b, int64_t n, uint8_t* out, float eps = 1e-3f);
    // Camera queries (include/ort.h ort_trace_camera): for every pixel of the tile of cam's frame
    // (cfg's size, samples and walk) the camera ray the frame is drawn with and what it hits --
    // query.rays, .hits, .normals and .which as ort_camera_query describes them.  Synchronous;
    // builds and uploads the scene on first use.  Single-device configurations only (a group:
    // ORT_ERR_UNSUPPORTED).
    int traceCamera(const Camera& cam, const ort_tile& tile, const ort_camera_query& query);
    // Radiance queries (include/ort.h ort_trace_radiance): what each of n rays sees in the current
    // scene -- radiance[3 i ..] the mean of `paths` paths of at most maxDepth bounces along ray i,
    // chained through the RNG state states[2 i ..] (each component in [0, 1)) as a pixel's samples
    // are; statesOut (nullptr, or 2 floats per ray, may be == states) the states the chains end
    // with; flags ORT_QUERY_SORT | ORT_RADIANCE_*.  Directions are used as given (unit, or
    // ORT_RADIANCE_NORMALIZE).  By the walk the frames are drawn with (cfg.useOctree).  Host
    // pointers, synchronous; single-device configurations only (a group: ORT_ERR_UNSUPPORTED).
    int traceRadiance(const ort_ray* rays, const float* states, int64_t n, int maxDepth, int paths, float* radiance,
                      float* statesOut = nullptr, int flags = 0);
    // The sphere under pixel (x, y) of cam's frame, by the pinhole ray through the pixel centre
    // (ORT_CAMERA_PIXEL_CENTRE): *hit = {t, sphere index in getSpheres()} ({0, -1}: nothing
    // there), point (may be nullptr) = origin + t * direction.  y is a GL row, 0 at the bottom:
    // for a cursor at window row wy (0 at the top) pass height - 1 - wy.
    int pick(const Camera& cam, int x, int y, ort_ray_hit* hit, float point[3] = nullptr);
    // The interactive loop's frame (include/ort.h ort_accum_*): `samples` more of the frame's
    // cfg.numSamples samples per pixel, then the picture of the samples done so far into rgb (as
    // render(cam, rgb); divided by the samples done, so every call's picture is a frame).  It
    // continues the current accumulation while cam's view, position and zoom are the ones it was
    // begun with, and starts again otherwise; with all samples done the picture is render()'s, bit
    // for bit, and further calls write it again.  samplesDone (may be nullptr) receives the samples
    // in the picture.  Single-device configurations only (a group: ORT_ERR_UNSUPPORTED).
    int renderProgressive(const Camera& cam, int samples, float* rgb, int* samplesDone = nullptr);

    // The guided denoiser for few-sample previews (include/ort.h ort_denoise): filters the tile's
    // picture rgb (tight RGB32F rows, as render and renderProgressive write them) into output, any
    // ort_output with ORT_PLACE_TILE; rgb is host or device memory as output.is_device says, and
    // output.data may be rgb itself.  The guides are cam's pixel-centre camera query of the tile
    // (ORT_CAMERA_PIXEL_CENTRE, normals), traced here.  The tile must be one band
    // (ORT_ERR_INVALID_ARG otherwise); rows with y >= height are neither filtered nor used as taps
    // and come out as render writes them (zeros), as in Renderer.denoise.  Synchronous; single-device configurations only (a
    // group: ORT_ERR_UNSUPPORTED).
    int denoise(const Camera& cam, const ort_tile& tile, const float* rgb, const ort_output& output,
                const DenoiseOptions& options = {});
    // The camera at rest (include/ort.h ort_accum_begin_ex, ort_accum_read_moments, ort_denoise_ex):
    // with setProgressiveMoments(true) renderProgressive's accumulation also keeps each pixel's
    // second luminance moment (the switch starts the accumulation again); readMoments writes the
    // linear mean (nullptr, or width * height * 3 floats) and the variance of its luminance (nullptr,
    // or width * height floats; -1: no estimate) of the samples done so far, host memory or, with
    // onDevice, device memory; and this denoise filters such a mean guided by that variance
    // (nullptr: the term off) -- taps further than sigmaVariance standard deviations add nothing --
    // and, with gamma, writes pow(result, 1/2.2), the display picture.  variance lives where rgb does.
    void setProgressiveMoments(bool on);
    int readMoments(float* mean, float* variance, bool onDevice = false);
    int denoise(const Camera& cam, const ort_tile& tile, const float* rgb, const float* variance, float sigmaVariance,
                bool gamma, const ort_output& output, const DenoiseOptions& options = {});

    // The moving camera (include/ort.h ort_history_update): reprojects the history of the tile's
    // pixels into cam's frame and blends the frame's LINEAR sample picture rgb (tight RGB32F rows:
    // readMoments' mean, traceRadiance without gamma) in; outColor (nullptr, or 3 floats per pixel)
    // receives the integrated colour and outVariance (nullptr, or 1 float per pixel; -1: no estimate)
    // the variance of its luminance, both for denoise(cam, tile, outColor, outVariance, ..., gamma).
    // The guides are cam's pixel-centre camera query of the tile, traced here.  The history is begun
    // by the first call and begun again when the tile's width or rows change; resetHistory makes the
    // next call a first frame.  Host pointers, synchronous; single-device configurations only (a
    // group: ORT_ERR_UNSUPPORTED).
    static constexpr float kHistoryAlpha = 0.1f, kHistoryDepthTolerance = 0.1f;  // as Renderer's History.update
    int reproject(const Camera& cam, const ort_tile& tile, const float* rgb, float* outColor, float* outVariance,
                  float alpha = kHistoryAlpha, float depthTolerance = kHistoryDepthTolerance);
    void resetHistory();
    // The moving scene (include/ort.h ort_history_update_ex, ORT_HISTORY_MOTION): with
    // setHistoryMotion(true) reproject's history survives moveSpheres -- sphere k stays sphere k --
    // and a pixel's surface point is moved back with its sphere before it is projected, a resting
    // camera included (the switch alone changes no picture: nothing has moved).  moveSpheres gives
    // the n spheres indices[i] of getSpheres() the centre and radius centerRadius[4 i ..], builds the
    // octree again (cfg.gpuBuild: on the device) and replaces the resident scene; an accumulation of
    // renderProgressive starts again.  The animated loop per frame: moveSpheres, one-sample picture,
    // reproject, denoise.  Single-device configurations only (a group: ORT_ERR_UNSUPPORTED).
    void setHistoryMotion(bool on);
    int moveSpheres(const int* indices, const float* centerRadius, int n);

    // Adaptive sampling (include/ort.h ort_accum_render_adaptive): with setProgressiveAdaptive(true, ...)
    // renderProgressive's accumulation keeps a sample count per pixel (and the moments; the switch
    // starts the accumulation again) and each call traces `samples` more samples only of the pixels
    // that hold fewer than minSamples or whose mean luminance's standard error is still above
    // threshold x max(luminance, luminanceFloor); every pixel is shown at its own count, and
    // samplesDone is then the largest count a pixel can have.  readSampleCounts writes width *
    // height counts (host memory or, with onDevice, device memory); pendingPixels is the number of
    // pixels the next call would trace (-1: no adaptive accumulation yet, or an error) -- the loop of
    // a camera at rest ends when it is 0.  readMoments gives every pixel's mean and variance at its own count.
    void setProgressiveAdaptive(bool on, float threshold = 0.02f, int minSamples = 4, float luminanceFloor = 0.05f);
    int readSampleCounts(int32_t* counts, bool onDevice = false);
    long long pendingPixels();

    Camera camera;  // the reference keeps a global Camera (src/main.cpp:18); pose set like main()
    const RaytracerConfig& config() const { return cfg; }
    const std::vector<Sphere>& getSpheres() const { return spheres; }
    const Octree& getOctree() const { return octree; }
    const std::vector<double>& getRenderTimes() const { return renderTimes; }
    const char* lastError() const;

    // The saveStats row for these frame times (seconds), without the newline: the reference's
    // 15 ';'-separated columns (src/raytracer.cpp:441-446: useOctree, numSpheres, maxDepth,
    // maxSpheresPerNode, numSamples, maxRaysDepth, width, height, min, max, avg, minFPS,
    // maxFPS, fpsAvg, buildTime) after its 2.5-sigma z-score filter (:372-434), then, when
    // `work` is given, mrays_per_s (traversals / avg frame time), bytes_per_ray (algorithmic
    // reference-layout bytes / traversal), ref_layout_bytes_frac (mrays_per_s x bytes_per_ray /
    // 8 TB/s: the bytes the REFERENCE's record layout would move at this ray rate, SURVEY.md
    // 8(d)'s algorithmic figure -- not a roofline: it exceeds 1 because the compact layout never
    // reads the reference's child records; bench.py reports the measured VALU-issue roofline),
    // gpus, host_cores.  buildSeconds: Octree::buildTime, the root box + subdivision like the
    // reference's column (its flatten excluded), or with gpuBuild the GPU builder's device time
    // (one pass, the layout included: there is no separate flatten to leave out).
    // Returns "" for no frames.
    static std::string statsRow(const RaytracerConfig& cfg, const std::vector<double>& frameSeconds,
                                double buildSeconds, const StatsWork* work);

private:
    RaytracerConfig cfg;
    int width, height;
    ort_ctx* ctx;
    ort_group* group = nullptr;    // cfg.devices.size() > 1
    bool sceneReady;
    std::vector<Sphere> spheres;
    Octree octree;
    std::string statsFilename;
    int frameCount;
    std::vector<double> renderTimes;
    std::vector<float> frame;
    float* dframe = nullptr;       // run()'s device frame (readback off), on the context's device
    void* dguides = nullptr;       // denoise's guides for device pictures (20 bytes a pixel, grow-only)
    size_t dguidesBytes = 0;
    int renderRun();               // one frame of run(): into dframe, or into `frame` with readback
    ort_accum* accum = nullptr;    // renderProgressive's accumulation (the context owns it) and its camera
    ort_params accumParams{};
    ort_history* history = nullptr;  // reproject's history (the context owns it) and its shape
    int historyWidth = 0, historyRows = 0;
    bool historyMotion = false;    // setHistoryMotion
    bool accumMoments = false;     // setProgressiveMoments
    bool accumAdaptive = false;    // setProgressiveAdaptive and its criterion
    float adaptiveThreshold = 0.02f, adaptiveFloor = 0.05f;
    int adaptiveMinSamples = 4;
    ort_accum_adaptive adaptiveCriterion(int samples) const;
    double gpuBuildSeconds = 0.0;
    StatsWork work;               // counted after the timed frames when cfg.extendedStats

    void setupScene();
    void setupBuffers();
    void cleanupBuffers();
    std::vector<Sphere> generateSpheres();
    std::vector<Sphere> generatePreBuiltSpheres();
    std::vector<Sphere> generateRandomSpheres();
    void saveStats();
    bool countWork();
    ort_params frameParams(const Camera& cam) const;
};
