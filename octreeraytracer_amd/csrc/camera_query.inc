// camera_query.inc -- camera queries (ort_trace_camera): per tile pixel the camera ray the shader
// makes for it and what that ray hits, {ray, t, sphere[, normal]} records.
// Included by ort_kernel.hip after ray_query.inc (its kernels follow the query kernels in the code
// object, whose code is unchanged).  ort_camera_lane is ray_query.inc's query_lane_body over
// CameraSource; ort_camera_rays keeps its own copy of the loop (see there).  The host side is ray_query.inc's staging (query_begin / query_start /
// query_finish) and state (ort_ctx::query).
//   ort_camera_rays<DEEP>  compact layout: at refill a lane makes its pixel's ray in registers
//                          instead of loading a caller's
//   ort_camera_exact       the literal exact walk of the deferred pixels (the ray made again)
//   ort_camera_lane<MODE>  explicit layout (1) and brute force (2): one pixel per lane
//   ort_camera_gen         ray generation only (hits == NULL): a plain grid
// The work item is the record index: output row j x tile width + column, so consecutive items are
// row runs (a wave's 64 items one run of 64 pixels where the tile is that wide) and a wave's
// records and rays are stored side by side.

namespace {

struct CameraArgs {
    QueryArgs q;        // scene, hits, normals, defer list, counters, n = tile pixels (rays, qlist: unused)
    ort::PixelParams pp;  // the full frame's camera, W, H, ns (maxDepth: not read)
    TileMap tm;
    float* rays_out;    // 6 floats per tile pixel, or null (wave-uniform)
    int which;          // ORT_CAMERA_*
};

// ORT_CAMERA_PIXEL_CENTRE: Camera_getRay (glsl:205-221) at s = (x + 0.5) / W, t = (y + 0.5) / H with
// the jitter and the lens offset left out, then radiance()'s normalize (glsl:602): no RNG draw.
ORT_FN ort::Ray pixel_centre_ray(const ort::PixelParams& P, int px, int py) {
    const ort::KCamera& c = P.cam;
    const float a = ((float)px + 0.5f) / (float)P.W, b = ((float)py + 0.5f) / (float)P.H;
    ort::Ray r;
    r.o = c.origin;
    r.d = ort::normalize(ort::mk(((c.lowerLeft.x + a * c.horizontal.x) + b * c.vertical.x) - c.origin.x,
                                 ((c.lowerLeft.y + a * c.horizontal.y) + b * c.vertical.y) - c.origin.y,
                                 ((c.lowerLeft.z + a * c.horizontal.z) + b * c.vertical.z) - c.origin.z));
    r.d = ort::normalize(r.d);
    return r;
}

// The ray of frame pixel (px, py): ORT_CAMERA_FIRST_SAMPLE is main()'s prologue and sample 0 up to
// radiance()'s first line, the ray the render kernels walk first (pixel_rng_init, primary_ray).
ORT_FN ort::Ray camera_query_ray(const ort::PixelParams& P, int px, int py, int which) {
    if (which == ORT_CAMERA_PIXEL_CENTRE) return pixel_centre_ray(P, px, py);
    ort_rng st;
    ort::pixel_rng_init(P, px, py, st);
    return ort::primary_ray(P, px, py, 0, st);
}

// Work item i -> its ray; false for a row past the frame (band padding, a tile reaching below
// height): the caller writes the empty record.
__device__ inline bool camera_item_ray(const CameraArgs& A, int i, ort::Ray& ray) {
    const int row = i / A.tm.tw, col = i - row * A.tm.tw;
    const int y = tile_row_to_y(A.tm, row);
    if (y >= A.pp.H) return false;
    ray = camera_query_ray(A.pp, A.tm.x0 + col, y, A.which);
    return true;
}

__device__ inline void camera_store_ray(const CameraArgs& A, int i, const ort::Ray& ray) {
    float* p = A.rays_out + 6 * (size_t)i;
    p[0] = ray.o.x;
    p[1] = ray.o.y;
    p[2] = ray.o.z;
    p[3] = ray.d.x;
    p[4] = ray.d.y;
    p[5] = ray.d.z;
}

// A row past the frame: the miss record, a zero normal, a zero ray.
__device__ inline void camera_store_empty(const CameraArgs& A, int i) {
    ort::Ray zero;
    zero.o = ort::mk(0.0f, 0.0f, 0.0f);
    zero.d = ort::mk(0.0f, 0.0f, 0.0f);
    if (A.rays_out) camera_store_ray(A, i, zero);
    if (A.q.hits) query_store(A.q, i, ort::query_hit<0>(A.q.S, zero, false, 0.0f, -1, false));
}

// The camera's pixels as ray_query.inc's item source: the work item is the record index, the ray
// is made in registers and stored only where the caller asked for rays; a row past the frame gets
// its empty record here.
struct CameraSource {
    const CameraArgs& A;
    __device__ __forceinline__ int index(int pos) const { return pos; }
    __device__ __forceinline__ bool item(int i, ort::Ray& ray) const {
        if (!camera_item_ray(A, i, ray)) {
            camera_store_empty(A, i);
            return false;
        }
        if (A.rays_out) camera_store_ray(A, i, ray);
        return true;
    }
};

// NOT folded into ray_query.inc's query_item_loop: over CameraSource with FastQueryWalk the compiler
// spills more (104-124 B of scratch against this body's 100 B at the same 80 VGPRs:
// profiles/query_refactor/resource_usage.md), so this kernel keeps its own copy of the loop --
// ort_query_rays' with the ray made at refill: the same chunks, refill threshold, leaf hold and walk
// configuration.  A change to query_item_loop is made here too.  The ray lives in registers from
// camera_item_ray to fast_begin and is stored only where the caller asked for rays; the walk state
// gives it back for the record (st.ray()).
template <bool DEEP>
__global__ void __launch_bounds__(DEEP ? kPersistDeepBlock : kBlock) __attribute__((amdgpu_waves_per_eu(ORT_PERSISTENT_WAVES)))
ort_camera_rays(CameraArgs A) {
    extern __shared__ __attribute__((aligned(4096))) unsigned char query_smem[];
    unsigned char* const smem = query_smem;
    constexpr bool REV = DEEP && kRevBounce;
    LdsView L = setup_lds<true, DEEP ? kPersistDeepBlock : kBlock, REV>(smem, A.q.S);
    const uint8_t* lut = L.lut;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    ort::Counters cnt;  // (fast_step's COUNT = false: unused)
    for (int q = 0; q < 6; ++q) cnt.v[q] = 0;
    using Masks = typename std::conditional<DEEP, ort::Masks96Lean, ort::Masks64Plain>::type;
    ort::FastStateT<Masks> st;
    int k = -1;              // the lane's pixel (record index), -1 idle
    int next = 0, end = 0;   // wave-uniform: remaining work items [next, end) of the wave's chunk
    bool drained = false;    // wave-uniform: the global cursor passed the item count
    const int total = A.q.n;
#if ORT_CHUNK_ADAPT
    const int chunk = total >= (int)(gridDim.x * (blockDim.x >> 6)) * ORT_CHUNK_ADAPT ? 2 * kChunk : kChunk;
#else
    constexpr int chunk = kChunk;
#endif
    const bool want_normal = A.q.normals != nullptr;
    for (;;) {
        const unsigned long long idle = __ballot(k < 0);
        const int n_idle = __popcll(idle);
        if (n_idle == 64 && drained) break;
        if (!drained && n_idle >= A.q.refill) {
            if (next == end) {
                int base = 0;
                if (lane == 0) base = atomicAdd(A.q.sync + 1, chunk);
                base = __shfl(base, 0);
                if (base >= total) {
                    drained = true;
                    continue;
                }
                next = base;
                end = min(base + chunk, total);
            }
            const int take = min(n_idle, end - next);
            if (k < 0) {
                const int rank = __popcll(idle & below);
                if (rank < take) {
                    const int cand = next + rank;
                    ort::Ray ray;
                    if (!camera_item_ray(A, cand, ray)) {
                        camera_store_empty(A, cand);
                    } else {
                        if (A.rays_out) camera_store_ray(A, cand, ray);
                        ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
                        if (A.q.exact_only || !ort::fast_prepare(A.q.S, ray, inv)) {
                            A.q.defer_list[atomicAdd(A.q.sync, 1)] = cand;
                        } else if (ort::fast_begin(A.q.S, L.planes, lut, ray, inv, 0.001f, ORT_MAXFLOAT, st)) {
                            k = cand;
                        } else {  // misses the root box
                            query_store(A.q, cand, ort::query_hit<0>(A.q.S, ray, false, 0.0f, -1, false));
                        }
                    }
                }
            }
            next += take;
            continue;
        }
#if ORT_LEAF_HOLD
        bool hold = false;
        if (DEEP) {
            const bool at_leaf = k >= 0 && !(st.rec.y & ORT_INTERNAL_FLAG);
            const unsigned long long lm = __ballot(at_leaf), im = __ballot(k >= 0 && !at_leaf);
            hold = at_leaf && __popcll(im) >= ORT_LEAF_HOLD_MIN_INTERNAL && __popcll(lm) < ORT_LEAF_HOLD;
        }
        if (k >= 0 && !hold) {
#else
        if (k >= 0) {
#endif
            if (ort::fast_step<false>(A.q.S, lut, st, L.fr, cnt)) {
                query_store(A.q, k, ort::query_hit<0>(A.q.S, st.ray(), st.hit(), st.closest, st.hitEntry, want_normal));
                k = -1;
            }
        }
    }
}

// The exact compact walk of the deferred pixels, each ray made again from its pixel; grid-stride.
__global__ void __launch_bounds__(kBlock) ort_camera_exact(CameraArgs A) {
    extern __shared__ __attribute__((aligned(4096))) unsigned char query_smem[];
    unsigned char* const smem = query_smem;
    const int n = *A.q.sync;
    if ((int)(blockIdx.x * kBlock) >= n) return;  // usually no deferred pixel: no LDS image copy
    LdsView L = setup_lds<false>(smem, A.q.S);
    const bool want_normal = A.q.normals != nullptr;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int k = A.q.defer_list[i];
        ort::Ray ray;
        if (!camera_item_ray(A, k, ray)) continue;  // (never deferred: stored at refill)
        query_store(A.q, k, ort::query_ray<0>(A.q.S, L.planes, nullptr, nullptr, ray, L.fr, nullptr, nullptr, want_normal));
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) ort_camera_lane(CameraArgs A) {
    query_lane_body<MODE>(A.q, CameraSource{A}, [&](const ort::Ray& ray, int, ort::LocalFrames& lf, int* snode, float* stmin, bool want_normal) {
        return ort::query_ray<MODE>(A.q.S, nullptr, nullptr, nullptr, ray, lf, snode, stmin, want_normal);
    });
}

// Ray generation only: nothing is walked, no scene is read (A.q.hits is null).
__global__ void __launch_bounds__(kBlock) ort_camera_gen(CameraArgs A) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.q.n) return;
    ort::Ray ray;
    if (!camera_item_ray(A, (int)i, ray)) {
        camera_store_empty(A, (int)i);
        return;
    }
    camera_store_ray(A, (int)i, ray);
}

std::string check_camera_query(const ort_params* p, const ort_tile* t, const ort_camera_query* q) {
    const std::string bad = check_params(p, t);  // what ort_render refuses, with its code
    if (!bad.empty()) return bad;
    if (!q) return "null query";
    if (q->which != ORT_CAMERA_FIRST_SAMPLE && q->which != ORT_CAMERA_PIXEL_CENTRE) return "which: unknown ORT_CAMERA_*";
    if (q->reserved[0] != 0 || q->reserved[1] != 0) return "reserved must be 0";
    if (!q->rays && !q->hits) return "rays and hits are both null";
    if (q->normals && !q->hits) return "normals need hits";
    if (((uintptr_t)q->rays & 3) || ((uintptr_t)q->hits & 3) || ((uintptr_t)q->normals & 3))
        return "rays, hits and normals must be 4-byte aligned";
    if ((long long)t->width * (long long)t->rows > kQueryMaxRays) return "a tile of at most 2^30 pixels";
    return "";
}

int camera_impl(ort_ctx* ctx, const ort_params* p, const ort_tile* t, const ort_camera_query* q, void* stream) {
    const std::string bad = check_camera_query(p, t, q);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_trace_camera: " + bad);
    const bool walk = q->hits != nullptr;
    QueryCall c;
    CameraArgs a;
    std::memset(&a, 0, sizeof(a));
    const QueryIo io = {nullptr, q->rays, q->hits, q->normals, q->on_device != 0, false, true};
    int rc = query_begin(ctx, "ort_trace_camera", walk, p->use_octree, (size_t)t->width * (size_t)t->rows, io, stream, c, a.q);
    if (rc || c.n == 0) return rc;
    a.pp = pixel_params(p);
    a.tm = {t->x0, t->width, t->y0, t->rows, t->band_height, t->band_stride};
    a.rays_out = q->rays ? (c.host ? (float*)ctx->query.rays.p : (float*)q->rays) : nullptr;
    a.which = q->which;
    if ((rc = query_start(ctx, c, a.q))) return rc;
    hipError_t e;
    if (!walk) {
        hipLaunchKernelGGL(ort_camera_gen, dim3((unsigned)c.blocks), dim3(kBlock), 0, c.s, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_camera_gen launch");
    } else if (c.mode == 0) {
        if ((rc = launch_fast_walk(ctx, c, a, ort_camera_rays<true>, ort_camera_rays<false>, ort_camera_exact, "ort_camera"))) return rc;
    } else {
        pick<1, 2>(c.mode, [&](auto MODE) {
            hipLaunchKernelGGL((ort_camera_lane<ORT_V(MODE)>), dim3((unsigned)c.blocks), dim3(kBlock), 0, c.s, a);
        });
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_camera_lane launch");
    }
    return query_finish(ctx, c);
}

}  // namespace

extern "C" {

int ort_trace_camera(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, const ort_camera_query* q, void* stream) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_trace_camera: null ctx");
    return camera_impl(ctx, params, tile, q, stream);
}

#if ORT_ANALYSIS
// TEST-ONLY host emulation (ort_internal.h): camera_query_ray for every tile pixel, then
// ort_debug_query_rays (query_ray) over the rays of the pixels inside the frame.
int ort_debug_camera_query(const float* cr, int32_t n_spheres, const float* node_min, const float* node_max,
                           const int32_t* co, const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx,
                           int64_t n_indices, int32_t layout, const ort_params* p, const ort_tile* t, int32_t which,
                           float* rays, ort_ray_hit* hits, float* normals) {
    try {
        ort_camera_query q;
        std::memset(&q, 0, sizeof(q));
        q.rays = (ort_ray*)rays;
        q.hits = hits;
        q.normals = normals;
        q.which = which;
        const std::string bad = check_camera_query(p, t, &q);
        if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_camera_query: " + bad);
        const ort::PixelParams pp = pixel_params(p);
        const TileMap tm = {t->x0, t->width, t->y0, t->rows, t->band_height, t->band_stride};
        const size_t n = (size_t)t->width * (size_t)t->rows;
        std::vector<float> made;   // the rays of the pixels inside the frame, in record order
        std::vector<size_t> where;  // their record indices
        made.reserve(6 * n);
        where.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            const int row = (int)(i / (size_t)tm.tw), col = (int)(i % (size_t)tm.tw);
            const int y = tile_row_to_y(tm, row);
            float r6[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (y < pp.H) {
                const ort::Ray ray = camera_query_ray(pp, tm.x0 + col, y, which);
                const float v[6] = {ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z};
                std::memcpy(r6, v, sizeof v);
                made.insert(made.end(), v, v + 6);
                where.push_back(i);
            }
            if (rays) std::memcpy(rays + 6 * i, r6, sizeof r6);
            if (hits) {
                hits[i].t = 0.0f;
                hits[i].sphere = -1;
            }
            if (normals) normals[3 * i] = normals[3 * i + 1] = normals[3 * i + 2] = 0.0f;
        }
        if (!hits || where.empty()) return ORT_OK;
        std::vector<ort_ray_hit> h(where.size());
        std::vector<float> nrm(normals ? 3 * where.size() : 0);
        const int rc = ort_debug_query_rays(cr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, layout,
                                            p->use_octree == 1 ? 1 : 0, made.data(), (int64_t)where.size(), h.data(),
                                            normals ? nrm.data() : nullptr);
        if (rc != ORT_OK) return rc;
        for (size_t k = 0; k < where.size(); ++k) {
            hits[where[k]] = h[k];
            if (normals) std::memcpy(normals + 3 * where[k], nrm.data() + 3 * k, 12);
        }
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}
#endif  // ORT_ANALYSIS

}  // extern "C"
