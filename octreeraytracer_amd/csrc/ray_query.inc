// ray_query.inc -- ray queries (ort_trace_rays): caller rays -> {t, sphere[, normal]} records, and
// what every query shares (camera_query.inc, ray_modes.inc): QueryArgs, the record store, the one
// persistent item loop (query_item_loop) with its item sources and walks, the lane body, and the
// host staging (query_begin / query_start / query_finish, query_sort).
// Included by ort_kernel.hip after the render path (its kernels follow the render kernels in the
// code object, whose code is unchanged); shares ort_ctx, the LDS image and the walks.
//   ort_query_rays<DEEP>   compact layout: query_item_loop over the caller's rays with the fast walk;
//                          rays the fast walk cannot take go to a defer list
//   ort_query_exact        the literal exact walk of the deferred rays
//   ort_query_lane<MODE>   explicit layout (1) and brute force (2): one ray per lane
//   k_query_keys           ORT_QUERY_SORT: the coherence key of every ray (path_key.h)
// A query owns its buffers (ort_ctx::query) and its cursor and defer counters: it reads the scene
// and writes the caller's records, nothing of the per-frame pipeline state.

namespace {

struct QueryArgs {
    ort::KScene S;
    const float* rays;   // 6 floats per ray (ort_ray): origin, direction
    int2* hits;          // per ray {t bits, sphere} (ort_ray_hit); 4-byte aligned
    float* normals;      // 3 floats per ray, or null (wave-uniform: tested like the output format)
    const int* qlist;    // ORT_QUERY_SORT: work item -> ray index, or null = the index itself
    int* defer_list;
    int* sync;           // [0] deferred count, [1] work cursor
    int n;               // rays
    int refill;          // ORT_OPT_REFILL
    int exact_only;      // ORT_OPT_EXACT_TRAVERSAL, or an unordered tree
};

__device__ inline ort::Ray query_load_ray(const QueryArgs& A, int i) {
    const float* p = A.rays + 6 * (size_t)i;
    ort::Ray r;
    r.o = ort::mk(p[0], p[1], p[2]);
    r.d = ort::mk(p[3], p[4], p[5]);
    return r;
}

// The record as one 8-byte store (dword-aligned, as the ABI promises no more), the normal only
// where asked.
struct __attribute__((packed, aligned(4))) QueryRecord {
    int t, sphere;
};
__device__ inline void query_store(const QueryArgs& A, int i, const ort::RayHit& q) {
    QueryRecord rec;
    rec.t = __float_as_int(q.t);
    rec.sphere = q.sphere;
    *reinterpret_cast<QueryRecord*>(A.hits + (size_t)i) = rec;
    if (A.normals) {
        float* nrm = A.normals + 3 * (size_t)i;
        nrm[0] = q.normal.x;
        nrm[1] = q.normal.y;
        nrm[2] = q.normal.z;
    }
}

__device__ inline void query_store_miss(const QueryArgs& Q, int i, const ort::Ray& ray) {
    query_store(Q, i, ort::query_hit<0>(Q.S, ray, false, 0.0f, -1, false));
}

// ---- item sources: work item -> (record index, ray) -------------------------------------------
//   index(pos)    the record a work item stands for
//   item(i, ray)  record i's ray; false = handled here, nothing to walk
// The caller's rays, through the sorted list where there is one.  (camera_query.inc: CameraSource.)
struct RaySource {
    const QueryArgs& Q;
    __device__ __forceinline__ int index(int pos) const { return Q.qlist ? Q.qlist[pos] : pos; }
    __device__ __forceinline__ bool item(int i, ort::Ray& ray) const {
        ray = query_load_ray(Q, i);
        return true;
    }
};

// ---- walks: begin(i, ray, k) at refill (k = i where the lane now walks), held(walking), step()
// until done, finish(i) the record.  kAdaptChunk: ORT_CHUNK_ADAPT's doubled chunks on long lists.
// The fast walk in the bounce walk's configuration (caller rays are incoherent in general):
// Masks64Plain at depth <= 8, Masks96Lean over the reversed tables at depth 9-10 with its leaf
// hold, the rejected-sphere skip per S.kid / S.nk.  A ray fast_prepare refuses goes to the defer
// list (ort_query_exact, ort_camera_exact); one that misses the root box gets its miss record.
template <bool DEEP>
struct FastQueryWalk {
    static constexpr bool kAdaptChunk = true;  // ORT_CHUNK_ADAPT, as ort_trace_persistent
    static constexpr bool kFast = true;
    using Args = QueryArgs;
    static constexpr int kThreads = DEEP ? kPersistDeepBlock : kBlock;
    const QueryArgs& Q;
    LdsView L;
    const uint8_t* const lut;
    const bool want_normal;
    ort::FastStateT<typename std::conditional<DEEP, ort::Masks96Lean, ort::Masks64Plain>::type> st;
    ort::Counters cnt;  // (fast_step's COUNT = false: unused)
    __device__ __forceinline__ FastQueryWalk(const QueryArgs& q, unsigned char* smem)
        : Q(q), L(setup_lds<true, kThreads, DEEP && kRevBounce>(smem, q.S)), lut(L.lut), want_normal(q.normals != nullptr) {
        for (int c = 0; c < 6; ++c) cnt.v[c] = 0;
    }
    // (begin: spelled in query_item_loop, under kFast)
    // Called by every lane of the wave (two ballots): is this walking lane held at its leaf?
    __device__ __forceinline__ bool held(bool walking) const {
#if ORT_LEAF_HOLD
        if (DEEP) {
            const bool at_leaf = walking && !(st.rec.y & ORT_INTERNAL_FLAG);
            const unsigned long long lm = __ballot(at_leaf), im = __ballot(walking && !at_leaf);
            return at_leaf && __popcll(im) >= ORT_LEAF_HOLD_MIN_INTERNAL && __popcll(lm) < ORT_LEAF_HOLD;
        }
#endif
        return false;
    }
    __device__ __forceinline__ bool step() { return ort::fast_step<false>(Q.S, lut, st, L.fr, cnt); }
    // (the ray back from the walk state, bit-identical: no registers held across the walk)
    __device__ __forceinline__ void finish(int i) const {
        query_store(Q, i, ort::query_hit<0>(Q.S, st.ray(), st.hit(), st.closest, st.hitEntry, want_normal));
    }
};

// The one persistent item loop of the queries -- ort_trace_persistent's (left where it is, with
// its instrumentation): every lane keeps one item's walk state, a wave draws chunks of consecutive
// items from the atomic cursor Q.sync[1] and refills its idle lanes from its chunk, by rank among
// the idle, once Q.refill of them are idle; when the cursor passes Q.n the wave drains.
// block_waves: blockDim.x >> 6, read by the kernel itself (where the compiler folds it to a scalar
// load of the launch's size), for a walk that adapts its chunk to the resident waves.
template <class Source, class Walk>
__device__ __forceinline__ void query_item_loop(const QueryArgs& Q, const Source& src, const typename Walk::Args& WA,
                                                unsigned char* smem, unsigned block_waves) {
    Walk w(WA, smem);  // (the walk's state: a local of this function)
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int k = -1;              // the lane's record index, -1 idle
    int next = 0, end = 0;   // wave-uniform: remaining work items [next, end) of the wave's chunk
    bool drained = false;    // wave-uniform: the global cursor passed the item count
    const int total = Q.n;
    const int chunk = Walk::kAdaptChunk && ORT_CHUNK_ADAPT && total >= (int)(gridDim.x * block_waves) * ORT_CHUNK_ADAPT ? 2 * kChunk : kChunk;
    for (;;) {
        const unsigned long long idle = __ballot(k < 0);
        const int n_idle = __popcll(idle);
        if (n_idle == 64 && drained) break;
        if (!drained && n_idle >= Q.refill) {
            if (next == end) {
                int base = 0;
                if (lane == 0) base = atomicAdd(Q.sync + 1, chunk);
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
                    const int cand = src.index(next + rank);
                    ort::Ray ray;
                    if (src.item(cand, ray)) {
                        if constexpr (Walk::kFast) {
                            // FastQueryWalk's begin, spelled here: called as a member it cost ort_query_rays a
                            // register and 28-48 B of scratch (profiles/query_refactor/resource_usage.md)
                            ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
                            if (Q.exact_only || !ort::fast_prepare(Q.S, ray, inv)) {
                                Q.defer_list[atomicAdd(Q.sync, 1)] = cand;
                            } else if (ort::fast_begin(Q.S, w.L.planes, w.lut, ray, inv, 0.001f, ORT_MAXFLOAT, w.st)) {
                                k = cand;
                            } else {  // misses the root box
                                query_store_miss(Q, cand, ray);
                            }
                        } else {
                            w.begin(cand, ray, k);
                        }
                    }
                }
            }
            next += take;
            continue;
        }
        const bool hold = w.held(k >= 0);
        if (k >= 0 && !hold && w.step()) {
            w.finish(k);
            k = -1;
        }
    }
}

// One record per lane: the explicit layout's literal 200-entry stack walk (MODE 1), brute force
// (2).  trace(ray, i, frames, snode, stmin, want_normal) is the entry point's query of one ray.
template <int MODE, class Source, class Trace>
__device__ __forceinline__ void query_lane_body(const QueryArgs& Q, const Source& src, Trace trace) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= Q.n) return;
    ort::Ray ray;
    if (!src.item((int)i, ray)) return;
    const bool want_normal = Q.normals != nullptr;
    ort::LocalFrames unused;
    if constexpr (MODE == 1) {
        int snode[ORT_MAX_STACK];
        float stmin[ORT_MAX_STACK];
        query_store(Q, (int)i, trace(ray, (int)i, unused, snode, stmin, want_normal));
    } else {
        query_store(Q, (int)i, trace(ray, (int)i, unused, nullptr, nullptr, want_normal));
    }
}

template <bool DEEP>
__global__ void __launch_bounds__(DEEP ? kPersistDeepBlock : kBlock) __attribute__((amdgpu_waves_per_eu(ORT_PERSISTENT_WAVES)))
ort_query_rays(QueryArgs A) {
    // (the queries' own symbol: the render kernels' dynamic LDS symbol keeps its alignment)
    extern __shared__ __attribute__((aligned(4096))) unsigned char query_smem[];
    query_item_loop<RaySource, FastQueryWalk<DEEP>>(A, RaySource{A}, A, query_smem, blockDim.x >> 6);
}

// The exact compact walk (traverse_compact through query_ray) of the deferred rays; grid-stride.
__global__ void __launch_bounds__(kBlock) ort_query_exact(QueryArgs A) {
    extern __shared__ __attribute__((aligned(4096))) unsigned char query_smem[];  // plane tables: 1 KiB-aligned at least
    unsigned char* const smem = query_smem;
    const int n = *A.sync;
    if ((int)(blockIdx.x * kBlock) >= n) return;  // usually few deferred rays: no LDS image copy
    LdsView L = setup_lds<false>(smem, A.S);
    const bool want_normal = A.normals != nullptr;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int k = A.defer_list[i];
        const ort::Ray ray = query_load_ray(A, k);
        query_store(A, k, ort::query_ray<0>(A.S, L.planes, nullptr, nullptr, ray, L.fr, nullptr, nullptr, want_normal));
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) ort_query_lane(QueryArgs A) {
    query_lane_body<MODE>(A, RaySource{A}, [&](const ort::Ray& ray, int, ort::LocalFrames& lf, int* snode, float* stmin, bool want_normal) {
        return ort::query_ray<MODE>(A.S, nullptr, nullptr, nullptr, ray, lf, snode, stmin, want_normal);
    });
}

// ORT_QUERY_SORT: (coherence key, ray index) of every ray.  A ray with a component that is not
// finite gets key 0: the key's table lookups are only for finite coordinates, and the order
// never changes a record.
__global__ void __launch_bounds__(kBlock) k_query_keys(QueryArgs A, ort::MortonPlan mp, const uint32_t* spread,
                                                       uint32_t* keys, int* vals) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < A.n; i += (long long)gridDim.x * kBlock) {
        const ort::Ray r = query_load_ray(A, (int)i);
        const bool finite = fabsf(r.o.x) <= ORT_MAXFLOAT && fabsf(r.o.y) <= ORT_MAXFLOAT && fabsf(r.o.z) <= ORT_MAXFLOAT &&
                            fabsf(r.d.x) <= ORT_MAXFLOAT && fabsf(r.d.y) <= ORT_MAXFLOAT && fabsf(r.d.z) <= ORT_MAXFLOAT;
        keys[i] = finite ? ort::path_key(make_float4(r.o.x, r.o.y, r.o.z, 0.0f), make_float4(r.d.x, r.d.y, r.d.z, 0.0f), mp, spread)
                         : 0u;
        vals[i] = (int)i;
    }
}

constexpr long long kQueryMaxRays = 1ll << 30;

std::string check_query(const ort_ray_query* q) {
    if (!q) return "null query";
    if (q->n_rays < 0 || q->n_rays > kQueryMaxRays) return "n_rays must be 0 .. 2^30";
    if (q->flags & ~ORT_QUERY_SORT) return "unknown flag bits";
    if (q->reserved != 0) return "reserved must be 0";
    if (q->n_rays > 0 && (!q->rays || !q->hits)) return "null rays or hits";
    if (((uintptr_t)q->rays & 3) || ((uintptr_t)q->hits & 3) || ((uintptr_t)q->normals & 3))
        return "rays, hits and normals must be 4-byte aligned";
    return "";
}

// ---- host staging: what ort_trace_rays, ort_trace_rays_ex and ort_trace_camera share ---------------
// The caller's arrays of one call (null: not asked for), host or device memory.
struct QueryIo {
    const void* rays_in;  // the caller's rays
    void* rays_out;       // the rays the call makes (ort_trace_camera)
    void* hits;
    float* normals;
    bool on_device;
    bool sort;            // ORT_QUERY_SORT (applies on the compact layout)
    bool defer;           // the call's compact kernel defers records to an exact walk
};

struct QueryCall {
    hipStream_t s;
    bool caller_stream, host, sort;
    int mode;     // 0 compact, 1 explicit, 2 brute force
    size_t n;     // records; 0: nothing to launch (query_begin returned ORT_OK)
    long long blocks;
    QueryIo io;
};

// Scene and mode (walk: the call reads the scene), device and stream, the counters, the defer list
// and the staged arrays a host call needs, ORT_QUERY_SORT's buffers, the events, the common
// QueryArgs, the rays' upload.
int query_begin(ort_ctx* ctx, const char* who, bool walk, int use_octree, size_t n, const QueryIo& io, void* stream,
                QueryCall& c, QueryArgs& a) {
    c = QueryCall{};
    c.mode = 2;
    if (walk) {
        if (!ctx->scene.has_scene) return fail(ctx, ORT_ERR_NO_SCENE, std::string(who) + ": no scene uploaded");
        c.mode = (use_octree == 1) ? (ctx->scene.layout == ORT_LAYOUT_COMPACT ? 0 : 1) : 2;
        if (c.mode != 2 && ctx->scene.n_nodes <= 0) return fail(ctx, ORT_ERR_NO_SCENE, std::string(who) + ": scene has no octree");
    }
    if (n == 0) return ORT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    QueryState& q = ctx->query;
    c.s = stream ? (hipStream_t)stream : ctx->stream;
    c.caller_stream = stream != nullptr;
    c.host = !io.on_device;
    c.sort = c.mode == 0 && io.sort;
    c.blocks = ((long long)n + kBlock - 1) / kBlock;
    c.io = io;
    int rc;
    if ((rc = ensure(ctx, q.sync, 64))) return rc;
    if (walk && c.mode == 0 && io.defer && (rc = ensure(ctx, q.defer, 4 * n))) return rc;
    if (c.host && (((io.rays_in || io.rays_out) && (rc = ensure(ctx, q.rays, sizeof(ort_ray) * n))) ||
                   (io.hits && (rc = ensure(ctx, q.hits, sizeof(ort_ray_hit) * n))) ||
                   (io.normals && (rc = ensure(ctx, q.normals, 12 * n)))))
        return rc;
    if (c.sort && ((rc = ensure(ctx, q.keys, 4 * n)) || (rc = ensure(ctx, q.keys2, 4 * n)) || (rc = ensure(ctx, q.vals, 4 * n)) ||
                   (rc = ensure(ctx, q.list, 4 * n)) ||
                   (rc = ensure(ctx, q.temp, std::max<size_t>(ort::sortAliveTempBytes((int)n), 16))) || (rc = ensure_key_spread(ctx))))
        return rc;
    HIPCHK(ctx, q.ev.create());
    std::memset(&a, 0, sizeof(a));
    if (walk) {
        a.S = device_scene(ctx);
        a.hits = c.host ? (int2*)q.hits.p : (int2*)io.hits;
        a.normals = io.normals ? (c.host ? (float*)q.normals.p : io.normals) : nullptr;
        a.defer_list = (int*)q.defer.p;
    }
    a.rays = io.rays_in ? (c.host ? (const float*)q.rays.p : (const float*)io.rays_in) : nullptr;
    a.sync = (int*)q.sync.p;
    a.n = (int)n;
    a.refill = ctx->opt.refill;
    a.exact_only = ctx->opt.exact_only || !ctx->scene.ordered;
    if (c.host && io.rays_in) HIPCHK(ctx, hipMemcpyAsync(q.rays.p, io.rays_in, sizeof(ort_ray) * n, hipMemcpyHostToDevice, c.s));
    c.n = n;
    return ORT_OK;
}

// ORT_QUERY_SORT: the key of every ray, one sort of n pairs (the count is known here: no host
// wait), a.qlist = the sorted ray indices.
int query_sort(ort_ctx* ctx, const QueryCall& c, QueryArgs& a) {
    QueryState& q = ctx->query;
    hipError_t e;
    hipLaunchKernelGGL(k_query_keys, dim3((unsigned)std::min<long long>(c.blocks, 2048)), dim3(kBlock), 0, c.s, a,
                       ort::mortonPlan(ctx->scene.root_lo, ctx->scene.root_hi), (const uint32_t*)ctx->pipe.key_spread.p, (uint32_t*)q.keys.p,
                       (int*)q.vals.p);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "k_query_keys launch");
    const ort::SortBuffers sb = {(uint32_t*)q.keys.p, (uint32_t*)q.keys2.p, (int*)q.vals.p, (int*)q.list.p};
    if ((e = ort::sortList(q.temp.p, ort::sortAliveTempBytes((int)c.n), (int)c.n, sb, c.s)) != hipSuccess)
        return hip_fail(ctx, e, "query sort");
    a.qlist = (const int*)q.list.p;
    return ORT_OK;
}

// After the entry point staged its own inputs: the counters' reset, the first timing event, the sort.
int query_start(ort_ctx* ctx, const QueryCall& c, QueryArgs& a) {
    HIPCHK(ctx, hipMemsetAsync(ctx->query.sync.p, 0, 64, c.s));
    HIPCHK(ctx, ctx->query.ev.begin(c.s));
    return c.sort ? query_sort(ctx, c, a) : ORT_OK;
}

// After the entry point's launches: the second event, the copies back.  Host output synchronises;
// device output synchronises only without a caller stream.
int query_finish(ort_ctx* ctx, const QueryCall& c) {
    QueryState& q = ctx->query;
    const size_t n = c.n;
    HIPCHK(ctx, q.ev.end(c.s));
    if (c.host) {
        if (c.io.rays_out) HIPCHK(ctx, hipMemcpyAsync(c.io.rays_out, q.rays.p, sizeof(ort_ray) * n, hipMemcpyDeviceToHost, c.s));
        if (c.io.hits) HIPCHK(ctx, hipMemcpyAsync(c.io.hits, q.hits.p, sizeof(ort_ray_hit) * n, hipMemcpyDeviceToHost, c.s));
        if (c.io.normals) HIPCHK(ctx, hipMemcpyAsync(c.io.normals, q.normals.p, 12 * n, hipMemcpyDeviceToHost, c.s));
    }
    if (c.host || !c.caller_stream) HIPCHK(ctx, hipStreamSynchronize(c.s));
    return ORT_OK;
}

// The compact layout's launches of a query with a fast walk: the persistent kernel (deep: depth
// 9-10) on the resident grid, then the exact walk of what it deferred.  family: "ort_query", "ort_camera".
template <class Args>
int launch_fast_walk(ort_ctx* ctx, const QueryCall& c, const Args& a, void (*deep_k)(Args), void (*flat_k)(Args),
                     void (*exact_k)(Args), const char* family) {
    const bool deep = ctx->scene.depth > 8;
    const int nb = deep ? kPersistDeepBlock : kBlock;
    const size_t lds = deep ? lds_bytes(0, ctx->scene.depth, false, kRevBounce, kPersistDeepBlock) : lds_bytes(0, ctx->scene.depth, false);
    void (*const rays_k)(Args) = deep ? deep_k : flat_k;
    hipError_t e;
    hipLaunchKernelGGL(rays_k, dim3(resident_blocks(ctx->device, rays_k, nb, lds, c.blocks)), dim3(nb), lds, c.s, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, (std::string(family) + "_rays launch").c_str());
    hipLaunchKernelGGL(exact_k, dim3((unsigned)std::min<long long>(c.blocks, 256)), dim3(kBlock), lds_bytes(0, ctx->scene.depth, true),
                       c.s, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, (std::string(family) + "_exact launch").c_str());
    return ORT_OK;
}

int query_impl(ort_ctx* ctx, const ort_ray_query* q, void* stream) {
    const std::string bad = check_query(q);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_trace_rays: " + bad);
    QueryCall c;
    QueryArgs a;
    const QueryIo io = {q->rays, nullptr, q->hits, q->normals, q->on_device != 0, (q->flags & ORT_QUERY_SORT) != 0, true};
    int rc = query_begin(ctx, "ort_trace_rays", true, q->use_octree, (size_t)q->n_rays, io, stream, c, a);
    if (rc || c.n == 0 || (rc = query_start(ctx, c, a))) return rc;
    if (c.mode == 0) {
        if ((rc = launch_fast_walk(ctx, c, a, ort_query_rays<true>, ort_query_rays<false>, ort_query_exact, "ort_query"))) return rc;
    } else {
        pick<1, 2>(c.mode, [&](auto MODE) {
            hipLaunchKernelGGL((ort_query_lane<ORT_V(MODE)>), dim3((unsigned)c.blocks), dim3(kBlock), 0, c.s, a);
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(ctx, e, "ort_query_lane launch");
    }
    return query_finish(ctx, c);
}

#if ORT_ANALYSIS
ort::RayHit debug_query_mode(const ort::KScene& S, int mode, int qmode, const float* planes, const ort::Ray& r, float t0, float t1,
                             ort::LocalFrames& lf, int* snode, float* stmin, bool want_normal) {
    const bool nearest = qmode == ORT_QM_NEAREST;
    if (mode == 0)
        return nearest ? ort::query_ray_mode<0, ORT_QM_NEAREST>(S, planes, r, t0, t1, lf, nullptr, nullptr, want_normal)
                       : ort::query_ray_mode<0, ORT_QM_ANY>(S, planes, r, t0, t1, lf, nullptr, nullptr, want_normal);
    if (mode == 1)
        return nearest ? ort::query_ray_mode<1, ORT_QM_NEAREST>(S, nullptr, r, t0, t1, lf, snode, stmin, want_normal)
                       : ort::query_ray_mode<1, ORT_QM_ANY>(S, nullptr, r, t0, t1, lf, snode, stmin, want_normal);
    return nearest ? ort::query_ray_mode<2, ORT_QM_NEAREST>(S, nullptr, r, t0, t1, lf, nullptr, nullptr, want_normal)
                   : ort::query_ray_mode<2, ORT_QM_ANY>(S, nullptr, r, t0, t1, lf, nullptr, nullptr, want_normal);
}

// TEST-ONLY host emulation (ort_internal.h): query_ray on the CPU, one ray after another; with
// qmode ORT_QM_NEAREST / ORT_QM_ANY query_ray_mode and the ray's interval (ray_modes.inc).
int debug_query_rays(const float* cr, int32_t n_spheres, const float* node_min, const float* node_max,
                     const int32_t* co, const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx,
                     int64_t n_indices, int32_t layout, int32_t use_octree, const float* rays, int64_t n_rays,
                     int qmode, const float* t_range, ort_ray_hit* hits, float* normals) {
    try {
        if (!cr || n_spheres <= 0 || n_rays < 0 || (n_rays > 0 && (!rays || !hits)))
            return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_query_rays: bad argument");
        HostScene hs;
        if (int rc = hs.build(cr, nullptr, nullptr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, layout,
                              use_octree, HostScene::kNoOctree | HostScene::kValidateTree))
            return fail(nullptr, rc, hs.error);
        const ort::KScene& S = hs.S;
        const std::vector<float>&fplanes = hs.fplanes, &fplanes_b = hs.fplanes_b;
        const int mode = hs.mode;
        const uint8_t* rank_lut = hs.rank_lut;
        std::vector<int> snode(ORT_MAX_STACK);
        std::vector<float> stmin(ORT_MAX_STACK);
        ort::LocalFrames lf;
        for (int64_t i = 0; i < n_rays; ++i) {
            ort::Ray r;
            r.o = ort::mk(rays[6 * (size_t)i], rays[6 * (size_t)i + 1], rays[6 * (size_t)i + 2]);
            r.d = ort::mk(rays[6 * (size_t)i + 3], rays[6 * (size_t)i + 4], rays[6 * (size_t)i + 5]);
            ort::RayHit h;
            const float t0 = t_range ? t_range[2 * (size_t)i] : 0.001f, t1 = t_range ? t_range[2 * (size_t)i + 1] : ORT_MAXFLOAT;
            if (qmode != 0)
                h = debug_query_mode(S, mode, qmode, fplanes.data(), r, t0, t1, lf, snode.data(), stmin.data(), normals != nullptr);
            else if (mode == 0)
                h = ort::query_ray<0>(S, fplanes.data(), fplanes_b.data(), rank_lut, r, lf, nullptr, nullptr, normals != nullptr);
            else if (mode == 1)
                h = ort::query_ray<1>(S, nullptr, nullptr, nullptr, r, lf, snode.data(), stmin.data(), normals != nullptr);
            else
                h = ort::query_ray<2>(S, nullptr, nullptr, nullptr, r, lf, nullptr, nullptr, normals != nullptr);
            hits[i].t = h.t;
            hits[i].sphere = h.sphere;
            if (normals) {
                normals[3 * (size_t)i] = h.normal.x;
                normals[3 * (size_t)i + 1] = h.normal.y;
                normals[3 * (size_t)i + 2] = h.normal.z;
            }
        }
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}
#endif  // ORT_ANALYSIS

}  // namespace

extern "C" {

int ort_trace_rays(ort_ctx* ctx, const ort_ray_query* q, void* stream) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_trace_rays: null ctx");
    return query_impl(ctx, q, stream);
}

int ort_last_query_ms(ort_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_last_query_ms: null argument");
    if (!ctx->query.ev.timed) return fail(ctx, ORT_ERR_NO_SCENE, "no query launched yet");
    HIPCHK(ctx, ctx->query.ev.elapsed(ms));
    return ORT_OK;
}

#if ORT_ANALYSIS
int ort_debug_query_rays(const float* cr, int32_t n_spheres, const float* node_min, const float* node_max,
                         const int32_t* co, const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx,
                         int64_t n_indices, int32_t layout, int32_t use_octree, const float* rays, int64_t n_rays,
                         ort_ray_hit* hits, float* normals) {
    return debug_query_rays(cr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, layout, use_octree, rays,
                            n_rays, 0, nullptr, hits, normals);
}
#endif  // ORT_ANALYSIS

}  // extern "C"
