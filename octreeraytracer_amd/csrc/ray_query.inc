// ray_query.inc -- ray queries (ort_trace_rays): caller rays -> {t, sphere[, normal]} records.
// Included by ort_kernel.hip after the render path (its kernels follow the render kernels in the
// code object, whose code is unchanged); shares ort_ctx, the LDS image and the walks.
//   ort_query_rays<DEEP>   compact layout: the persistent bounce walk (ort_trace_persistent's
//                          configuration) over the caller's rays; rays the fast walk cannot take
//                          go to a defer list
//   ort_query_exact        the literal exact walk of the deferred rays
//   ort_query_lane<MODE>   explicit layout (1) and brute force (2): one ray per lane
//   k_query_keys           ORT_QUERY_SORT: the coherence key of every ray (path_key.h)
// A query owns its buffers (ort_ctx::q_*) and its cursor and defer counters: it reads the scene
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

// The persistent walk over the caller's rays, after ort_trace_persistent: every lane keeps one
// ray's FastState, a wave draws chunks of consecutive items from the atomic cursor and refills
// its idle lanes from its chunk.  The bounce walk's configuration (caller rays are incoherent in
// general): Masks64Plain at depth <= 8, Masks96Lean over the reversed tables at depth 9-10 with
// its leaf hold, the rejected-sphere skip per S.kid / S.nk.
template <bool DEEP>
__global__ void __launch_bounds__(DEEP ? kPersistDeepBlock : kBlock) __attribute__((amdgpu_waves_per_eu(ORT_PERSISTENT_WAVES)))
ort_query_rays(QueryArgs A) {
    // (a symbol of the queries' own: the render kernels' dynamic LDS symbol keeps its alignment)
    extern __shared__ __attribute__((aligned(4096))) unsigned char query_smem[];
    unsigned char* const smem = query_smem;
    constexpr bool REV = DEEP && kRevBounce;
    LdsView L = setup_lds<true, DEEP ? kPersistDeepBlock : kBlock, REV>(smem, A.S);
    const uint8_t* lut = L.lut;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    ort::Counters cnt;  // (fast_step's COUNT = false: unused)
    for (int q = 0; q < 6; ++q) cnt.v[q] = 0;
    using Masks = typename std::conditional<DEEP, ort::Masks96Lean, ort::Masks64Plain>::type;
    ort::FastStateT<Masks> st;
    int k = -1;              // the lane's ray index, -1 idle
    int next = 0, end = 0;   // wave-uniform: remaining work items [next, end) of the wave's chunk
    bool drained = false;    // wave-uniform: the global cursor passed the item count
    const int total = A.n;
#if ORT_CHUNK_ADAPT
    const int chunk = total >= (int)(gridDim.x * (blockDim.x >> 6)) * ORT_CHUNK_ADAPT ? 2 * kChunk : kChunk;
#else
    constexpr int chunk = kChunk;
#endif
    const bool want_normal = A.normals != nullptr;
    for (;;) {
        const unsigned long long idle = __ballot(k < 0);
        const int n_idle = __popcll(idle);
        if (n_idle == 64 && drained) break;
        if (!drained && n_idle >= A.refill) {
            if (next == end) {
                int base = 0;
                if (lane == 0) base = atomicAdd(A.sync + 1, chunk);
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
                    const int cand = A.qlist ? A.qlist[next + rank] : next + rank;
                    const ort::Ray ray = query_load_ray(A, cand);
                    ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
                    if (A.exact_only || !ort::fast_prepare(A.S, ray, inv)) {
                        A.defer_list[atomicAdd(A.sync, 1)] = cand;
                    } else if (ort::fast_begin(A.S, L.planes, lut, ray, inv, 0.001f, ORT_MAXFLOAT, st)) {
                        k = cand;
                    } else {  // misses the root box
                        query_store(A, cand, ort::query_hit<0>(A.S, ray, false, 0.0f, -1, false));
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
            if (ort::fast_step<false>(A.S, lut, st, L.fr, cnt)) {
                // (the ray back from the walk state, bit-identical: no registers held across the walk)
                query_store(A, k, ort::query_hit<0>(A.S, st.ray(), st.hit(), st.closest, st.hitEntry, want_normal));
                k = -1;
            }
        }
    }
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

// One ray per lane: the explicit layout's literal 200-entry stack walk (MODE 1), brute force (2).
template <int MODE>
__global__ void __launch_bounds__(kBlock) ort_query_lane(QueryArgs A) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n) return;
    const ort::Ray ray = query_load_ray(A, (int)i);
    const bool want_normal = A.normals != nullptr;
    ort::LocalFrames unused;
    if constexpr (MODE == 1) {
        int snode[ORT_MAX_STACK];
        float stmin[ORT_MAX_STACK];
        query_store(A, (int)i, ort::query_ray<1>(A.S, nullptr, nullptr, nullptr, ray, unused, snode, stmin, want_normal));
    } else {
        query_store(A, (int)i, ort::query_ray<2>(A.S, nullptr, nullptr, nullptr, ray, unused, nullptr, nullptr, want_normal));
    }
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

// The scene's origin-code tables (path_key.h), built once per root box (shared with the path sort:
// scene state, not frame state).
int ensure_key_spread(ort_ctx* ctx) {
    const float box[6] = {ctx->root_lo[0], ctx->root_lo[1], ctx->root_lo[2], ctx->root_hi[0], ctx->root_hi[1], ctx->root_hi[2]};
    if (ctx->key_spread.p && std::memcmp(box, ctx->spread_box, sizeof box) == 0) return ORT_OK;
    int rc;
    if ((rc = ensure(ctx, ctx->key_spread, 4 * (size_t)ort::kSpreadWords))) return rc;
    std::vector<uint32_t> tab((size_t)ort::kSpreadWords);
    ort::mortonSpread(ort::mortonPlan(ctx->root_lo, ctx->root_hi), tab.data());
    HIPCHK(ctx, hipMemcpy(ctx->key_spread.p, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice));
    std::memcpy(ctx->spread_box, box, sizeof box);
    return ORT_OK;
}

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

int query_impl(ort_ctx* ctx, const ort_ray_query* q, void* stream) {
    const std::string bad = check_query(q);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_trace_rays: " + bad);
    if (!ctx->has_scene) return fail(ctx, ORT_ERR_NO_SCENE, "ort_trace_rays: no scene uploaded");
    const int mode = (q->use_octree == 1) ? (ctx->layout == ORT_LAYOUT_COMPACT ? 0 : 1) : 2;
    if (mode != 2 && ctx->n_nodes <= 0) return fail(ctx, ORT_ERR_NO_SCENE, "ort_trace_rays: scene has no octree");
    const size_t n = (size_t)q->n_rays;
    if (n == 0) return ORT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const bool host = !q->on_device;
    const bool sort = mode == 0 && (q->flags & ORT_QUERY_SORT) != 0;
    int rc;
    if ((rc = ensure(ctx, ctx->q_sync, 64))) return rc;
    if (mode == 0 && (rc = ensure(ctx, ctx->q_defer, 4 * n))) return rc;
    if (host && ((rc = ensure(ctx, ctx->q_rays, sizeof(ort_ray) * n)) || (rc = ensure(ctx, ctx->q_hits, sizeof(ort_ray_hit) * n)) ||
                 (q->normals && (rc = ensure(ctx, ctx->q_normals, 12 * n)))))
        return rc;
    size_t temp_bytes = 0;
    if (sort) {
        temp_bytes = ort::sortAliveTempBytes((int)n);
        if ((rc = ensure(ctx, ctx->q_keys, 4 * n)) || (rc = ensure(ctx, ctx->q_keys2, 4 * n)) || (rc = ensure(ctx, ctx->q_vals, 4 * n)) ||
            (rc = ensure(ctx, ctx->q_list, 4 * n)) || (rc = ensure(ctx, ctx->q_temp, std::max<size_t>(temp_bytes, 16))) ||
            (rc = ensure_key_spread(ctx)))
            return rc;
    }
    if (!ctx->qev0) HIPCHK(ctx, hipEventCreate(&ctx->qev0));
    if (!ctx->qev1) HIPCHK(ctx, hipEventCreate(&ctx->qev1));
    QueryArgs a;
    std::memset(&a, 0, sizeof(a));
    a.S = device_scene(ctx);
    a.rays = host ? (const float*)ctx->q_rays.p : (const float*)q->rays;
    a.hits = host ? (int2*)ctx->q_hits.p : (int2*)q->hits;
    a.normals = q->normals ? (host ? (float*)ctx->q_normals.p : q->normals) : nullptr;
    a.defer_list = (int*)ctx->q_defer.p;
    a.sync = (int*)ctx->q_sync.p;
    a.n = (int)n;
    a.refill = ctx->refill;
    a.exact_only = ctx->exact_only || !ctx->ordered;
    if (host) HIPCHK(ctx, hipMemcpyAsync(ctx->q_rays.p, q->rays, sizeof(ort_ray) * n, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(ctx->q_sync.p, 0, 64, s));
    HIPCHK(ctx, hipEventRecord(ctx->qev0, s));
    hipError_t e;
    const long long blocks = ((long long)n + kBlock - 1) / kBlock;
    if (mode == 0) {
        if (sort) {  // the ray count is known here: one sort of n pairs, no host wait
            hipLaunchKernelGGL(k_query_keys, dim3((unsigned)std::min<long long>(blocks, 2048)), dim3(kBlock), 0, s, a,
                               ort::mortonPlan(ctx->root_lo, ctx->root_hi), (const uint32_t*)ctx->key_spread.p,
                               (uint32_t*)ctx->q_keys.p, (int*)ctx->q_vals.p);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "k_query_keys launch");
            const ort::SortBuffers sb = {(uint32_t*)ctx->q_keys.p, (uint32_t*)ctx->q_keys2.p, (int*)ctx->q_vals.p, (int*)ctx->q_list.p};
            if ((e = ort::sortList(ctx->q_temp.p, temp_bytes, (int)n, sb, s)) != hipSuccess) return hip_fail(ctx, e, "query sort");
            a.qlist = (const int*)ctx->q_list.p;
        }
        const bool deep = ctx->depth > 8;
        const size_t lds = deep ? lds_bytes(0, ctx->depth, false, kRevBounce, kPersistDeepBlock) : lds_bytes(0, ctx->depth, false);
        if (deep) {
            const int g = resident_blocks(ctx->device, ort_query_rays<true>, kPersistDeepBlock, lds, blocks);
            hipLaunchKernelGGL((ort_query_rays<true>), dim3(g), dim3(kPersistDeepBlock), lds, s, a);
        } else {
            const int g = resident_blocks(ctx->device, ort_query_rays<false>, kBlock, lds, blocks);
            hipLaunchKernelGGL((ort_query_rays<false>), dim3(g), dim3(kBlock), lds, s, a);
        }
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_query_rays launch");
        hipLaunchKernelGGL(ort_query_exact, dim3((unsigned)std::min<long long>(blocks, 256)), dim3(kBlock),
                           lds_bytes(0, ctx->depth, true), s, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_query_exact launch");
    } else {
        if (mode == 1) hipLaunchKernelGGL((ort_query_lane<1>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
        else hipLaunchKernelGGL((ort_query_lane<2>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_query_lane launch");
    }
    HIPCHK(ctx, hipEventRecord(ctx->qev1, s));
    ctx->q_timed = true;
    if (host) {
        HIPCHK(ctx, hipMemcpyAsync(q->hits, ctx->q_hits.p, sizeof(ort_ray_hit) * n, hipMemcpyDeviceToHost, s));
        if (q->normals) HIPCHK(ctx, hipMemcpyAsync(q->normals, ctx->q_normals.p, 12 * n, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    } else if (!stream) {
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return ORT_OK;
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
        ort::KScene S;
        std::memset(&S, 0, sizeof(S));
        S.sph_cr = (const float4*)cr;
        S.n_spheres = n_spheres;
        S.n_nodes = n_nodes;
        ort::CompactLayout cl;
        std::vector<float> fplanes, fplanes_b, A, B;
        std::vector<float> ma, fr;
        int mode = 2;
        if (use_octree == 1) {
            if (n_nodes <= 0) return fail(nullptr, ORT_ERR_NO_SCENE, "no octree");
            ma.assign((size_t)n_spheres * 4, 0.0f);
            fr.assign((size_t)n_spheres * 4, 0.0f);
            ort::SceneInput in{cr, ma.data(), fr.data(), n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices};
            const std::string vbad = ort::validateScene(in);
            if (!vbad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, vbad);
            if (layout == ORT_LAYOUT_COMPACT) {
                std::string why;
                if (!ort::buildCompactLayout(in, ORT_COMPACT_MAX_DEPTH, cl, why)) return fail(nullptr, ORT_ERR_UNSUPPORTED, why);
                mode = 0;
                S.node = (const uint2*)cl.node.data();
                S.kid = (const uint2*)cl.kid.data();
                S.tail_base = (uint32_t)in.n_indices;
                S.leaf_sph = (const float4*)cl.leaf_sph.data();
                S.leaf_idx = cl.leaf_idx.data();
                S.planes = cl.planes.data();
                S.depth = cl.depth;
                fplanes.resize(ort::fast_plane_floats(cl.depth));
                ort::fill_fast_planes(cl.planes.data(), fplanes.data(), cl.depth);
                const bool rev_b = ort::Masks96Lean::kRevPlanes || ort::fast_rev_planes(cl.depth);
                fplanes_b.resize(ort::fast_plane_floats(cl.depth, rev_b));
                ort::fill_fast_planes(cl.planes.data(), fplanes_b.data(), cl.depth, rev_b);
            } else {
                mode = 1;
                A.resize(4 * (size_t)n_nodes);
                B.resize(4 * (size_t)n_nodes);
                for (int32_t i = 0; i < n_nodes; ++i) {
                    for (int k = 0; k < 3; ++k) {
                        A[4 * (size_t)i + k] = node_min[3 * (size_t)i + k];
                        B[4 * (size_t)i + k] = node_max[3 * (size_t)i + k];
                    }
                    std::memcpy(&A[4 * (size_t)i + 3], &co[i], 4);
                    std::memcpy(&B[4 * (size_t)i + 3], &oo[i], 4);
                }
                S.nodeA = (const float4*)A.data();
                S.nodeB = (const float4*)B.data();
                S.count = cnt;
                S.indices = idx;
            }
        }
        std::vector<uint8_t> lut(kRankLutBytes);
        for (size_t i = 0; i < lut.size(); ++i) lut[i] = ort::rank_lut_entry((uint32_t)i >> 8, (uint32_t)i & 255u);
        const uint8_t* rank_lut = (mode == 0 && cl.ordered) ? lut.data() : nullptr;
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
    if (!ctx->q_timed) return fail(ctx, ORT_ERR_NO_SCENE, "no query launched yet");
    HIPCHK(ctx, hipEventSynchronize(ctx->qev1));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->qev0, ctx->qev1));
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
