// ray_modes.inc -- query modes (ort_trace_rays_ex): the nearest hit (ORT_QUERY_NEAREST) and any
// hit (ORT_QUERY_ANY) inside a per-ray interval (t_min, t_max).  Included by ort_kernel.hip last,
// after camera_query.inc, so that every earlier kernel keeps its place in the code object; shares
// ray_query.inc's arguments, record store, buffers, sort and timing events.  ORT_QUERY_DRAWN goes
// to ray_query.inc's query_impl: the same kernels as ort_trace_rays.
//   ort_query_mode_tree<QM>      compact layout: ort_query_rays' persistent loop (chunks, refill) around
//                                render_core.h mode_walk_begin / mode_walk_step over the LDS plane
//                                tables (the exact walk's image, one frame column per lane)
//   ort_query_mode_lane<MODE,QM> explicit layout (1) and brute force (2): one ray per lane
// Every ray takes the literal walk with the zero-axis rule: there is no fast walk and so no defer
// list for these modes yet, and ORT_OPT_KID_SKIP, ORT_OPT_EXACT_TRAVERSAL and ORT_OPT_REFILL change
// no record (ORT_OPT_REFILL sets when a wave refills, the other two touch nothing here).
// ORT_QUERY_SORT orders the work items of the compact walk as it does for ort_trace_rays.

namespace {

struct ModeArgs {
    QueryArgs q;
    const float* t_range;  // 2 floats per ray {t_min, t_max}, or null = (0.001, MAXFLOAT)
};

__device__ inline void mode_interval(const ModeArgs& A, int i, float& t_min, float& t_max) {
    t_min = 0.001f;
    t_max = ORT_MAXFLOAT;
    if (A.t_range) {
        t_min = A.t_range[2 * (size_t)i];
        t_max = A.t_range[2 * (size_t)i + 1];
    }
}

// The persistent loop of ort_query_rays around the literal walk: every lane keeps one ray's
// ModeWalk and its frame column in LDS, a wave draws chunks of consecutive items from the atomic
// cursor and refills its idle lanes from its chunk when ORT_OPT_REFILL of them are idle, so a lane
// whose ray is done -- early, in ANY -- takes the next ray instead of waiting for the wave's
// longest walk.  Item -> ray through the sorted list where there is one.  A ray with an invalid
// interval, or one that misses the root box, gets its miss record at refill.
template <int QM>
__global__ void __launch_bounds__(kBlock) ort_query_mode_tree(ModeArgs A) {
    extern __shared__ __attribute__((aligned(4096))) unsigned char query_smem[];  // plane tables: 1 KiB-aligned at least
    unsigned char* const smem = query_smem;
    LdsView L = setup_lds<false>(smem, A.q.S);
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const bool want_normal = A.q.normals != nullptr;
    const int total = A.q.n;
    ort::ModeWalk w;
    int k = -1;              // the lane's ray index, -1 idle
    int next = 0, end = 0;   // wave-uniform: remaining work items [next, end) of the wave's chunk
    bool drained = false;    // wave-uniform: the global cursor passed the item count
    for (;;) {
        const unsigned long long idle = __ballot(k < 0);
        const int n_idle = __popcll(idle);
        if (n_idle == 64 && drained) break;
        if (!drained && n_idle >= A.q.refill) {
            if (next == end) {
                int base = 0;
                if (lane == 0) base = atomicAdd(A.q.sync + 1, kChunk);
                base = __shfl(base, 0);
                if (base >= total) {
                    drained = true;
                    continue;
                }
                next = base;
                end = min(base + kChunk, total);
            }
            const int take = min(n_idle, end - next);
            if (k < 0) {
                const int rank = __popcll(idle & below);
                if (rank < take) {
                    const int cand = A.q.qlist ? A.q.qlist[next + rank] : next + rank;
                    const ort::Ray ray = query_load_ray(A.q, cand);
                    float t_min, t_max;
                    mode_interval(A, cand, t_min, t_max);
                    if (ort::query_interval(t_min, t_max) && ort::mode_walk_begin(A.q.S, L.planes, ray, t_min, t_max, w))
                        k = cand;
                    else
                        query_store(A.q, cand, ort::query_hit<0>(A.q.S, ray, false, 0.0f, -1, false));
                }
            }
            next += take;
            continue;
        }
        if (k >= 0 && ort::mode_walk_step<QM>(A.q.S, L.planes, w, L.fr)) {
            query_store(A.q, k, ort::query_hit<0>(A.q.S, w.r, w.hit, w.closest, w.hitEntry, want_normal));
            k = -1;
        }
    }
}

template <int MODE, int QM>
__global__ void __launch_bounds__(kBlock) ort_query_mode_lane(ModeArgs A) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.q.n) return;
    const ort::Ray ray = query_load_ray(A.q, (int)i);
    const bool want_normal = A.q.normals != nullptr;
    float t_min, t_max;
    mode_interval(A, (int)i, t_min, t_max);
    ort::LocalFrames unused;
    if constexpr (MODE == 1) {
        int snode[ORT_MAX_STACK];
        float stmin[ORT_MAX_STACK];
        query_store(A.q, (int)i, ort::query_ray_mode<1, QM>(A.q.S, nullptr, ray, t_min, t_max, unused, snode, stmin, want_normal));
    } else {
        query_store(A.q, (int)i, ort::query_ray_mode<2, QM>(A.q.S, nullptr, ray, t_min, t_max, unused, nullptr, nullptr, want_normal));
    }
}

std::string check_query_ex(const ort_ray_query_ex* q) {
    if (!q) return "null query";
    const std::string bad = check_query(&q->base);
    if (!bad.empty()) return bad;
    if (q->mode != ORT_QUERY_DRAWN && q->mode != ORT_QUERY_NEAREST && q->mode != ORT_QUERY_ANY) return "unknown mode";
    if (q->reserved[0] != 0 || q->reserved[1] != 0 || q->reserved[2] != 0) return "reserved must be 0";
    if ((uintptr_t)q->t_range & 3) return "t_range must be 4-byte aligned";
    if (q->t_range && q->mode == ORT_QUERY_DRAWN) return "ORT_QUERY_DRAWN takes no t_range: its interval is the shader's";
    return "";
}

// ort_trace_rays_ex for NEAREST and ANY: query_impl's staging, sort and timing around the mode's kernel.
int query_mode_impl(ort_ctx* ctx, const ort_ray_query_ex* qx, void* stream) {
    const ort_ray_query* q = &qx->base;
    if (!ctx->has_scene) return fail(ctx, ORT_ERR_NO_SCENE, "ort_trace_rays_ex: no scene uploaded");
    const int mode = (q->use_octree == 1) ? (ctx->layout == ORT_LAYOUT_COMPACT ? 0 : 1) : 2;
    if (mode != 2 && ctx->n_nodes <= 0) return fail(ctx, ORT_ERR_NO_SCENE, "ort_trace_rays_ex: scene has no octree");
    const size_t n = (size_t)q->n_rays;
    if (n == 0) return ORT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const bool host = !q->on_device;
    const bool sort = mode == 0 && (q->flags & ORT_QUERY_SORT) != 0;
    const bool nearest = qx->mode == ORT_QUERY_NEAREST;
    int rc;
    if ((rc = ensure(ctx, ctx->q_sync, 64))) return rc;
    if (host && ((rc = ensure(ctx, ctx->q_rays, sizeof(ort_ray) * n)) || (rc = ensure(ctx, ctx->q_hits, sizeof(ort_ray_hit) * n)) ||
                 (q->normals && (rc = ensure(ctx, ctx->q_normals, 12 * n))) ||
                 (qx->t_range && (rc = ensure(ctx, ctx->q_trange, 8 * n)))))
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
    ModeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q.S = device_scene(ctx);
    a.q.rays = host ? (const float*)ctx->q_rays.p : (const float*)q->rays;
    a.q.hits = host ? (int2*)ctx->q_hits.p : (int2*)q->hits;
    a.q.normals = q->normals ? (host ? (float*)ctx->q_normals.p : q->normals) : nullptr;
    a.q.sync = (int*)ctx->q_sync.p;  // [1] the work cursor
    a.q.n = (int)n;
    a.q.refill = ctx->refill;
    a.t_range = qx->t_range ? (host ? (const float*)ctx->q_trange.p : qx->t_range) : nullptr;
    if (host) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->q_rays.p, q->rays, sizeof(ort_ray) * n, hipMemcpyHostToDevice, s));
        if (qx->t_range) HIPCHK(ctx, hipMemcpyAsync(ctx->q_trange.p, qx->t_range, 8 * n, hipMemcpyHostToDevice, s));
    }
    HIPCHK(ctx, hipMemsetAsync(ctx->q_sync.p, 0, 64, s));
    HIPCHK(ctx, hipEventRecord(ctx->qev0, s));
    hipError_t e;
    const long long blocks = ((long long)n + kBlock - 1) / kBlock;
    if (mode == 0) {
        if (sort) {
            hipLaunchKernelGGL(k_query_keys, dim3((unsigned)std::min<long long>(blocks, 2048)), dim3(kBlock), 0, s, a.q,
                               ort::mortonPlan(ctx->root_lo, ctx->root_hi), (const uint32_t*)ctx->key_spread.p,
                               (uint32_t*)ctx->q_keys.p, (int*)ctx->q_vals.p);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "k_query_keys launch");
            const ort::SortBuffers sb = {(uint32_t*)ctx->q_keys.p, (uint32_t*)ctx->q_keys2.p, (int*)ctx->q_vals.p, (int*)ctx->q_list.p};
            if ((e = ort::sortList(ctx->q_temp.p, temp_bytes, (int)n, sb, s)) != hipSuccess) return hip_fail(ctx, e, "query sort");
            a.q.qlist = (const int*)ctx->q_list.p;
        }
        const size_t lds = lds_bytes(0, ctx->depth, false);
        if (nearest) {
            const int g = resident_blocks(ctx->device, ort_query_mode_tree<ORT_QM_NEAREST>, kBlock, lds, blocks);
            hipLaunchKernelGGL((ort_query_mode_tree<ORT_QM_NEAREST>), dim3(g), dim3(kBlock), lds, s, a);
        } else {
            const int g = resident_blocks(ctx->device, ort_query_mode_tree<ORT_QM_ANY>, kBlock, lds, blocks);
            hipLaunchKernelGGL((ort_query_mode_tree<ORT_QM_ANY>), dim3(g), dim3(kBlock), lds, s, a);
        }
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_query_mode_tree launch");
    } else {
        const dim3 grid((unsigned)blocks);
        if (mode == 1) {
            if (nearest) hipLaunchKernelGGL((ort_query_mode_lane<1, ORT_QM_NEAREST>), grid, dim3(kBlock), 0, s, a);
            else hipLaunchKernelGGL((ort_query_mode_lane<1, ORT_QM_ANY>), grid, dim3(kBlock), 0, s, a);
        } else {
            if (nearest) hipLaunchKernelGGL((ort_query_mode_lane<2, ORT_QM_NEAREST>), grid, dim3(kBlock), 0, s, a);
            else hipLaunchKernelGGL((ort_query_mode_lane<2, ORT_QM_ANY>), grid, dim3(kBlock), 0, s, a);
        }
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_query_mode_lane launch");
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

}  // namespace

extern "C" {

int ort_trace_rays_ex(ort_ctx* ctx, const ort_ray_query_ex* q, void* stream) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_trace_rays_ex: null ctx");
    const std::string bad = check_query_ex(q);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_trace_rays_ex: " + bad);
    if (q->mode == ORT_QUERY_DRAWN) return query_impl(ctx, &q->base, stream);
    return query_mode_impl(ctx, q, stream);
}

#if ORT_ANALYSIS
// TEST-ONLY host emulation (ort_internal.h): query_ray_mode on the CPU, one ray after another;
// ORT_QUERY_DRAWN is ort_debug_query_rays.
int ort_debug_query_rays_ex(const float* cr, int32_t n_spheres, const float* node_min, const float* node_max,
                            const int32_t* co, const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx,
                            int64_t n_indices, int32_t layout, int32_t use_octree, const float* rays, int64_t n_rays,
                            int32_t qmode, const float* t_range, ort_ray_hit* hits, float* normals) {
    if (qmode == ORT_QUERY_DRAWN) {
        if (t_range) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_query_rays_ex: ORT_QUERY_DRAWN takes no t_range");
        return ort_debug_query_rays(cr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, layout, use_octree,
                                    rays, n_rays, hits, normals);
    }
    if (qmode != ORT_QUERY_NEAREST && qmode != ORT_QUERY_ANY)
        return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_query_rays_ex: unknown mode");
    return debug_query_rays(cr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, layout, use_octree, rays,
                            n_rays, qmode, t_range, hits, normals);
}
#endif  // ORT_ANALYSIS

}  // extern "C"
