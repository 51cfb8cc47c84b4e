// ray_modes.inc -- query modes (ort_trace_rays_ex): the nearest hit (ORT_QUERY_NEAREST) and any
// hit (ORT_QUERY_ANY) inside a per-ray interval (t_min, t_max).  Included by ort_kernel.hip last,
// after camera_query.inc, so that every earlier kernel keeps its place in the code object; shares
// ray_query.inc's arguments, record store, buffers, sort and timing events.  ORT_QUERY_DRAWN goes
// to ray_query.inc's query_impl: the same kernels as ort_trace_rays.
//   ort_query_mode_tree<QM>      compact layout: ray_query.inc's query_item_loop over RaySource with
//                                ModeQueryWalk: render_core.h mode_walk_begin / mode_walk_step over the
//                                LDS plane tables (the exact walk's image, one frame column per lane)
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

// The literal mode walk as ray_query.inc's walk: every lane keeps one ray's ModeWalk and its frame
// column in LDS, so a lane whose ray is done -- early, in ANY -- takes the next ray instead of
// waiting for the wave's longest walk.  No defer and no hold; a ray with an invalid interval, or
// one that misses the root box, gets its miss record at refill.
template <int QM>
struct ModeQueryWalk {
    static constexpr bool kAdaptChunk = false;  // fixed kChunk chunks
    static constexpr bool kFast = false;
    using Args = ModeArgs;
    const ModeArgs& A;
    LdsView L;
    ort::ModeWalk w;
    __device__ __forceinline__ ModeQueryWalk(const ModeArgs& a, unsigned char* smem) : A(a), L(setup_lds<false>(smem, a.q.S)) {}
    __device__ __forceinline__ void begin(int i, const ort::Ray& ray, int& k) {
        float t_min, t_max;
        mode_interval(A, i, t_min, t_max);
        if (ort::query_interval(t_min, t_max) && ort::mode_walk_begin(A.q.S, L.planes, ray, t_min, t_max, w)) k = i;
        else query_store_miss(A.q, i, ray);
    }
    __device__ __forceinline__ bool held(bool) const { return false; }
    __device__ __forceinline__ bool step() { return ort::mode_walk_step<QM>(A.q.S, L.planes, w, L.fr); }
    __device__ __forceinline__ void finish(int i) const {
        query_store(A.q, i, ort::query_hit<0>(A.q.S, w.r, w.hit, w.closest, w.hitEntry, A.q.normals != nullptr));
    }
};

template <int QM>
__global__ void __launch_bounds__(kBlock) ort_query_mode_tree(ModeArgs A) {
    extern __shared__ __attribute__((aligned(4096))) unsigned char query_smem[];  // plane tables: 1 KiB-aligned at least
    query_item_loop<RaySource, ModeQueryWalk<QM>>(A.q, RaySource{A.q}, A, query_smem, blockDim.x >> 6);
}

template <int MODE, int QM>
__global__ void __launch_bounds__(kBlock) ort_query_mode_lane(ModeArgs A) {
    query_lane_body<MODE>(A.q, RaySource{A.q}, [&](const ort::Ray& ray, int i, ort::LocalFrames& lf, int* snode, float* stmin, bool want_normal) {
        float t_min, t_max;
        mode_interval(A, i, t_min, t_max);
        return ort::query_ray_mode<MODE, QM>(A.q.S, nullptr, ray, t_min, t_max, lf, snode, stmin, want_normal);
    });
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

// ort_trace_rays_ex for NEAREST and ANY: ray_query.inc's staging, sort and timing around the mode's
// kernel; the intervals are this entry point's own staged input.
int query_mode_impl(ort_ctx* ctx, const ort_ray_query_ex* qx, void* stream) {
    const ort_ray_query* q = &qx->base;
    QueryCall c;
    ModeArgs a;
    std::memset(&a, 0, sizeof(a));
    const QueryIo io = {q->rays, nullptr, q->hits, q->normals, q->on_device != 0, (q->flags & ORT_QUERY_SORT) != 0, false};
    int rc = query_begin(ctx, "ort_trace_rays_ex", true, q->use_octree, (size_t)q->n_rays, io, stream, c, a.q);
    if (rc || c.n == 0) return rc;
    if (qx->t_range) {
        a.t_range = qx->t_range;
        if (c.host) {
            if ((rc = ensure(ctx, ctx->query.trange, 8 * c.n))) return rc;
            HIPCHK(ctx, hipMemcpyAsync(ctx->query.trange.p, qx->t_range, 8 * c.n, hipMemcpyHostToDevice, c.s));
            a.t_range = (const float*)ctx->query.trange.p;
        }
    }
    if ((rc = query_start(ctx, c, a.q))) return rc;
    const dim3 block(kBlock);
    if (c.mode == 0) {
        const size_t lds = lds_bytes(0, ctx->scene.depth, false);
        pick<ORT_QM_NEAREST, ORT_QM_ANY>(qx->mode == ORT_QUERY_NEAREST ? ORT_QM_NEAREST : ORT_QM_ANY, [&](auto QM) {
            const int g = resident_blocks(ctx->device, ort_query_mode_tree<ORT_V(QM)>, kBlock, lds, c.blocks);
            hipLaunchKernelGGL((ort_query_mode_tree<ORT_V(QM)>), dim3(g), block, lds, c.s, a);
        });
    } else {
        pick<1, 2>(c.mode, [&](auto MODE) {
            pick<ORT_QM_NEAREST, ORT_QM_ANY>(qx->mode == ORT_QUERY_NEAREST ? ORT_QM_NEAREST : ORT_QM_ANY, [&](auto QM) {
                hipLaunchKernelGGL((ort_query_mode_lane<ORT_V(MODE), ORT_V(QM)>), dim3((unsigned)c.blocks), block, 0, c.s, a);
            });
        });
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, c.mode == 0 ? "ort_query_mode_tree launch" : "ort_query_mode_lane launch");
    return query_finish(ctx, c);
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
