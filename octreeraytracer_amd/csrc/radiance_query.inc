// radiance_query.inc -- radiance queries (ort_trace_radiance): caller rays and caller RNG states ->
// what each ray sees, the mean of `paths` evaluations of the shader's radiance() chained through
// the ray's state, {rgb[, end state]} records.
// Included last by ort_kernel.hip (its kernels follow every other kernel in the code object, whose
// code is unchanged).  The lane loop is ort_pixel_paths' -- a lane owns a chain of paths and steps
// it one bounce at a time: pixel_trace, hit_record, shade_bounce -- fed from the caller's arrays
// instead of pixels and primary_ray; the host side is ray_query.inc's staging (query_begin /
// query_start, query_sort) and state (ort_ctx::query), with two staging buffers of its own.
//   ort_radiance_paths<MODE, DEEP, LDS>  the four walk variants launch_accum_paths picks: brute
//                                        force, deep compact, LDS-resident scene, plain compact
// The work item is the ray index, through the sorted list where there is one.

namespace {

struct RadianceArgs {
    PipeArgs P;          // what pixel_trace and the LDS scene copy read: S, exact_only, lds_*
    const float* rays;   // 6 floats per ray (ort_ray)
    const float* states; // 2 floats per ray: randState at the start of the ray's first path
    float* radiance;     // 3 floats per ray
    float* states_out;   // 2 floats per ray, or null (wave-uniform); may be == states
    const int* qlist;    // ORT_QUERY_SORT: work item -> ray index, or null = the index itself
    int* sync;           // [1] work cursor
    int n;               // rays
    int max_depth, paths, flags;
};

// rand2D's float -> uint conversion is defined for states in [0, 1) only (NaN fails every test).
ORT_FN bool radiance_state_ok(const ort_rng& st) { return st.x >= 0.0f && st.x < 1.0f && st.y >= 0.0f && st.y < 1.0f; }

// The ray a path starts from: the caller's, its direction through the shader's normalize (glsl:602)
// where asked.
ORT_FN ort::Ray radiance_ray(const float* rays, long long i, int flags) {
    const float* p = rays + 6 * (size_t)i;
    ort::Ray r;
    r.o = ort::mk(p[0], p[1], p[2]);
    r.d = ort::mk(p[3], p[4], p[5]);
    if (flags & ORT_RADIANCE_NORMALIZE) r.d = ort::normalize(r.d);
    return r;
}

// The record of a finished chain: col / paths (paths == 1: col itself: x / 1.0f == x exactly), with
// ORT_RADIANCE_GAMMA main()'s last lines (finish_pixel: the same division, then pow).
ORT_FN ort::V3 radiance_value(ort::V3 col, int paths, int flags) {
    if (flags & ORT_RADIANCE_GAMMA) return ort::finish_pixel(col, paths);
    const float fp = (float)paths;
    return paths != 1 ? ort::mk(col.x / fp, col.y / fp, col.z / fp) : col;
}

ORT_FN void radiance_store(float* radiance, float* states_out, long long i, const ort::V3& v, const ort_rng& st) {
    float* o = radiance + 3 * (size_t)i;
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
    if (states_out) {
        states_out[2 * (size_t)i] = st.x;
        states_out[2 * (size_t)i + 1] = st.y;
    }
}

// ort_pixel_paths' loop over rays: every lane keeps one ray's chain (path s of A.paths, bounce b,
// throughput c, importance, the sum col, the RNG state st); a wave draws chunks of 64 consecutive
// work items from the atomic cursor A.sync[1] and refills its idle lanes from its chunk by rank
// among the idle; when the cursor passes A.n the wave drains.  A path that ends adds c to col and
// the next one starts from the ray read again (not held in registers across the chain).
template <int MODE, bool DEEP, bool LDS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_PIXEL_WAVES)))
ort_radiance_paths(RadianceArgs A) {
    // (the queries' own symbol: the render kernels' dynamic LDS symbol keeps its alignment)
    extern __shared__ __attribute__((aligned(4096))) unsigned char query_smem[];
    unsigned char* const smem = query_smem;
    LdsView L{};
    ort::KScene S = A.P.S;
    if (LDS) {  // the workgroup's copies of nk[] and leaf_sph[], as ort_pixel_paths makes them (before setup_lds's barrier)
        uint4* dn = reinterpret_cast<uint4*>(smem + A.P.lds_nk_off);
        uint4* ds = reinterpret_cast<uint4*>(smem + A.P.lds_sph_off);
        const uint4* sl = reinterpret_cast<const uint4*>(A.P.S.leaf_sph);
        for (int i = threadIdx.x; i < A.P.lds_nk_n16; i += kBlock) dn[i] = A.P.S.nk[i];
        for (int i = threadIdx.x; i < A.P.lds_sph_n16; i += kBlock) ds[i] = sl[i];
        S.lds_nk = (uint32_t)(size_t)(const __attribute__((address_space(3))) unsigned char*)(smem + A.P.lds_nk_off);
        S.lds_sph = (uint32_t)(size_t)(const __attribute__((address_space(3))) unsigned char*)(smem + A.P.lds_sph_off);
    }
    if (MODE == 0) L = setup_lds<true>(smem, A.P.S);
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int maxd = A.max_depth, paths = A.paths, total = A.n;
    int k = -1;             // the lane's ray (record index), -1 idle
    int s = 0, b = 0;       // the path of the chain, the bounce of the path
    ort::Ray ray;
    ray.o = ray.d = ort::mk(0.0f, 0.0f, 0.0f);
    ort::V3 c = ort::mk(1.0f, 1.0f, 1.0f), col = ort::mk(0.0f, 0.0f, 0.0f);
    float importance = 1.0f;
    ort_rng st;
    st.x = st.y = 0.0f;
    int next = 0, end = 0;  // wave-uniform: remaining work items [next, end) of the wave's chunk
    bool drained = false;   // wave-uniform: the cursor passed the item count
    for (;;) {
        const unsigned long long idle = __ballot(k < 0);
        if (idle && !drained) {  // refill: idle lanes take the chunk's next rays
            if (next == end) {
                int base = 0;
                if (lane == 0) base = atomicAdd(A.sync + 1, 64);
                base = __shfl(base, 0);
                if (base >= total) {
                    drained = true;
                } else {
                    next = base;
                    end = min(base + 64, total);
                }
            }
            if (!drained) {
                const int take = min(__popcll(idle), end - next);
                if (k < 0) {
                    const int rank = __popcll(idle & below);
                    if (rank < take) {
                        const int cand = A.qlist ? A.qlist[next + rank] : next + rank;
                        st.x = A.states[2 * (size_t)cand];
                        st.y = A.states[2 * (size_t)cand + 1];
                        if (radiance_state_ok(st)) {
                            k = cand;
                            s = 0;
                            b = 0;
                            c = ort::mk(1.0f, 1.0f, 1.0f);
                            col = ort::mk(0.0f, 0.0f, 0.0f);
                            importance = 1.0f;
                            ray = radiance_ray(A.rays, cand, A.flags);
                        } else {  // not traced: zeros, the state as given
                            radiance_store(A.radiance, A.states_out, cand, ort::mk(0.0f, 0.0f, 0.0f), st);
                        }
                    }
                }
                next += take;
            }
        }
        if (!__ballot(k >= 0)) {
            if (drained) break;
            continue;
        }
        if (k >= 0) {  // one bounce of the lane's current path (radiance(), glsl:604-627)
            float t;
            int entry;
            const bool hit = pixel_trace<MODE, DEEP, LDS>(A.P, S, L, ray, t, entry);
            ort::HitRec h;
            if (hit) h = ort::hit_record<MODE>(A.P.S, ray, t, entry);
            bool ended = ort::shade_bounce(hit, h, ray, c, importance, st);
            ++b;
            ended = ended || b >= maxd || importance < 0.01f;
            if (ended) {  // col += radiance(r); the chain's next path, or the record
                col = ort::add(col, c);
                if (++s < paths) {
                    b = 0;
                    c = ort::mk(1.0f, 1.0f, 1.0f);
                    importance = 1.0f;
                    ray = radiance_ray(A.rays, k, A.flags);
                } else {
                    radiance_store(A.radiance, A.states_out, k, radiance_value(col, paths, A.flags), st);
                    k = -1;
                }
            }
        }
    }
}

constexpr int kRadianceMaxPaths = 65536;

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// What ort_trace_radiance refuses (ORT_ERR_INVALID_ARG), the emulation too.  host: the pointers
// are host pointers (the overlap rule is checked for those only).
std::string check_radiance(const void* rays, int64_t n, const float* states, const float* radiance, const float* states_out,
                           int max_depth, int paths, int flags, int reserved, bool host) {
    if (n < 0 || n > kQueryMaxRays) return "n_rays must be 0 .. 2^30";  // (as check_query)
    if (flags & ~(ORT_QUERY_SORT | ORT_RADIANCE_NORMALIZE | ORT_RADIANCE_GAMMA)) return "unknown flag bits";
    if (reserved != 0) return "reserved must be 0";
    if (n > 0 && (!rays || !states || !radiance)) return "null rays, states or radiance";
    if (((uintptr_t)rays & 3) || ((uintptr_t)states & 3) || ((uintptr_t)radiance & 3) || ((uintptr_t)states_out & 3))
        return "rays, states, radiance and states_out must be 4-byte aligned";
    if (max_depth < 1) return "max_depth must be at least 1";
    if (paths < 1 || paths > kRadianceMaxPaths) return "paths must be 1 .. 65536";
    if (host && n > 0 && states_out && states_out != states && ranges_overlap(states, 8 * (size_t)n, states_out, 8 * (size_t)n))
        return "states_out overlaps states (it may be equal to it)";
    return "";
}

int radiance_impl(ort_ctx* ctx, const ort_radiance_query* q, void* stream) {
    if (!q) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_trace_radiance: null query");
    const std::string bad = check_radiance(q->rays, q->n_rays, q->states, q->radiance, q->states_out, q->max_depth, q->paths,
                                           q->flags, q->reserved, q->on_device == 0);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_trace_radiance: " + bad);
    // the walk, as accum_mode picks it: the whole-pixel walk exists for the compact layout and brute force
    if (!ctx->scene.has_scene) return fail(ctx, ORT_ERR_NO_SCENE, "ort_trace_radiance: no scene uploaded");
    const int mode = (q->use_octree == 1) ? (ctx->scene.layout == ORT_LAYOUT_COMPACT ? 0 : 1) : 2;
    if (mode != 2 && ctx->scene.n_nodes <= 0) return fail(ctx, ORT_ERR_NO_SCENE, "ort_trace_radiance: scene has no octree");
    if (mode == 1)
        return fail(ctx, ORT_ERR_UNSUPPORTED, "ort_trace_radiance: use_octree = 1 on the explicit layout (radiance queries "
                                              "take the whole-pixel walk: compact layout or brute force)");
    QueryCall c;
    RadianceArgs a;
    std::memset(&a, 0, sizeof(a));
    QueryArgs qa;
    const size_t n = (size_t)q->n_rays;
    const QueryIo io = {q->rays, nullptr, nullptr, nullptr, q->on_device != 0, (q->flags & ORT_QUERY_SORT) != 0, false};
    int rc = query_begin(ctx, "ort_trace_radiance", true, q->use_octree, n, io, stream, c, qa);
    if (rc || c.n == 0) return rc;
    QueryState& qs = ctx->query;
    if (c.host) {  // the states in, the radiance and (in place) the end states out
        if ((rc = ensure(ctx, qs.states, 8 * n)) || (rc = ensure(ctx, qs.radiance, 12 * n))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(qs.states.p, q->states, 8 * n, hipMemcpyHostToDevice, c.s));
    }
    a.P.S = qa.S;
    a.P.exact_only = qa.exact_only;
    a.rays = qa.rays;
    a.states = c.host ? (const float*)qs.states.p : q->states;
    a.radiance = c.host ? (float*)qs.radiance.p : q->radiance;
    a.states_out = q->states_out ? (c.host ? (float*)qs.states.p : q->states_out) : nullptr;
    a.sync = qa.sync;
    a.n = qa.n;
    a.max_depth = q->max_depth;
    a.paths = q->paths;
    a.flags = q->flags;
    if ((rc = query_start(ctx, c, qa))) return rc;
    a.qlist = qa.qlist;
    bool lds_scene;
    const size_t lds = pixel_paths_lds(ctx, c.mode, a.P, lds_scene);
    const int variant = c.mode == 2 ? 0 : (ctx->scene.depth > 8 ? 1 : (lds_scene ? 2 : 3));
    pick<0, 1, 2, 3>(variant, [&](auto V) {
        constexpr int MODE = ORT_V(V) == 0 ? 2 : 0;
        constexpr bool DEEP = ORT_V(V) == 1, LDS = ORT_V(V) == 2;
        const int g = resident_blocks(ctx->device, ort_radiance_paths<MODE, DEEP, LDS>, kBlock, lds, c.blocks);
        hipLaunchKernelGGL((ort_radiance_paths<MODE, DEEP, LDS>), dim3(g), dim3(kBlock), lds, c.s, a);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_radiance_paths launch");
    // query_finish with this call's arrays: the second event, the copies back, the wait
    HIPCHK(ctx, qs.ev.end(c.s));
    if (c.host) {
        HIPCHK(ctx, hipMemcpyAsync(q->radiance, qs.radiance.p, 12 * n, hipMemcpyDeviceToHost, c.s));
        if (q->states_out) HIPCHK(ctx, hipMemcpyAsync(q->states_out, qs.states.p, 8 * n, hipMemcpyDeviceToHost, c.s));
    }
    if (c.host || !c.caller_stream) HIPCHK(ctx, hipStreamSynchronize(c.s));
    return ORT_OK;
}

#if ORT_ANALYSIS
// One ray's chain on the CPU: shade_pixel's loops (trace_ray + hit_record + shade_bounce per
// bounce) from the caller's ray and state instead of primary_ray and the pixel's seed.
template <int MODE>
void radiance_chain(const HostScene& hs, const float* rays, int64_t i, int max_depth, int paths, int flags, ort_rng& st,
                    ort::V3& col) {
    ort::LocalFrames lf;
    ort::Counters cnt;
    for (int q = 0; q < 6; ++q) cnt.v[q] = 0;
    for (int s = 0; s < paths; ++s) {
        ort::Ray ray = radiance_ray(rays, i, flags);
        ort::V3 c = ort::mk(1.0f, 1.0f, 1.0f);
        float importance = 1.0f;
        for (int b = 0; b < max_depth; ++b) {
            if (importance < 0.01f) break;
            float t;
            int entry;
            const int tr = ort::trace_ray<MODE, false>(hs.S, hs.fplanes.data(), hs.rank_lut, ray, false, t, entry, lf, nullptr,
                                                       nullptr, cnt, b > 0, hs.fplanes_b.data());
            ort::HitRec h;
            if (tr == ORT_TRACE_HIT) h = ort::hit_record<MODE>(hs.S, ray, t, entry);
            if (ort::shade_bounce(tr == ORT_TRACE_HIT, h, ray, c, importance, st)) break;
        }
        col = ort::add(col, c);
    }
}
#endif  // ORT_ANALYSIS

}  // namespace

extern "C" {

int ort_trace_radiance(ort_ctx* ctx, const ort_radiance_query* q, void* stream) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_trace_radiance: null ctx");
    try {
        return radiance_impl(ctx, q, stream);
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_trace_radiance: ") + ex.what());
    }
}

#if ORT_ANALYSIS
// TEST-ONLY host emulation (ort_internal.h): the chain of every ray, one ray after another.
int ort_debug_radiance_rays(const float* cr, const float* ma, const float* fr, int32_t n_spheres, const float* node_min,
                            const float* node_max, const int32_t* co, const int32_t* oo, const int32_t* cnt, int32_t n_nodes,
                            const int32_t* idx, int64_t n_indices, int32_t layout, int32_t use_octree, const float* rays,
                            const float* states, int64_t n_rays, int32_t max_depth, int32_t paths, int32_t flags,
                            float* radiance, float* states_out) {
    try {
        const std::string bad = check_radiance(rays, n_rays, states, radiance, states_out, max_depth, paths, flags, 0, true);
        if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_radiance_rays: " + bad);
        if (!cr || !ma || !fr || n_spheres <= 0) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_radiance_rays: bad scene argument");
        if (use_octree == 1 && layout != ORT_LAYOUT_COMPACT)
            return fail(nullptr, ORT_ERR_UNSUPPORTED, "ort_debug_radiance_rays: use_octree = 1 on the explicit layout");
        HostScene hs;
        if (int rc = hs.build(cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, layout, use_octree,
                              HostScene::kValidate | HostScene::kNoOctree))
            return fail(nullptr, rc, hs.error);
        for (int64_t i = 0; i < n_rays; ++i) {
            ort_rng st;
            st.x = states[2 * (size_t)i];
            st.y = states[2 * (size_t)i + 1];
            ort::V3 v = ort::mk(0.0f, 0.0f, 0.0f);
            if (radiance_state_ok(st)) {
                ort::V3 col = ort::mk(0.0f, 0.0f, 0.0f);
                if (hs.mode == 0) radiance_chain<0>(hs, rays, i, max_depth, paths, flags, st, col);
                else radiance_chain<2>(hs, rays, i, max_depth, paths, flags, st, col);
                v = radiance_value(col, paths, flags);
            }
            radiance_store(radiance, states_out, i, v, st);
        }
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}
#endif  // ORT_ANALYSIS

}  // extern "C"
