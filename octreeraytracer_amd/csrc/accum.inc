// accum.inc -- progressive frames (ort_accum_*): a frame's samples accumulated over several calls.
// Included by ort_kernel.hip after the render path and the ray queries, so that every kernel of
// theirs keeps its place and its code: the passes are ort_pixel_paths<..., PM 3>, instantiated
// here for the four walk variants, and nothing else names them.
//   ort_pixel_paths<MODE, DEEP, LDS, 3>  a pass: samples s0 .. s1-1 of every pixel of the tile, each
//                                        pixel's chain continued from its slot's stored RNG state
//                                        and colour sum (s0 == 0: from the pixel's seed), both
//                                        stored back; with an output, the picture of s1 samples
//   ort_accum_resolve                    stored sums -> the picture (a call on a finished accumulation)
// An accumulation owns its state, its cursor and done count and its timing events (ort_accum): a
// pass reads the scene and the context's options, and nothing of the per-frame render state --
// the counter sets, the speculation buffers, the heavy-first lists, the frame timing ring.

namespace {

// The picture of A.sp_chunk samples from the stored sums; padding rows as the passes write them.
__global__ void __launch_bounds__(256) ort_accum_resolve(PipeArgs A) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= A.total) return;
    int cx, cy;
    if (!slot_coords(A, k, cx, cy)) return;
    if (tile_row_to_y(A.tm, cy) >= A.pp.H) {
        store_padding(A, cy, cx);
        return;
    }
    const ort::V3 col = ort::mk(A.fx_col[k], A.fx_col[(size_t)A.total + k], A.fx_col[2 * (size_t)A.total + k]);
    store_pixel(A, cy, cx, -1, ort::finish_pixel(col, A.sp_chunk));
}

// One pass launch: the variant of the scene's walk, as launch_pixel_paths picks it.
hipError_t launch_accum_paths(int device, int mode, bool deep, bool lds_scene, size_t lds, long long needed,
                              const PipeArgs& a, hipStream_t s) {
    const int variant = mode == 2 ? 0 : (deep ? 1 : (lds_scene ? 2 : 3));
    pick<0, 1, 2, 3>(variant, [&](auto V) {
        constexpr int MODE = ORT_V(V) == 0 ? 2 : 0;
        constexpr bool DEEP = ORT_V(V) == 1, LDS = ORT_V(V) == 2;
        const int g = resident_blocks(device, ort_pixel_paths<MODE, DEEP, LDS, 3>, kBlock, lds, needed);
        hipLaunchKernelGGL((ort_pixel_paths<MODE, DEEP, LDS, 3>), dim3(g), dim3(kBlock), lds, s, a);
    });
    return hipGetLastError();
}

// The same launch for an accumulation that keeps moments: ort_pixel_paths<..., 4>, named in
// accum_moments.inc so that those kernels follow every other one.
hipError_t launch_accum_moments_paths(int device, int mode, bool deep, bool lds_scene, size_t lds, long long needed,
                                      const PipeArgs& a, hipStream_t s);
// ... and for an adaptive one: ort_pixel_paths<..., 5>, named in adaptive.inc, after those.
hipError_t launch_accum_adaptive_paths(int device, int mode, bool deep, bool lds_scene, size_t lds, long long needed,
                                       const PipeArgs& a, hipStream_t s);
void launch_adaptive_list(const PipeArgs& a, size_t slots, hipStream_t s);

// The walk an accumulation of params p takes on ctx's scene (0 compact, 2 brute force), or the
// refusal: what the whole-pixel kernel does not exist for.
int accum_mode(ort_ctx* ctx, const ort_params* p, const char* call, int& mode) {
    const std::string who = std::string(call) + ": ";
    if (!ctx->scene.has_scene) return fail(ctx, ORT_ERR_NO_SCENE, who + "no scene uploaded");
    mode = (p->use_octree == 1) ? (ctx->scene.layout == ORT_LAYOUT_COMPACT ? 0 : 1) : 2;
    if (mode != 2 && ctx->scene.n_nodes <= 0) return fail(ctx, ORT_ERR_NO_SCENE, who + "scene has no octree");
    if (mode == 1)
        return fail(ctx, ORT_ERR_UNSUPPORTED, who + "use_octree = 1 on the explicit layout (passes take the whole-pixel "
                                                    "kernel: compact layout or brute force)");
    if (p->max_depth < 1) return fail(ctx, ORT_ERR_UNSUPPORTED, who + "max_depth must be at least 1");
    return ORT_OK;
}

bool accum_known(const ort_ctx* ctx, const ort_accum* acc) {
    return acc->ctx == ctx && std::find(ctx->accums.begin(), ctx->accums.end(), acc) != ctx->accums.end();
}

int accum_begin_impl(ort_ctx* ctx, const ort_params* p, const ort_tile* t, int flags, ort_accum** out) {
    *out = nullptr;
    if (flags & ~(ORT_ACCUM_MOMENTS | ORT_ACCUM_ADAPTIVE)) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_begin_ex: unknown flag bits");
    const std::string bad = check_params(p, t);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_begin: " + bad);
    int mode = 0, rc;
    if ((rc = accum_mode(ctx, p, "ort_accum_begin", mode))) return rc;
    const long long blocks = (long long)((t->width + 15) / 16) * ((t->rows + 15) / 16);
    if (blocks * kBlock > 0x7fffffffLL) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_begin: tile too large");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ort_accum* acc = new (std::nothrow) ort_accum();
    if (!acc) return fail(ctx, ORT_ERR_OUT_OF_MEMORY, "ort_accum_begin: out of host memory");
    acc->ctx = ctx;
    acc->p = *p;
    acc->t = *t;
    acc->mode = mode;
    acc->adaptive = (flags & ORT_ACCUM_ADAPTIVE) != 0;
    acc->moments = acc->adaptive || (flags & ORT_ACCUM_MOMENTS) != 0;
    acc->blocks = blocks;
    acc->scene_gen = ctx->scene.scene_gen;
    const size_t slots = (size_t)blocks * kBlock;
    hipError_t e = hipSuccess;
    if ((rc = ensure(ctx, acc->state, std::max<size_t>((acc->adaptive ? 28 : acc->moments ? 24 : 20) * slots, 16))) || (rc = ensure(ctx, acc->sync, 64)) ||
        (e = acc->ev.create()) != hipSuccess) {
        if (!rc) rc = hip_fail(ctx, e, "ort_accum_begin: events");
        free_accum(acc);
        return rc;
    }
    ctx->accums.push_back(acc);
    *out = acc;
    return ORT_OK;
}

int accum_restart_impl(ort_ctx* ctx, ort_accum* acc, const ort_params* p) {
    const std::string bad = check_params(p, &acc->t);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_restart: " + bad);
    if (p->width != acc->p.width || p->height != acc->p.height || p->num_samples != acc->p.num_samples ||
        p->max_depth != acc->p.max_depth || p->use_octree != acc->p.use_octree)
        return fail(ctx, ORT_ERR_INVALID_ARG,
                    "ort_accum_restart: width, height, num_samples, max_depth and use_octree must be those of "
                    "ort_accum_begin (the state has that shape)");
    int mode = 0, rc;
    if ((rc = accum_mode(ctx, p, "ort_accum_restart", mode))) return rc;  // (the scene may be another one)
    acc->p = *p;
    acc->mode = mode;
    acc->done = 0;
    acc->scene_gen = ctx->scene.scene_gen;
    return ORT_OK;
}

// ad: the criterion of a pass on an adaptive accumulation (ort_accum_render_adaptive, checked there), or
// NULL: ort_accum_render, which on an adaptive accumulation traces every pixel below N.
int accum_render_impl(ort_ctx* ctx, ort_accum* acc, int n_samples, const ort_output* o, void* stream,
                      const ort_accum_adaptive* ad = nullptr) {
    if (n_samples < 1) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_render: n_samples must be at least 1");
    const ort_params* p = &acc->p;
    const ort_tile* t = &acc->t;
    const size_t pix = (size_t)t->width * (size_t)t->rows;
    if (o) {
        const std::string bad_out = check_output(p, t, o);
        if (!bad_out.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_render: " + bad_out);
        if (!o->data && pix > 0) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_render: null output data");
    }
    if (acc->scene_gen != ctx->scene.scene_gen || !ctx->scene.has_scene)
        return fail(ctx, ORT_ERR_NO_SCENE,
                    "ort_accum_render: the scene changed since the accumulation was begun (ort_accum_restart starts "
                    "it again on the new scene)");
    const int N = p->num_samples;
    const int s0 = acc->done, s1 = s0 + std::min(n_samples, N - s0);
    if (pix == 0) {
        acc->done = s1;
        return ORT_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const int tilesX = (t->width + 15) / 16, tilesY = (t->rows + 15) / 16;
    const size_t slots = (size_t)acc->blocks * kBlock;
    DevOutput dout = {nullptr, 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE};
    long long pitch = 0;
    int rc;
    if (o) {
        const long long tight = (long long)(o->placement == ORT_PLACE_FRAME ? p->width : t->width) * format_bpp(o->format);
        pitch = o->row_pitch_bytes ? (long long)o->row_pitch_bytes : tight;
        dout = {o->data, pitch, o->format, o->placement};
        if (!o->is_device) {  // the tight picture on the device, copied out (finish_output)
            if ((rc = ensure(ctx, acc->stage, (size_t)format_bpp(o->format) * pix))) return rc;
            dout.data = acc->stage.p;
            dout.pitch = tight;
        }
    }
    PipeArgs a = base_args(ctx, p, t, dout, tilesX, tilesY, acc->blocks);
#if ORT_ANALYSIS
    a.wclock = nullptr;  // (the frames' analysis records)
    a.wclock_n = 0;
#endif
    a.sync = (int*)acc->sync.p;
    a.fx_st = (float2*)acc->state.p;
    a.fx_col = (float*)((char*)acc->state.p + sizeof(float2) * slots);
    a.sample = s0;
    a.sp_chunk = s1;
    if (acc->adaptive) {  // (adaptive.inc: the pass's samples and the criterion, in fields no whole-pixel pass reads)
        a.sp_nch = std::min(n_samples, N);
        a.hcap = ad ? std::min(ad->min_samples, N) : 0;
        a.gthr[0] = ad ? ad->threshold : 0.0f;
        a.gthr[1] = ad ? ad->luminance_floor : 1.0f;
        // a criterion that may hold pixels: the pre-pass lists the slots to trace and writes the others'
        // preview; else -- threshold 0, or no pixel can have min_samples yet (no count exceeds s0) --
        // every pixel below N is traced, in tile order, which keeps neighbouring blocks together
        // (DESIGN.md 4.16 (b)).  The list's length lives after the list, in a cache line of its own:
        // the cursor's line is under every wave's atomics
        if (ad && ad->threshold != 0.0f && s0 != 0 && s0 >= ad->min_samples) {
            if ((rc = ensure(ctx, acc->alist, 4 * slots + 256))) return rc;
            a.fx_slot = (int*)acc->alist.p;
            a.fx_n = (int*)((char*)acc->alist.p + 4 * slots + 128);
        }
    }
    HIPCHK(ctx, acc->ev.begin(s));
    if (s1 > s0 || acc->adaptive) {  // (adaptive: some pixels may sit below N whatever the passes' sum)
        HIPCHK(ctx, hipMemsetAsync(acc->sync.p, 0, 64, s));
        bool lds_scene;
        const size_t lds = pixel_paths_lds(ctx, acc->mode, a, lds_scene);
        if (a.fx_slot) {
            HIPCHK(ctx, hipMemsetAsync(a.fx_n, 0, 4, s));
            launch_adaptive_list(a, slots, s);
            const hipError_t el = hipGetLastError();
            if (el != hipSuccess) return hip_fail(ctx, el, "ort_accum_adaptive_list launch");
        }
        const hipError_t e = (acc->adaptive ? launch_accum_adaptive_paths : acc->moments ? launch_accum_moments_paths : launch_accum_paths)(
            ctx->device, acc->mode, ctx->scene.depth > 8, lds_scene, lds, acc->blocks, a, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "ort_pixel_paths (accumulation pass) launch");
        acc->done = s1;
    } else if (o) {  // finished before the call: the frame again, from the stored sums
        hipLaunchKernelGGL(ort_accum_resolve, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(ctx, e, "ort_accum_resolve launch");
    }
    HIPCHK(ctx, acc->ev.end(s));
    if (o) return finish_output(ctx, o, dout, t, pitch, stream, s);
    if (!stream) HIPCHK(ctx, hipStreamSynchronize(s));
    return ORT_OK;
}

}  // namespace

extern "C" {

int ort_accum_begin(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, ort_accum** out) {
    if (!ctx || !out) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_begin: null argument");
    try {
        return accum_begin_impl(ctx, params, tile, 0, out);
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_accum_begin: ") + ex.what());
    }
}

int ort_accum_render(ort_ctx* ctx, ort_accum* accum, int32_t n_samples, const ort_output* output, void* stream) {
    if (!ctx || !accum) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_render: null argument");
    if (!accum_known(ctx, accum)) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_render: not an accumulation of this context");
    return accum_render_impl(ctx, accum, n_samples, output, stream);
}

int ort_accum_restart(ort_ctx* ctx, ort_accum* accum, const ort_params* params) {
    if (!ctx || !accum || !params) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_restart: null argument");
    if (!accum_known(ctx, accum)) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_restart: not an accumulation of this context");
    return accum_restart_impl(ctx, accum, params);
}

int ort_accum_get_info(const ort_accum* accum, ort_accum_info* info) {
    if (!accum || !info) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_accum_get_info: null argument");
    info->samples_done = accum->done;
    info->samples_total = accum->p.num_samples;
    info->device_bytes = (int64_t)(accum->state.bytes + accum->sync.bytes + accum->stage.bytes + accum->mstage.bytes +
                                     accum->astage.bytes + accum->alist.bytes);
    return ORT_OK;
}

int ort_accum_last_pass_ms(ort_ctx* ctx, ort_accum* accum, float* ms) {
    if (!ctx || !accum || !ms) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_last_pass_ms: null argument");
    if (!accum_known(ctx, accum))
        return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_last_pass_ms: not an accumulation of this context");
    if (!accum->ev.timed) return fail(ctx, ORT_ERR_NO_SCENE, "no pass launched yet");
    HIPCHK(ctx, accum->ev.elapsed(ms));
    return ORT_OK;
}

int ort_accum_free(ort_ctx* ctx, ort_accum* accum) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_accum_free: null ctx");
    if (!accum) return ORT_OK;
    if (!accum_known(ctx, accum)) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_free: not an accumulation of this context");
    (void)hipSetDevice(ctx->device);
    if (accum->ev.timed) (void)hipEventSynchronize(accum->ev.ev1);  // its last pass has left the state
    ctx->accums.erase(std::find(ctx->accums.begin(), ctx->accums.end(), accum));
    free_accum(accum);
    return ORT_OK;
}

}  // extern "C"
