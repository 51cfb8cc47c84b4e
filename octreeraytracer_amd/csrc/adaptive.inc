// adaptive.inc -- adaptive accumulations (ort_accum_begin_ex with ORT_ACCUM_ADAPTIVE,
// ort_accum_render_adaptive, ort_accum_read_counts, ort_accum_adaptive_stats).  Included by
// ort_kernel.hip after accum_moments.inc, so that every earlier kernel keeps its place and its code:
// the adaptive passes are ort_pixel_paths<..., PM 5>, instantiated here for the four walk variants,
// and nothing else names them.
//   ort_pixel_paths<MODE, DEEP, LDS, 5>  a moments pass (accum_moments.inc) in which a lane, at its
//                                        refill, reads the slot's count k -- the int plane after m2 --
//                                        and the decision below: held, it writes the preview pixel
//                                        and stays idle for the next candidate (as a padding row);
//                                        traced, it starts at s = k from the stored state.  In tile
//                                        order (a pass that traces every pixel below N) the test
//                                        finds the finished pixels; over a list it finds nothing.  The
//                                        lane's end sample is recomputed at each sample's end from
//                                        the still-unwritten count[k] + n_samples (m2's trick: no
//                                        register more lives across the walk); the count is written
//                                        with the state at the pixel's last sample of the pass
//   ort_accum_adaptive_list              the pre-pass of a pass whose criterion may hold pixels: lists the
//                                        slots to trace (and writes the held pixels' preview); the pass
//                                        then takes its candidates from the list, 64 at a time, as the
//                                        fixup launch of a speculating frame does.  Skipping held
//                                        pixels at the refill alone cost a pass that holds everything
//                                        half a uniform pass (DESIGN.md 4.16 (b))
//   ort_accum_adaptive_resolve           stored sums and counts -> mean, variance and counts, tight,
//                                        one thread per path slot, each pixel at its own count
//   ort_accum_adaptive_reduce / _final   the stats record: per workgroup a partial record (LDS tree,
//                                        no atomics), then one workgroup over the partials
// adaptive_traces is the decision (include/ort.h), shared by the pass, the pre-pass, the stats kernel
// and the host emulation.  The pass's parameters travel in PipeArgs fields no whole-pixel pass reads:
// sample != 0 says the stored counts are valid (0: a fresh or restarted accumulation, every count
// reads as 0), sp_nch the pass's n_samples, hcap min_samples, gthr[0] threshold, gthr[1] the floor.

namespace {

// Does a pass trace the pixel that holds k of N samples with colour sum col and m2 (m2 is not
// read for k < 2)?
ORT_FN bool adaptive_traces(int k, int N, int min_samples, float threshold, float luminance_floor, ort::V3 col, float m2) {
    if (k >= N) return false;
    if (k < min_samples || threshold == 0.0f || k < 2) return true;  // (k < 2: no estimate)
    ort::V3 mean;
    float variance;
    accum_moments_pixel(col, m2, k, mean, variance);
    if (variance < 0.0f) return true;  // no estimate: a non-finite sum
    const float L = (0.2126f * mean.x + 0.7152f * mean.y) + 0.0722f * mean.z;
    const float ref = L > luminance_floor ? L : luminance_floor;
    const float tol = threshold * ref;
    return !(variance <= tol * tol);
}

__device__ __forceinline__ const int* adaptive_counts(const PipeArgs& A) {
    return reinterpret_cast<const int*>(A.fx_col) + 4 * (size_t)A.total;
}

// mean, variance, counts: NULL, or tight planes of the tile (row j first).
__global__ void __launch_bounds__(256) ort_accum_adaptive_resolve(PipeArgs A, float* mean, float* variance, int32_t* counts) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= A.total) return;
    int cx, cy;
    if (!slot_coords(A, k, cx, cy)) return;
    const size_t i = (size_t)cy * (size_t)A.tm.tw + (size_t)cx;
    ort::V3 m = ort::mk(0.0f, 0.0f, 0.0f);
    float v = -1.0f;
    int n = 0;
    if (tile_row_to_y(A.tm, cy) < A.pp.H) {
        n = A.sample ? adaptive_counts(A)[k] : 0;
        if (n >= 1 && (mean || variance)) {
            const ort::V3 col = ort::mk(A.fx_col[k], A.fx_col[(size_t)A.total + k], A.fx_col[2 * (size_t)A.total + k]);
            const float m2 = (variance && n >= 2) ? A.fx_col[3 * (size_t)A.total + k] : 0.0f;
            accum_moments_pixel(col, m2, n, m, v);
        }
    }
    if (mean) {
        mean[3 * i] = m.x;
        mean[3 * i + 1] = m.y;
        mean[3 * i + 2] = m.z;
    }
    if (variance) variance[i] = v;
    if (counts) counts[i] = n;
}

// The pre-pass of a pass that may hold pixels: the decision per slot; a traced slot goes onto the
// list (A.fx_slot, *A.fx_n: a wave's slots together and in order, one atomic per wave), a held pixel
// and a padding row get their preview pixel when there is an output.
__global__ void __launch_bounds__(256) ort_accum_adaptive_list(PipeArgs A) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    bool traced = false;
    int cx, cy;
    if (k < A.total && slot_coords(A, k, cx, cy)) {
        const int y = tile_row_to_y(A.tm, cy);
        if (y >= A.pp.H) {
            if (A.out) store_padding(A, cy, cx);
        } else {
            const int n = A.sample ? adaptive_counts(A)[k] : 0;
            ort::V3 col = ort::mk(0.0f, 0.0f, 0.0f);
            float m2 = 0.0f;
            if (n >= 1) col = ort::mk(A.fx_col[k], A.fx_col[(size_t)A.total + k], A.fx_col[2 * (size_t)A.total + k]);
            if (n >= 2) m2 = A.fx_col[3 * (size_t)A.total + k];
            traced = adaptive_traces(n, A.pp.ns, A.hcap, A.gthr[0], A.gthr[1], col, m2);
            if (!traced && A.out) store_pixel(A, cy, cx, y, ort::finish_pixel(col, n));
        }
    }
    const unsigned long long m = __ballot(traced);
    if (m) {
        const int lane = threadIdx.x & 63;
        int base = 0;
        if (lane == 0) base = atomicAdd(A.fx_n, __popcll(m));
        base = __shfl(base, 0);
        if (traced) A.fx_slot[base + __popcll(m & ((1ull << lane) - 1ull))] = k;
    }
}

void launch_adaptive_list(const PipeArgs& a, size_t slots, hipStream_t s) {
    hipLaunchKernelGGL(ort_accum_adaptive_list, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, a);
}

constexpr int kAdaptiveStatBlocks = 256;  // partial records (and the final one after them)

struct AdaptiveStat {
    long long pixels, samples, pending;
    int lo, hi;
};
__device__ __forceinline__ void adaptive_stat_merge(AdaptiveStat& a, const AdaptiveStat& b) {
    a.pixels += b.pixels;
    a.samples += b.samples;
    a.pending += b.pending;
    a.lo = min(a.lo, b.lo);
    a.hi = max(a.hi, b.hi);
}
__device__ __forceinline__ void adaptive_stat_block(AdaptiveStat& r) {  // thread 0 ends with the workgroup's
    __shared__ AdaptiveStat sh[256];
    sh[threadIdx.x] = r;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) adaptive_stat_merge(sh[threadIdx.x], sh[threadIdx.x + d]);
        __syncthreads();
    }
    r = sh[0];
}

// Workgroup b's record over the slots b * 256 + t, + gridDim.x * 256, ...: part[b].
__global__ void __launch_bounds__(256) ort_accum_adaptive_reduce(PipeArgs A, AdaptiveStat* part) {
    AdaptiveStat r = {0, 0, 0, 0x7fffffff, 0};
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < (long long)A.total; k += (long long)gridDim.x * 256) {
        int cx, cy;
        if (!slot_coords(A, (int)k, cx, cy) || tile_row_to_y(A.tm, cy) >= A.pp.H) continue;
        const int n = A.sample ? adaptive_counts(A)[k] : 0;
        ort::V3 col = ort::mk(0.0f, 0.0f, 0.0f);
        float m2 = 0.0f;
        if (n >= 1) col = ort::mk(A.fx_col[k], A.fx_col[(size_t)A.total + k], A.fx_col[2 * (size_t)A.total + k]);
        if (n >= 2) m2 = A.fx_col[3 * (size_t)A.total + k];
        r.pixels += 1;
        r.samples += n;
        r.pending += adaptive_traces(n, A.pp.ns, A.hcap, A.gthr[0], A.gthr[1], col, m2) ? 1 : 0;
        r.lo = min(r.lo, n);
        r.hi = max(r.hi, n);
    }
    adaptive_stat_block(r);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// part[0 .. n-1] -> part[kAdaptiveStatBlocks]
__global__ void __launch_bounds__(256) ort_accum_adaptive_final(AdaptiveStat* part, int n) {
    AdaptiveStat r = {0, 0, 0, 0x7fffffff, 0};
    if ((int)threadIdx.x < n) r = part[threadIdx.x];
    adaptive_stat_block(r);
    if (threadIdx.x == 0) {
        if (r.pixels == 0) r.lo = 0;
        part[kAdaptiveStatBlocks] = r;
    }
}

hipError_t launch_accum_adaptive_paths(int device, int mode, bool deep, bool lds_scene, size_t lds, long long needed,
                                       const PipeArgs& a, hipStream_t s) {
    const int variant = mode == 2 ? 0 : (deep ? 1 : (lds_scene ? 2 : 3));
    pick<0, 1, 2, 3>(variant, [&](auto V) {
        constexpr int MODE = ORT_V(V) == 0 ? 2 : 0;
        constexpr bool DEEP = ORT_V(V) == 1, LDS = ORT_V(V) == 2;
        const int g = resident_blocks(device, ort_pixel_paths<MODE, DEEP, LDS, 5>, kBlock, lds, needed);
        hipLaunchKernelGGL((ort_pixel_paths<MODE, DEEP, LDS, 5>), dim3(g), dim3(kBlock), lds, s, a);
    });
    return hipGetLastError();
}

void launch_adaptive_resolve(const PipeArgs& a, size_t slots, float* mean, float* variance, int32_t* counts, hipStream_t s) {
    hipLaunchKernelGGL(ort_accum_adaptive_resolve, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, a, mean, variance,
                       counts);
}

// What ort_accum_render_adaptive and ort_accum_adaptive_stats refuse in a criterion ("" = fine).
std::string check_adaptive(const ort_accum_adaptive* a) {
    if (a->n_samples < 1) return "n_samples must be at least 1";
    if (a->min_samples < 0) return "min_samples must not be negative";
    if (!(a->threshold >= 0.0f)) return "threshold must not be negative or NaN";
    if (!(a->luminance_floor > 0.0f) || !am_finite(a->luminance_floor)) return "luminance_floor must be finite and positive";
    if (a->reserved[0] != 0 || a->reserved[1] != 0 || a->reserved[2] != 0 || a->reserved[3] != 0) return "reserved must be 0";
    return "";
}

// The checks the three calls share; who: the call's name.
int adaptive_known(ort_ctx* ctx, ort_accum* acc, const char* who) {
    if (!accum_known(ctx, acc)) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + ": not an accumulation of this context");
    if (!acc->adaptive)
        return fail(ctx, ORT_ERR_INVALID_ARG,
                    std::string(who) + ": needs an accumulation begun with ORT_ACCUM_ADAPTIVE (ort_accum_begin_ex)");
    return ORT_OK;
}

int adaptive_scene(ort_ctx* ctx, ort_accum* acc, const char* who) {
    if (acc->scene_gen != ctx->scene.scene_gen || !ctx->scene.has_scene)
        return fail(ctx, ORT_ERR_NO_SCENE,
                    std::string(who) + ": the scene changed since the accumulation was begun (ort_accum_restart starts "
                                       "it again on the new scene)");
    return ORT_OK;
}

// The argument block of the resolve and the stats kernels: the passes' slot order and state.
PipeArgs adaptive_state_args(ort_ctx* ctx, ort_accum* acc) {
    const ort_tile* t = &acc->t;
    const int tilesX = (t->width + 15) / 16, tilesY = (t->rows + 15) / 16;
    const size_t slots = (size_t)acc->blocks * kBlock;
    const DevOutput none = {nullptr, 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE};
    PipeArgs a = base_args(ctx, &acc->p, t, none, tilesX, tilesY, acc->blocks);
#if ORT_ANALYSIS
    a.wclock = nullptr;
    a.wclock_n = 0;
#endif
    a.fx_col = (float*)((char*)acc->state.p + sizeof(float2) * slots);
    a.sample = acc->done;
    a.sp_chunk = acc->done;
    return a;
}

int accum_read_counts_impl(ort_ctx* ctx, ort_accum* acc, int32_t* counts, int on_device, void* stream) {
    const ort_tile* t = &acc->t;
    const size_t pix = (size_t)t->width * (size_t)t->rows;
    if (pix == 0) return ORT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    int32_t* d_counts = counts;
    if (!on_device) {  // tight on the device, copied out
        int rc;
        if ((rc = ensure(ctx, acc->astage, std::max<size_t>(4 * pix, sizeof(AdaptiveStat) * (kAdaptiveStatBlocks + 1))))) return rc;
        d_counts = (int32_t*)acc->astage.p;
    }
    const PipeArgs a = adaptive_state_args(ctx, acc);
    launch_adaptive_resolve(a, (size_t)acc->blocks * kBlock, nullptr, nullptr, d_counts, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_accum_adaptive_resolve launch");
    if (!on_device) {
        HIPCHK(ctx, hipMemcpyAsync(counts, d_counts, 4 * pix, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    } else if (!stream) {
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return ORT_OK;
}

int accum_adaptive_stats_impl(ort_ctx* ctx, ort_accum* acc, const ort_accum_adaptive* c, struct ort_accum_adaptive_stats* out) {
    std::memset(out, 0, sizeof *out);
    const ort_tile* t = &acc->t;
    const size_t pix = (size_t)t->width * (size_t)t->rows;
    if (pix == 0) return ORT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = ensure(ctx, acc->astage, std::max<size_t>(4 * pix, sizeof(AdaptiveStat) * (kAdaptiveStatBlocks + 1))))) return rc;
    AdaptiveStat* part = (AdaptiveStat*)acc->astage.p;
    PipeArgs a = adaptive_state_args(ctx, acc);
    const int N = acc->p.num_samples;
    a.sp_nch = std::min(c->n_samples, N);
    a.hcap = std::min(c->min_samples, N);
    a.gthr[0] = c->threshold;
    a.gthr[1] = c->luminance_floor;
    const int g = (int)std::min<long long>(acc->blocks, kAdaptiveStatBlocks);
    hipLaunchKernelGGL(ort_accum_adaptive_reduce, dim3(g), dim3(256), 0, s, a, part);
    hipLaunchKernelGGL(ort_accum_adaptive_final, dim3(1), dim3(256), 0, s, part, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_accum_adaptive_reduce launch");
    AdaptiveStat r;
    HIPCHK(ctx, hipMemcpyAsync(&r, part + kAdaptiveStatBlocks, sizeof r, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    out->pixels = r.pixels;
    out->samples = r.samples;
    out->pending = r.pending;
    out->min_count = r.lo;
    out->max_count = r.hi;
    return ORT_OK;
}

}  // namespace

extern "C" {

int ort_accum_render_adaptive(ort_ctx* ctx, ort_accum* accum, const ort_accum_adaptive* pass, const ort_output* output,
                              void* stream) {
    const char* who = "ort_accum_render_adaptive";
    if (!ctx || !accum || !pass) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (int rc = adaptive_known(ctx, accum, who)) return rc;
    const std::string bad = check_adaptive(pass);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + ": " + bad);
    return accum_render_impl(ctx, accum, pass->n_samples, output, stream, pass);
}

int ort_accum_read_counts(ort_ctx* ctx, ort_accum* accum, int32_t* counts, int32_t on_device, void* stream) {
    const char* who = "ort_accum_read_counts";
    if (!ctx || !accum || !counts) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (int rc = adaptive_known(ctx, accum, who)) return rc;
    if ((uintptr_t)counts & 3) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + ": counts must be 4-byte aligned");
    if (int rc = adaptive_scene(ctx, accum, who)) return rc;
    return accum_read_counts_impl(ctx, accum, counts, on_device, stream);
}

int ort_accum_adaptive_stats(ort_ctx* ctx, ort_accum* accum, const ort_accum_adaptive* criterion,
                             struct ort_accum_adaptive_stats* out) {
    const char* who = "ort_accum_adaptive_stats";
    if (!ctx || !accum || !criterion || !out) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (int rc = adaptive_known(ctx, accum, who)) return rc;
    const std::string bad = check_adaptive(criterion);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + ": " + bad);
    if (int rc = adaptive_scene(ctx, accum, who)) return rc;
    return accum_adaptive_stats_impl(ctx, accum, criterion, out);
}

#if ORT_ANALYSIS
// TEST-ONLY (ort_internal.h): an adaptive accumulation driven by `passes`, on the host CPU: per pixel
// and pass the shared decision on the state at the pixel's count, and, where it traces, shade_pixel's
// chain to the new count (the chain from sample 0: a pixel's state at k is the k-sample prefix's).
int ort_debug_emulate_adaptive(const float* cr, const float* ma, const float* fr, int32_t n_spheres, const float* node_min,
                               const float* node_max, const int32_t* co, const int32_t* oo, const int32_t* cnt,
                               int32_t n_nodes, const int32_t* idx, int64_t n_indices, int32_t layout, const ort_params* p,
                               const ort_tile* t, const ort_accum_adaptive* passes, int32_t n_passes, int32_t* counts,
                               float* mean, float* variance) {
    try {
        const std::string bad = check_frame_tile(p, t);
        if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, bad);
        if (n_passes < 0 || (n_passes > 0 && !passes)) return fail(nullptr, ORT_ERR_INVALID_ARG, "passes: null or a negative number");
        if (!counts && !mean && !variance) return fail(nullptr, ORT_ERR_INVALID_ARG, "counts, mean and variance are all NULL");
        for (int i = 0; i < n_passes; ++i) {
            const std::string bad_pass = check_adaptive(passes + i);
            if (!bad_pass.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, "pass " + std::to_string(i) + ": " + bad_pass);
        }
        HostScene hs;
        if (int rc = hs.build(cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices,
                              layout == 2 ? ORT_LAYOUT_COMPACT : layout, p->use_octree, HostScene::kValidate | HostScene::kNoOctree))
            return fail(nullptr, rc, hs.error);
        const ort::KScene& S = hs.S;
        const ort::PixelParams pp = pixel_params(p);
        const TileMap tm = {t->x0, t->width, t->y0, t->rows, t->band_height, t->band_stride};
        const uint8_t* rank_lut = layout == ORT_LAYOUT_COMPACT ? hs.rank_lut : nullptr;
        std::vector<int> snode(ORT_MAX_STACK);
        std::vector<float> stmin(ORT_MAX_STACK);
        ort::LocalFrames lf;
        const int N = p->num_samples;
        for (int row = 0; row < t->rows; ++row) {
            const int y = tile_row_to_y(tm, row);
            for (int c = 0; c < t->width; ++c) {
                const size_t i = (size_t)row * t->width + c;
                ort::V3 m = ort::mk(0.0f, 0.0f, 0.0f);
                float v = -1.0f;
                int k = 0;
                if (y < p->height) {
                    ort::V3 col = ort::mk(0.0f, 0.0f, 0.0f);
                    float m2 = 0.0f;
                    for (int q = 0; q < n_passes; ++q) {
                        const ort_accum_adaptive& a = passes[q];
                        if (!adaptive_traces(k, N, std::min(a.min_samples, N), a.threshold, a.luminance_floor, col, m2)) continue;
                        k = std::min(k + std::min(a.n_samples, N), N);
                        ort::Counters cc;
                        for (int j = 0; j < 6; ++j) cc.v[j] = 0;
                        if (hs.mode == 0)
                            (void)ort::shade_pixel<0, false>(pp, S, hs.fplanes.data(), hs.fplanes_b.data(), rank_lut, lf, nullptr,
                                                             nullptr, t->x0 + c, y, cc, k, &col, &m2);
                        else if (hs.mode == 1)
                            (void)ort::shade_pixel<1, false>(pp, S, nullptr, nullptr, nullptr, lf, snode.data(), stmin.data(),
                                                             t->x0 + c, y, cc, k, &col, &m2);
                        else
                            (void)ort::shade_pixel<2, false>(pp, S, nullptr, nullptr, nullptr, lf, nullptr, nullptr, t->x0 + c, y,
                                                             cc, k, &col, &m2);
                    }
                    if (k >= 1) accum_moments_pixel(col, m2, k, m, v);
                }
                if (counts) counts[i] = k;
                if (mean) {
                    mean[3 * i] = m.x;
                    mean[3 * i + 1] = m.y;
                    mean[3 * i + 2] = m.z;
                }
                if (variance) variance[i] = v;
            }
        }
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

// TEST-ONLY (ort_internal.h): the shared decision for one stored state.
int ort_debug_adaptive_decision(int32_t k, int32_t n_total, const ort_accum_adaptive* criterion, const float* col, float m2) {
    if (!criterion || !col || k < 0 || n_total < 1 || !check_adaptive(criterion).empty()) return -1;
    return adaptive_traces(k, n_total, std::min(criterion->min_samples, n_total), criterion->threshold,
                           criterion->luminance_floor, ort::mk(col[0], col[1], col[2]), m2)
               ? 1
               : 0;
}
#endif  // ORT_ANALYSIS

}  // extern "C"
