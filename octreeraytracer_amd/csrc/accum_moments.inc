// accum_moments.inc -- accumulations that keep luminance moments (ort_accum_begin_ex with
// ORT_ACCUM_MOMENTS, ort_accum_read_moments).  Included by ort_kernel.hip after denoise.inc, so that
// every earlier kernel keeps its place and its code: the moments passes are ort_pixel_paths<..., PM 4>,
// instantiated here for the four walk variants, and nothing else names them.
//   ort_pixel_paths<MODE, DEEP, LDS, 4>  a pass (accum.inc) that also adds each sample's squared
//                                        luminance to the slot's m2, the float plane after the three
//                                        colour-sum planes: read, added to and written at the sample's
//                                        end, so no register more lives across the walk
//   ort_accum_moments_resolve            stored sums -> the linear mean and the variance of the mean's
//                                        luminance, tight, one thread per path slot
// accum_moments_pixel is the arithmetic (include/ort.h), shared by the kernel and the host emulation.

namespace {

ORT_FN bool am_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

// A pixel's mean and variance from its colour sum, its m2 and the samples done (m2 is not read
// for k < 2).
ORT_FN void accum_moments_pixel(ort::V3 col, float m2, int k, ort::V3& mean, float& variance) {
    const float fk = (float)k;
    mean = col;
    if (k != 1) mean = ort::mk(col.x / fk, col.y / fk, col.z / fk);  // finish_pixel's division
    variance = -1.0f;
    if (k < 2) return;
    const float L = (0.2126f * mean.x + 0.7152f * mean.y) + 0.0722f * mean.z;
    const float e2 = m2 / fk;
    if (!am_finite(e2) || !am_finite(L)) return;
    const float d = e2 - L * L;
    variance = (d < 0.0f ? 0.0f : d) / (float)(k - 1);
}

// A.sp_chunk samples done; mean and variance: NULL, or tight planes of the tile (row j first).
__global__ void __launch_bounds__(256) ort_accum_moments_resolve(PipeArgs A, float* mean, float* variance) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= A.total) return;
    int cx, cy;
    if (!slot_coords(A, k, cx, cy)) return;
    const size_t i = (size_t)cy * (size_t)A.tm.tw + (size_t)cx;
    ort::V3 m = ort::mk(0.0f, 0.0f, 0.0f);
    float v = -1.0f;
    if (tile_row_to_y(A.tm, cy) < A.pp.H) {
        const ort::V3 col = ort::mk(A.fx_col[k], A.fx_col[(size_t)A.total + k], A.fx_col[2 * (size_t)A.total + k]);
        const float m2 = (variance && A.sp_chunk >= 2) ? A.fx_col[3 * (size_t)A.total + k] : 0.0f;
        accum_moments_pixel(col, m2, A.sp_chunk, m, v);
    }
    if (mean) {
        mean[3 * i] = m.x;
        mean[3 * i + 1] = m.y;
        mean[3 * i + 2] = m.z;
    }
    if (variance) variance[i] = v;
}

hipError_t launch_accum_moments_paths(int device, int mode, bool deep, bool lds_scene, size_t lds, long long needed,
                                      const PipeArgs& a, hipStream_t s) {
    const int variant = mode == 2 ? 0 : (deep ? 1 : (lds_scene ? 2 : 3));
    pick<0, 1, 2, 3>(variant, [&](auto V) {
        constexpr int MODE = ORT_V(V) == 0 ? 2 : 0;
        constexpr bool DEEP = ORT_V(V) == 1, LDS = ORT_V(V) == 2;
        const int g = resident_blocks(device, ort_pixel_paths<MODE, DEEP, LDS, 4>, kBlock, lds, needed);
        hipLaunchKernelGGL((ort_pixel_paths<MODE, DEEP, LDS, 4>), dim3(g), dim3(kBlock), lds, s, a);
    });
    return hipGetLastError();
}

// The resolve of an adaptive accumulation (adaptive.inc, after every kernel of this file): a.sample != 0
// says the stored counts are valid; mean, variance and counts: NULL, or tight planes of the tile.
void launch_adaptive_resolve(const PipeArgs& a, size_t slots, float* mean, float* variance, int32_t* counts, hipStream_t s);

int accum_read_moments_impl(ort_ctx* ctx, ort_accum* acc, const ort_accum_moments* m, void* stream) {
    const char* who = "ort_accum_read_moments: ";
    if (!m->mean && !m->variance) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + "mean and variance are both NULL");
    if (m->reserved[0] != 0 || m->reserved[1] != 0 || m->reserved[2] != 0)
        return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + "reserved must be 0");
    if (((uintptr_t)m->mean & 3) || ((uintptr_t)m->variance & 3))
        return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + "mean and variance must be 4-byte aligned");
    if (m->variance && !acc->moments)
        return fail(ctx, ORT_ERR_INVALID_ARG,
                    std::string(who) + "variance needs an accumulation begun with ORT_ACCUM_MOMENTS (ort_accum_begin_ex)");
    if (acc->done < 1) return fail(ctx, ORT_ERR_INVALID_ARG, std::string(who) + "no sample done yet");
    if (acc->scene_gen != ctx->scene.scene_gen || !ctx->scene.has_scene)
        return fail(ctx, ORT_ERR_NO_SCENE,
                    std::string(who) + "the scene changed since the accumulation was begun (ort_accum_restart starts "
                                       "it again on the new scene)");
    const ort_tile* t = &acc->t;
    const size_t pix = (size_t)t->width * (size_t)t->rows;
    if (pix == 0) return ORT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const bool host = m->on_device == 0;
    float* d_mean = m->mean;
    float* d_var = m->variance;
    if (host) {  // tight on the device, copied out
        int rc;
        if ((rc = ensure(ctx, acc->mstage, 16 * pix))) return rc;
        d_mean = m->mean ? (float*)acc->mstage.p : nullptr;
        d_var = m->variance ? (float*)acc->mstage.p + 3 * pix : nullptr;
    }
    const int tilesX = (t->width + 15) / 16, tilesY = (t->rows + 15) / 16;
    const size_t slots = (size_t)acc->blocks * kBlock;
    const DevOutput none = {nullptr, 0, ORT_FORMAT_RGB32F, ORT_PLACE_TILE};
    PipeArgs a = base_args(ctx, &acc->p, t, none, tilesX, tilesY, acc->blocks);  // the passes' slot order
#if ORT_ANALYSIS
    a.wclock = nullptr;
    a.wclock_n = 0;
#endif
    a.fx_col = (float*)((char*)acc->state.p + sizeof(float2) * slots);
    a.sp_chunk = acc->done;
    a.sample = acc->done;
    if (acc->adaptive)  // each pixel at its own count (adaptive.inc)
        launch_adaptive_resolve(a, slots, d_mean, d_var, nullptr, s);
    else
        hipLaunchKernelGGL(ort_accum_moments_resolve, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, a, d_mean, d_var);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_accum_moments_resolve launch");
    if (host) {
        if (m->mean) HIPCHK(ctx, hipMemcpyAsync(m->mean, d_mean, 12 * pix, hipMemcpyDeviceToHost, s));
        if (m->variance) HIPCHK(ctx, hipMemcpyAsync(m->variance, d_var, 4 * pix, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    } else if (!stream) {
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return ORT_OK;
}

}  // namespace

extern "C" {

int ort_accum_begin_ex(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, int32_t flags, ort_accum** out) {
    if (!ctx || !out) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_begin_ex: null argument");
    try {
        return accum_begin_impl(ctx, params, tile, flags, out);
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_accum_begin_ex: ") + ex.what());
    }
}

int ort_accum_read_moments(ort_ctx* ctx, ort_accum* accum, const ort_accum_moments* moments, void* stream) {
    if (!ctx || !accum || !moments) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_read_moments: null argument");
    if (!accum_known(ctx, accum))
        return fail(ctx, ORT_ERR_INVALID_ARG, "ort_accum_read_moments: not an accumulation of this context");
    return accum_read_moments_impl(ctx, accum, moments, stream);
}

#if ORT_ANALYSIS
// TEST-ONLY (ort_internal.h): ort_accum_read_moments after samples_done samples, on the host CPU:
// shade_pixel's chain with its colour sum and m2, then accum_moments_pixel.
int ort_debug_emulate_moments(const float* cr, const float* ma, const float* fr, int32_t n_spheres, const float* node_min,
                              const float* node_max, const int32_t* co, const int32_t* oo, const int32_t* cnt,
                              int32_t n_nodes, const int32_t* idx, int64_t n_indices, int32_t layout, const ort_params* p,
                              const ort_tile* t, int32_t samples_done, float* mean, float* variance) {
    try {
        const std::string bad = check_frame_tile(p, t);
        if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, bad);
        if (samples_done < 1 || samples_done > p->num_samples)
            return fail(nullptr, ORT_ERR_INVALID_ARG, "samples_done must be 1 .. num_samples");
        if (!mean && !variance) return fail(nullptr, ORT_ERR_INVALID_ARG, "mean and variance are both NULL");
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
        for (int row = 0; row < t->rows; ++row) {
            const int y = tile_row_to_y(tm, row);
            for (int c = 0; c < t->width; ++c) {
                const size_t i = (size_t)row * t->width + c;
                ort::V3 m = ort::mk(0.0f, 0.0f, 0.0f);
                float v = -1.0f;
                if (y < p->height) {
                    ort::Counters cc;
                    for (int k = 0; k < 6; ++k) cc.v[k] = 0;
                    ort::V3 col;
                    float m2;
                    if (hs.mode == 0)
                        (void)ort::shade_pixel<0, false>(pp, S, hs.fplanes.data(), hs.fplanes_b.data(), rank_lut, lf, nullptr, nullptr,
                                                         t->x0 + c, y, cc, samples_done, &col, &m2);
                    else if (hs.mode == 1)
                        (void)ort::shade_pixel<1, false>(pp, S, nullptr, nullptr, nullptr, lf, snode.data(), stmin.data(), t->x0 + c,
                                                         y, cc, samples_done, &col, &m2);
                    else
                        (void)ort::shade_pixel<2, false>(pp, S, nullptr, nullptr, nullptr, lf, nullptr, nullptr, t->x0 + c, y, cc,
                                                         samples_done, &col, &m2);
                    accum_moments_pixel(col, m2, samples_done, m, v);
                }
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

// TEST-ONLY (ort_internal.h): finish_pixel(v, 1) per pixel -- the gamma of ORT_DENOISE_GAMMA.
int ort_debug_gamma(const float* rgb, int64_t n_pixels, float* out) {
    if (!rgb || !out || n_pixels < 0) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_gamma: null argument");
    for (int64_t i = 0; i < n_pixels; ++i) {
        const ort::V3 v = ort::finish_pixel(ort::mk(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]), 1);
        out[3 * i] = v.x;
        out[3 * i + 1] = v.y;
        out[3 * i + 2] = v.z;
    }
    return ORT_OK;
}
#endif  // ORT_ANALYSIS

}  // extern "C"
