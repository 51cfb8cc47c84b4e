// Included by ort_kernel.hip after host_launch.inc.  What both render paths (host_pixel_paths.inc,
// host_pipeline.inc) share: the checks of a frame's parameters and output, the frame's shape
// signature, the argument block's common part, the counter sets, the key tables, the output's copy.
namespace {

ort::KCamera to_kcamera(const ort::CameraFrame& f) {
    ort::KCamera k;
    k.origin = ort::mk(f.origin[0], f.origin[1], f.origin[2]);
    k.lowerLeft = ort::mk(f.lowerLeft[0], f.lowerLeft[1], f.lowerLeft[2]);
    k.horizontal = ort::mk(f.horizontal[0], f.horizontal[1], f.horizontal[2]);
    k.vertical = ort::mk(f.vertical[0], f.vertical[1], f.vertical[2]);
    k.u = ort::mk(f.u[0], f.u[1], f.u[2]);
    k.v = ort::mk(f.v[0], f.v[1], f.v[2]);
    k.w = ort::mk(f.w[0], f.w[1], f.w[2]);
    k.lensRadius = f.lensRadius;
    return k;
}

// "" or what is wrong with the frame's size and the tile: what the host emulation checks too (it
// restates the shader, which defines a frame for every sample count).
std::string check_frame_tile(const ort_params* p, const ort_tile* t) {
    if (!p || !t) return "null params or tile";
    if (p->width <= 0 || p->height <= 0) return "width/height must be positive";
    if (t->width < 0 || t->rows < 0) return "negative tile size";
    if (t->x0 < 0 || (int64_t)t->x0 + t->width > p->width) return "tile columns outside the frame";
    if (t->y0 < 0) return "negative y0";
    if (t->band_height > 0 && t->band_stride < t->band_height) return "band_stride < band_height";
    // tile_row_to_y is 32-bit arithmetic: the pixel row of the tile's last row (the largest: rows
    // grow with j) must be an int, or it would wrap negative and pass for a row of the frame
    if (t->rows > 0) {
        const int64_t j = (int64_t)t->rows - 1;
        const int64_t last = t->band_height > 0 ? (int64_t)t->y0 + (j / t->band_height) * (int64_t)t->band_stride + j % t->band_height
                                                : (int64_t)t->y0 + j;
        if (last > 0x7fffffffLL) return "tile rows reach past pixel row 2^31 - 1";
    }
    return "";
}

// ... and with the frame's parameters, for the calls that render on the device (include/ort.h
// ort_params): no samples would leave the output unwritten or finalize stale sums.
std::string check_params(const ort_params* p, const ort_tile* t) {
    const std::string bad = check_frame_tile(p, t);
    if (!bad.empty()) return bad;
    if (p->num_samples < 1) return "num_samples must be at least 1";
    return "";
}

ort::PixelParams pixel_params(const ort_params* p) {
    ort::PixelParams pp;
    const ort::CameraFrame f = ort::cameraFrameFromView(p->view, p->camera_position, p->camera_zoom,
                                                        (float)p->width / (float)p->height);
    pp.cam = to_kcamera(f);
    pp.W = p->width;
    pp.H = p->height;
    pp.ns = p->num_samples;
    pp.maxDepth = p->max_depth;
    return pp;
}

// FNV-1a of the frame shape and scene: the previous-frame hints (list lengths, walk costs)
// belong to one of these
unsigned long long frame_sig(const ort_ctx* ctx, const ort_params* p, const ort_tile* t) {
    const long long v[] = {p->width, p->height, p->num_samples, p->max_depth, t->x0, t->width, t->y0,
                           t->rows, t->band_height, t->band_stride, ctx->scene.n_nodes, ctx->scene.n_spheres,
                           (long long)ctx->scene.n_indices, ctx->opt.xcd_swizzle, ctx->opt.tile_pairs};
    unsigned long long sig = 1469598103934665603ull;
    for (long long x : v) sig = (sig ^ (unsigned long long)x) * 1099511628211ull;
    return sig;
}

// Where the kernels write a frame (ort_output, checked and resolved by render_impl): data on the
// device, the row pitch in bytes.
struct DevOutput {
    void* data;
    long long pitch;
    int format, place;
};
inline int format_bpp(int format) { return format == ORT_FORMAT_RGBA8 ? 4 : 12; }
inline void set_output(PipeArgs& a, const DevOutput& o) {
    a.out = o.data;
    a.out_pitch = (unsigned)o.pitch;
    a.out_format = o.format;
    a.out_place = o.place;
}

// The argument block's part that both render paths fill alike: camera, scene, tile, grid, output.
PipeArgs base_args(const ort_ctx* ctx, const ort_params* p, const ort_tile* t, const DevOutput& o, int tilesX,
                   int tilesY, long long blocks) {
    PipeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.pp = pixel_params(p);
    a.S = device_scene(ctx);
    a.tm = {t->x0, t->width, t->y0, t->rows, t->band_height, t->band_stride};
    a.tilesX = tilesX;
    a.tilesY = tilesY;
    a.total = (int)(blocks * kBlock);
    a.exact_only = ctx->opt.exact_only || !ctx->scene.ordered;
    set_output(a, o);
#if ORT_ANALYSIS
    a.wclock = (ulonglong4*)ctx->wclock;  // ORT_PERSIST_CLOCK / ORT_PIXEL_CLOCK builds (tools/*_clock.py)
    a.wclock_n = (int)ctx->wclock_n;
#endif
    return a;
}

// Two sets of 16 counters (deferred count, persistent cursor, heavy list) in defer_count: a launch
// uses one and its exact kernel (or ort_pixel_paths' last workgroup) zeroes the other for the next
// launch; a memset re-zeroes both after a failed render or a new buffer (sync_ok).  fresh: it did.
int begin_counter_sets(ort_ctx* ctx, hipStream_t s, bool& fresh) {
    fresh = !ctx->pipe.sync_ok;
    if (fresh) {
        HIPCHK(ctx, hipMemsetAsync(ctx->pipe.defer_count.p, 0, 128, s));
        ctx->pipe.sync_set = 0;
        ctx->split.pre_ok = false;  // a failed render may not have listed the next frame's heavy rays
    }
    ctx->pipe.sync_ok = false;  // until this render has enqueued all its launches
    return ORT_OK;
}

// The frame's copy to a host output (the tight scratch frame; row by row where the caller gave a
// pitch), or the wait of a synchronous device-output call.
int finish_output(ort_ctx* ctx, const ort_output* o, const DevOutput& dout, const ort_tile* t, long long host_pitch,
                  void* stream, hipStream_t s) {
    if (!o->is_device) {
        const size_t row_bytes = (size_t)t->width * (size_t)format_bpp(o->format);
        if ((size_t)host_pitch == row_bytes)
            HIPCHK(ctx, hipMemcpyAsync(o->data, dout.data, row_bytes * (size_t)t->rows, hipMemcpyDeviceToHost, s));
        else
            HIPCHK(ctx, hipMemcpy2DAsync(o->data, (size_t)host_pitch, dout.data, row_bytes, row_bytes, (size_t)t->rows,
                                         hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    } else if (!stream) {
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return ORT_OK;
}

// "" or what is wrong with the output description (every case before anything is launched).
std::string check_output(const ort_params* p, const ort_tile* t, const ort_output* o) {
    if (!o) return "null output";
    if (o->format != ORT_FORMAT_RGB32F && o->format != ORT_FORMAT_RGBA8) return "output format: unknown ORT_FORMAT_*";
    if (o->placement != ORT_PLACE_TILE && o->placement != ORT_PLACE_FRAME)
        return "output placement: unknown ORT_PLACE_*";
    if (o->reserved != 0) return "output reserved must be 0";
    if (o->placement == ORT_PLACE_FRAME && !o->is_device)
        return "output placement: ORT_PLACE_FRAME needs device output (is_device)";
    const long long row_bytes =
        (long long)(o->placement == ORT_PLACE_FRAME ? p->width : t->width) * format_bpp(o->format);
    if (o->row_pitch_bytes % 4 != 0) return "output row_pitch_bytes must be a multiple of 4";
    if (o->row_pitch_bytes > 0x7fffffffLL || row_bytes > 0x7fffffffLL)
        return "output row_pitch_bytes: a row of at most 2^31 - 1 bytes";
    if (o->row_pitch_bytes != 0 && o->row_pitch_bytes < row_bytes)
        return "output row_pitch_bytes is below the row's " + std::to_string(row_bytes) + " bytes";
    if (((uintptr_t)o->data & 3) != 0) return "output data must be 4-byte aligned";
    return "";
}

// The scene's origin-code tables (path_key.h), built once per root box (shared by the path sort and
// the queries' sort: scene state, not frame state).
int ensure_key_spread(ort_ctx* ctx) {
    const float box[6] = {ctx->scene.root_lo[0], ctx->scene.root_lo[1], ctx->scene.root_lo[2], ctx->scene.root_hi[0], ctx->scene.root_hi[1], ctx->scene.root_hi[2]};
    if (ctx->pipe.key_spread.p && std::memcmp(box, ctx->pipe.spread_box, sizeof box) == 0) return ORT_OK;
    int rc;
    if ((rc = ensure(ctx, ctx->pipe.key_spread, 4 * (size_t)ort::kSpreadWords))) return rc;
    std::vector<uint32_t> tab((size_t)ort::kSpreadWords);
    // (called, not inlined: the library keeps exporting its copy)
    const ort::MortonPlan plan = ort::mortonPlan(ctx->scene.root_lo, ctx->scene.root_hi);
    uint32_t* const words = tab.data();
    [[clang::noinline]] ort::mortonSpread(plan, words);
    HIPCHK(ctx, hipMemcpy(ctx->pipe.key_spread.p, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice));
    std::memcpy(ctx->pipe.spread_box, box, sizeof box);
    return ORT_OK;
}

}  // namespace
