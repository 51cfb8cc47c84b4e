// reproject.inc -- temporal reprojection (ort_history_*): a preview's history carried across camera
// moves, SVGF's temporal stage (Schied et al. 2017) over ort_trace_camera's pixel-centre rays and hit
// records.  Included by ort_kernel.hip after denoise.inc and every other kernel, whose code is
// unchanged.  It needs no scene and touches no render, accumulation, query or denoise state: its
// records, staging buffers and events are the ort_history's own (host_context.inc).
//   ort_reproject   one lane per pixel; a wave owns 64 consecutive pixels of a row and a 256-thread
//                   block a 256-pixel row segment (ort_denoise_iter's mapping).  A lane reads its
//                   sample, ray and hit record, projects its surface point into the previous frame,
//                   loads the (at most) four previous records of each kind -- aligned 16-byte loads,
//                   for a slow camera near-coherent runs of two previous rows -- blends and stores
//                   the two next records (aligned 16-byte stores) and the outputs.  No LDS, no atomics.
// reproject_pixel is the arithmetic (include/ort.h), shared by the kernel and the host emulation.

namespace {

constexpr int kReprojBlock = 256;
constexpr long long kHistoryMaxPixels = 1ll << 30;

// What an update needs beside the pixel's inputs: the tile, the previous camera frame and tile
// origin (made on the host, once, for the kernel and the emulation alike: reproj_frame).
struct ReprojFrame {
    int W, rows;        // the tile: the history's shape
    int y0, H;          // tile row j is past the frame if y0 + j >= H
    int has_prev;       // there is a previous frame
    int same;           // ... of the same camera, frame size and tile origin, bitwise
    float O[3], LL[3], hor[3], ver[3], w[3];  // the previous camera frame
    float hh, vv;       // dot(hor', hor'), dot(ver', ver')
    float Wp, Hp;       // (float)W', (float)H'
    float x0p, y0p;     // (float)x0', (float)y0'
    float alpha, depth_tol;
    int has_snap;       // motion: there is a snapshot of the spheres at the previous update ...
    int n_sph;          // ... of this many spheres, the resident scene's count
};

// The pixel's inputs and the previous records.
struct ReprojIn {
    const unsigned char* color;  // RGB32F rows, pitch bytes apart
    long long pitch;
    const float* rays;           // 6 floats per pixel
    const int* hits;             // {t bits, sphere} pairs
    const float4* pa;            // previous {r, g, b, n}
    const float4* pb;            // previous {m1, m2, t, sphere}
    const float4* now;           // motion: the resident scene's {centre, radius}, upload order
    const float4* snap;          // motion: the snapshot's
};

struct ReprojPixel {
    float4 a, b;  // the next records
    float var;    // out_variance
};

ORT_FN float rp_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// Pixel (c, j) of an update: the next records and the variance (include/ort.h, steps 1 - 5).
// kMotion (ort_history_update_ex, ORT_HISTORY_MOTION): a hit whose sphere differs bitwise from its
// snapshot -- two aligned 16-byte gathers keyed by the sphere id, coherent wherever a sphere covers
// neighbouring pixels -- is moved back with the sphere before it is projected, and never takes the
// same-camera shortcut.  Without kMotion none of that is compiled.
template <bool kMotion>
ORT_FN ReprojPixel reproject_pixel(const ReprojFrame& K, const ReprojIn& I, int c, int j) {
    ReprojPixel R;
    R.var = -1.0f;
    if (K.y0 + j >= K.H) {  // a row past the frame
        R.a.x = R.a.y = R.a.z = R.a.w = 0.0f;
        R.b.x = R.b.y = R.b.z = 0.0f;
        R.b.w = __builtin_bit_cast(float, (int32_t)-1);
        return R;
    }
    const size_t p = (size_t)j * (size_t)K.W + (size_t)c;
    const float* s = reinterpret_cast<const float*>(I.color + (size_t)j * (size_t)I.pitch) + 3 * (size_t)c;
    const float sr = s[0], sg = s[1], sb = s[2];
    const float l = (0.2126f * sr + 0.7152f * sg) + 0.0722f * sb;
    const float t = __builtin_bit_cast(float, I.hits[2 * p]);
    const int32_t id = I.hits[2 * p + 1];
    const bool ok = dn_finite(sr) && dn_finite(sg) && dn_finite(sb);

    bool have = false;
    float pr = 0.0f, pg = 0.0f, pbl = 0.0f, pm1 = 0.0f, pm2 = 0.0f, pn = 0.0f;
    bool moved = false;
    float4 now = {0.0f, 0.0f, 0.0f, 0.0f}, snap = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (kMotion) {
        if (K.has_prev && K.has_snap && id >= 0 && id < K.n_sph) {
            now = I.now[id];
            snap = I.snap[id];
            moved = __builtin_bit_cast(int32_t, now.x) != __builtin_bit_cast(int32_t, snap.x) ||
                    __builtin_bit_cast(int32_t, now.y) != __builtin_bit_cast(int32_t, snap.y) ||
                    __builtin_bit_cast(int32_t, now.z) != __builtin_bit_cast(int32_t, snap.z) ||
                    __builtin_bit_cast(int32_t, now.w) != __builtin_bit_cast(int32_t, snap.w);
        }
    }
    if (K.has_prev && K.same && !moved) {
        const float4 qa = I.pa[p], qb = I.pb[p];
        if (qa.w > 0.0f && __builtin_bit_cast(int32_t, qb.w) == id) {
            have = true;
            pr = qa.x;
            pg = qa.y;
            pbl = qa.z;
            pn = qa.w;
            pm1 = qb.x;
            pm2 = qb.y;
        }
    } else if (K.has_prev) {
        const float* r = I.rays + 6 * p;
        float ex = r[3], ey = r[4], ez = r[5];
        if (kMotion && moved) {  // the surface point where its sphere was: P' = snap.xyz + s * (P - now.xyz)
            const float sc = snap.w / now.w;
            ex = (snap.x + sc * ((r[0] + t * ex) - now.x)) - K.O[0];
            ey = (snap.y + sc * ((r[1] + t * ey) - now.y)) - K.O[1];
            ez = (snap.z + sc * ((r[2] + t * ez) - now.z)) - K.O[2];
        } else if (id >= 0) {
            ex = (r[0] + t * ex) - K.O[0];
            ey = (r[1] + t * ey) - K.O[1];
            ez = (r[2] + t * ez) - K.O[2];
        }
        const float z = -rp_dot(ex, ey, ez, K.w[0], K.w[1], K.w[2]);
        if (z > 0.0f) {
            const float k = 10.0f / z;
            const float qx = (k * ex + K.O[0]) - K.LL[0], qy = (k * ey + K.O[1]) - K.LL[1], qz = (k * ez + K.O[2]) - K.LL[2];
            const float a = rp_dot(qx, qy, qz, K.hor[0], K.hor[1], K.hor[2]) / K.hh;
            const float b = rp_dot(qx, qy, qz, K.ver[0], K.ver[1], K.ver[2]) / K.vv;
            const float fx = (a * K.Wp - 0.5f) - K.x0p, fy = (b * K.Hp - 0.5f) - K.y0p;
            if (dn_finite(fx) && dn_finite(fy) && fx >= -1.0f && fx < (float)K.W && fy >= -1.0f && fy < (float)K.rows) {
                const float flx = floorf(fx), fly = floorf(fy);
                const float wx = fx - flx, wy = fy - fly;
                const float ux = 1.0f - wx, uy = 1.0f - wy;
                const int ix = (int)flx, iy = (int)fly;
                const bool depth = id >= 0 && K.depth_tol > 0.0f;
                float dist = 0.0f, tol = 0.0f;
                if (depth) {
                    dist = sqrtf(rp_dot(ex, ey, ez, ex, ey, ez));
                    tol = K.depth_tol * dist;
                }
                // the four taps loaded together (a tap outside the tile reads the lane's own record
                // and is dropped below)
                float4 qa4[4], qb4[4];
                bool in4[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int tx = ix + (n & 1), ty = iy + (n >> 1);
                    in4[n] = tx >= 0 && tx < K.W && ty >= 0 && ty < K.rows;
                    const size_t iq = in4[n] ? (size_t)ty * (size_t)K.W + (size_t)tx : p;
                    qa4[n] = I.pa[iq];
                    qb4[n] = I.pb[iq];
                }
                float ws = 0.0f;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const float4 qa = qa4[n], qb = qb4[n];
                    if (!in4[n] || !(qa.w > 0.0f) || __builtin_bit_cast(int32_t, qb.w) != id) continue;
                    if (depth && !(fabsf(qb.z - dist) <= tol)) continue;
                    const float w = ((n & 1) ? wx : ux) * ((n >> 1) ? wy : uy);
                    ws = ws + w;
                    pr = pr + w * qa.x;
                    pg = pg + w * qa.y;
                    pbl = pbl + w * qa.z;
                    pm1 = pm1 + w * qb.x;
                    pm2 = pm2 + w * qb.y;
                    pn = pn + w * qa.w;
                }
                if (ws >= 0.01f) {
                    have = true;
                    pr = pr / ws;
                    pg = pg / ws;
                    pbl = pbl / ws;
                    pm1 = pm1 / ws;
                    pm2 = pm2 / ws;
                    pn = pn / ws;
                }
            }
        }
    }

    R.b.z = t;
    R.b.w = __builtin_bit_cast(float, id);
    if (!have) {
        R.a.x = ok ? sr : 0.0f;
        R.a.y = ok ? sg : 0.0f;
        R.a.z = ok ? sb : 0.0f;
        R.a.w = ok ? 1.0f : 0.0f;
        R.b.x = ok ? l : 0.0f;
        R.b.y = ok ? l * l : 0.0f;
        return R;
    }
    const float n = ok ? pn + 1.0f : pn;
    float a = 1.0f / n;
    if (a < K.alpha) a = K.alpha;
    if (ok) {
        R.a.x = pr + a * (sr - pr);
        R.a.y = pg + a * (sg - pg);
        R.a.z = pbl + a * (sb - pbl);
        R.b.x = pm1 + a * (l - pm1);
        R.b.y = pm2 + a * (l * l - pm2);
    } else {
        R.a.x = pr;
        R.a.y = pg;
        R.a.z = pbl;
        R.b.x = pm1;
        R.b.y = pm2;
    }
    R.a.w = n;
    const float ne = 1.0f / a;
    float v = R.b.y - R.b.x * R.b.x;
    if (v < 0.0f) v = 0.0f;
    const float rv = v / (ne - 1.0f);
    if (ne > 1.0f && dn_finite(rv)) R.var = rv;
    return R;
}

struct ReprojArgs {
    ReprojFrame K;
    ReprojIn I;
    float4* na;        // the next records
    float4* nb;
    float* out_color;  // each null or tight (wave-uniform)
    float* out_var;
    float* out_len;
    int segs;          // 256-pixel segments of a row
};

// Block b: row b / segs, pixels 256 (b % segs) .. of it; a wave's 64 lanes are 64 consecutive pixels.
template <bool kMotion>
__global__ void __launch_bounds__(kReprojBlock) ort_reproject(ReprojArgs A) {
    const int row = (int)(blockIdx.x / (unsigned)A.segs);
    const int x = (int)(blockIdx.x - (unsigned)row * (unsigned)A.segs) * kReprojBlock + (int)threadIdx.x;
    if (x >= A.K.W) return;
    const ReprojPixel R = reproject_pixel<kMotion>(A.K, A.I, x, row);
    const size_t p = (size_t)row * (size_t)A.K.W + (size_t)x;
    A.na[p] = R.a;
    A.nb[p] = R.b;
    if (A.out_color) {
        float* o = A.out_color + 3 * p;
        o[0] = R.a.x;
        o[1] = R.a.y;
        o[2] = R.a.z;
    }
    if (A.out_var) A.out_var[p] = R.var;
    if (A.out_len) A.out_len[p] = R.a.w;
}

// What ort_history_update refuses of a frame for a history of hw x hrows pixels
// (ORT_ERR_INVALID_ARG), the emulation too.  flags_allowed: 0, or ort_history_update_ex's bits.
std::string check_history_frame(int hw, int hrows, const ort_history_frame* f, int32_t flags_allowed = 0) {
    if (!f) return "null frame";
    if (!f->params || !f->tile) return "null params or tile";
    const std::string bad = check_params(f->params, f->tile);  // what ort_render refuses
    if (!bad.empty()) return bad;
    if (f->tile->width != hw || f->tile->rows != hrows) return "the tile's width and rows must be the history's";
    if (f->tile->band_height > 0 && f->tile->band_height < f->tile->rows)
        return "a banded tile's rows are not neighbours in the frame";
    if (!(f->alpha >= 0.0f && f->alpha <= 1.0f)) return "alpha must be 0 .. 1";
    if (!(f->depth_tolerance >= 0.0f)) return "depth_tolerance must be >= 0";
    if ((f->flags & ~flags_allowed) != 0) return "unknown flag bits";
    for (int r : f->reserved)
        if (r != 0) return "reserved must be 0";
    if (((uintptr_t)f->color & 3) || ((uintptr_t)f->rays & 3) || ((uintptr_t)f->hits & 3) || ((uintptr_t)f->out_color & 3) ||
        ((uintptr_t)f->out_variance & 3) || ((uintptr_t)f->out_length & 3))
        return "color, rays, hits and the outputs must be 4-byte aligned";
    const long long row_bytes = 12ll * hw;
    if (f->color_pitch_bytes != 0 &&
        (f->color_pitch_bytes % 4 != 0 || f->color_pitch_bytes < row_bytes || f->color_pitch_bytes > 0x7fffffffLL))
        return "color_pitch_bytes must be 0 or a multiple of 4, at least 12 * width and below 2^31";
    if (row_bytes > 0x7fffffffLL) return "a row of at most 2^31 - 1 bytes";
    if ((long long)hw * hrows > 0 && (!f->color || !f->rays || !f->hits)) return "null color, rays or hits";
    return "";
}

// The same camera, frame size and tile origin, bitwise.
bool reproj_same_camera(const ort_params& a, int ax0, int ay0, const ort_params& b, int bx0, int by0) {
    return a.width == b.width && a.height == b.height && ax0 == bx0 && ay0 == by0 &&
           std::memcmp(a.view, b.view, sizeof a.view) == 0 &&
           std::memcmp(a.camera_position, b.camera_position, sizeof a.camera_position) == 0 &&
           std::memcmp(&a.camera_zoom, &b.camera_zoom, sizeof(float)) == 0;
}

// prev: the previous update's params (NULL: no previous frame) and tile origin.
ReprojFrame reproj_frame(const ort_params* prev, int prev_x0, int prev_y0, const ort_history_frame* f) {
    ReprojFrame K;
    std::memset(&K, 0, sizeof(K));
    K.W = f->tile->width;
    K.rows = f->tile->rows;
    K.y0 = f->tile->y0;
    K.H = f->params->height;
    K.alpha = f->alpha;
    K.depth_tol = f->depth_tolerance;
    if (!prev) return K;
    K.has_prev = 1;
    K.same = reproj_same_camera(*prev, prev_x0, prev_y0, *f->params, f->tile->x0, f->tile->y0);
    const ort::CameraFrame c = ort::cameraFrameFromView(prev->view, prev->camera_position, prev->camera_zoom,
                                                        (float)prev->width / (float)prev->height);
    for (int k = 0; k < 3; ++k) {
        K.O[k] = c.origin[k];
        K.LL[k] = c.lowerLeft[k];
        K.hor[k] = c.horizontal[k];
        K.ver[k] = c.vertical[k];
        K.w[k] = c.w[k];
    }
    K.hh = rp_dot(K.hor[0], K.hor[1], K.hor[2], K.hor[0], K.hor[1], K.hor[2]);
    K.vv = rp_dot(K.ver[0], K.ver[1], K.ver[2], K.ver[0], K.ver[1], K.ver[2]);
    K.Wp = (float)prev->width;
    K.Hp = (float)prev->height;
    K.x0p = (float)prev_x0;
    K.y0p = (float)prev_y0;
    return K;
}

// ... and what ort_history_update_ex refuses beside it.
std::string check_history_frame_ex(int hw, int hrows, const ort_history_frame_ex* f) {
    if (!f) return "null frame";
    const std::string bad = check_history_frame(hw, hrows, &f->base, ORT_HISTORY_MOTION);
    if (!bad.empty()) return bad;
    for (int r : f->reserved)
        if (r != 0) return "reserved must be 0";
    return "";
}

bool history_known(const ort_ctx* ctx, const ort_history* h) {
    return h->ctx == ctx && std::find(ctx->histories.begin(), ctx->histories.end(), h) != ctx->histories.end();
}

// motion: ORT_HISTORY_MOTION (the caller has seen a resident scene).  The snapshot is taken behind
// the kernel on the update's stream, for a history of no pixels too.
int history_update_impl(ort_ctx* ctx, ort_history* h, const ort_history_frame* f, void* stream, bool motion) {
    const size_t W = (size_t)h->width, rows = (size_t)h->rows, n = W * rows;
    const int next = h->cur ^ 1;
    const int n_sph = motion ? ctx->scene.n_spheres : 0;
    const size_t snap_bytes = 16 * (size_t)n_sph;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (n > 0 || snap_bytes > 0) HIPCHK(ctx, hipSetDevice(ctx->device));
    if (snap_bytes > 0)
        if (int rc = ensure(ctx, h->snap, snap_bytes)) return rc;
    bool use_snap = false;
    if (motion) use_snap = h->motion_begin(n_sph);
    else h->forget_motion();
    const auto take_snapshot = [&]() -> int {
        if (!motion) return ORT_OK;
        if (snap_bytes > 0) HIPCHK(ctx, hipMemcpyAsync(h->snap.p, ctx->scene.sph_cr.p, snap_bytes, hipMemcpyDeviceToDevice, s));
        h->has_snap = true;
        h->snap_n = n_sph;
        return ORT_OK;
    };
    if (n > 0) {
        const bool host = f->on_device == 0;
        const size_t in_row = 12 * W;
        const size_t in_pitch = f->color_pitch_bytes ? (size_t)f->color_pitch_bytes : in_row;
        int rc;
        if (host && ((rc = ensure(ctx, h->in_color, 12 * n)) || (rc = ensure(ctx, h->in_rays, 24 * n)) ||
                     (rc = ensure(ctx, h->in_hits, 8 * n)) || (f->out_color && (rc = ensure(ctx, h->out_color, 12 * n))) ||
                     (f->out_variance && (rc = ensure(ctx, h->out_var, 4 * n))) ||
                     (f->out_length && (rc = ensure(ctx, h->out_len, 4 * n)))))
            return rc;
        if (host) {  // the inputs, tight on the device
            HIPCHK(ctx, hipMemcpy2DAsync(h->in_color.p, in_row, f->color, in_pitch, in_row, rows, hipMemcpyHostToDevice, s));
            HIPCHK(ctx, hipMemcpyAsync(h->in_rays.p, f->rays, 24 * n, hipMemcpyHostToDevice, s));
            HIPCHK(ctx, hipMemcpyAsync(h->in_hits.p, f->hits, 8 * n, hipMemcpyHostToDevice, s));
        }
        ReprojArgs a;
        std::memset(&a, 0, sizeof(a));
        a.K = reproj_frame(h->has_prev ? &h->prev_p : nullptr, h->prev_x0, h->prev_y0, f);
        a.I.color = host ? (const unsigned char*)h->in_color.p : (const unsigned char*)f->color;
        a.I.pitch = host ? (long long)in_row : (long long)in_pitch;
        a.I.rays = host ? (const float*)h->in_rays.p : (const float*)f->rays;
        a.I.hits = host ? (const int*)h->in_hits.p : (const int*)f->hits;
        a.I.pa = (const float4*)h->rec[h->cur][0].p;
        a.I.pb = (const float4*)h->rec[h->cur][1].p;
        a.K.has_snap = use_snap ? 1 : 0;
        a.K.n_sph = n_sph;
        a.I.now = (const float4*)ctx->scene.sph_cr.p;
        a.I.snap = (const float4*)h->snap.p;
        a.na = (float4*)h->rec[next][0].p;
        a.nb = (float4*)h->rec[next][1].p;
        a.out_color = host ? (f->out_color ? (float*)h->out_color.p : nullptr) : f->out_color;
        a.out_var = host ? (f->out_variance ? (float*)h->out_var.p : nullptr) : f->out_variance;
        a.out_len = host ? (f->out_length ? (float*)h->out_len.p : nullptr) : f->out_length;
        a.segs = (int)((W + kReprojBlock - 1) / kReprojBlock);
        const long long blocks = (long long)a.segs * (long long)rows;  // at most 2^30: a 1-D grid
        HIPCHK(ctx, h->ev.begin(s));
        if (motion) hipLaunchKernelGGL(ort_reproject<true>, dim3((unsigned)blocks), dim3(kReprojBlock), 0, s, a);
        else hipLaunchKernelGGL(ort_reproject<false>, dim3((unsigned)blocks), dim3(kReprojBlock), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(ctx, e, "ort_reproject launch");
        HIPCHK(ctx, h->ev.end(s));
        if (int rc = take_snapshot()) return rc;
        if (host) {
            if (f->out_color) HIPCHK(ctx, hipMemcpyAsync(f->out_color, h->out_color.p, 12 * n, hipMemcpyDeviceToHost, s));
            if (f->out_variance) HIPCHK(ctx, hipMemcpyAsync(f->out_variance, h->out_var.p, 4 * n, hipMemcpyDeviceToHost, s));
            if (f->out_length) HIPCHK(ctx, hipMemcpyAsync(f->out_length, h->out_len.p, 4 * n, hipMemcpyDeviceToHost, s));
        }
        // (the records are the history's: the next update is enqueued behind this one by the caller's order)
        h->cur = next;
        h->prev_p = *f->params;
        h->prev_x0 = f->tile->x0;
        h->prev_y0 = f->tile->y0;
        h->updated();
        if (host || !stream) HIPCHK(ctx, hipStreamSynchronize(s));
        return ORT_OK;
    }
    if (int rc = take_snapshot()) return rc;
    h->prev_p = *f->params;
    h->prev_x0 = f->tile->x0;
    h->prev_y0 = f->tile->y0;
    h->updated();
    if (motion && snap_bytes > 0 && !stream) HIPCHK(ctx, hipStreamSynchronize(s));
    return ORT_OK;
}

}  // namespace

extern "C" {

int ort_history_begin(ort_ctx* ctx, int32_t width, int32_t rows, ort_history** out) {
    if (!ctx || !out) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_begin: null argument");
    *out = nullptr;
    try {
        if (width < 0 || rows < 0) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_begin: negative size");
        const long long n = (long long)width * (long long)rows;
        if (n > kHistoryMaxPixels) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_begin: a history of at most 2^30 pixels");
        HIPCHK(ctx, hipSetDevice(ctx->device));
        ort_history* h = new (std::nothrow) ort_history();
        if (!h) return fail(ctx, ORT_ERR_OUT_OF_MEMORY, "ort_history_begin: out of host memory");
        h->ctx = ctx;
        h->width = width;
        h->rows = rows;
        int rc = ORT_OK;
        for (auto& set : h->rec)
            for (DevBuf& b : set)
                if (!rc && n > 0) rc = ensure(ctx, b, 16 * (size_t)n);
        hipError_t e = hipSuccess;
        if (rc || (e = h->ev.create()) != hipSuccess) {
            if (!rc) rc = hip_fail(ctx, e, "ort_history_begin: events");
            free_history(h);
            return rc;
        }
        ctx->histories.push_back(h);
        *out = h;
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_history_begin: ") + ex.what());
    }
}

int ort_history_update(ort_ctx* ctx, ort_history* history, const ort_history_frame* f, void* stream) {
    if (!ctx || !history || !f) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_update: null argument");
    try {
        if (!history_known(ctx, history)) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_update: not a history of this context");
        const std::string bad = check_history_frame(history->width, history->rows, f);
        if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_update: " + bad);
        return history_update_impl(ctx, history, f, stream, false);
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_history_update: ") + ex.what());
    }
}

int ort_history_update_ex(ort_ctx* ctx, ort_history* history, const ort_history_frame_ex* f, void* stream) {
    if (!ctx || !history || !f) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_update_ex: null argument");
    try {
        if (!history_known(ctx, history))
            return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_update_ex: not a history of this context");
        const std::string bad = check_history_frame_ex(history->width, history->rows, f);
        if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_update_ex: " + bad);
        const bool motion = (f->base.flags & ORT_HISTORY_MOTION) != 0;
        if (motion && !ctx->scene.has_scene)
            return fail(ctx, ORT_ERR_NO_SCENE, "ort_history_update_ex: ORT_HISTORY_MOTION needs a resident scene");
        ort_history_frame base = f->base;
        base.flags = 0;
        return history_update_impl(ctx, history, &base, stream, motion);
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_history_update_ex: ") + ex.what());
    }
}

int ort_history_reset(ort_ctx* ctx, ort_history* history) {
    if (!ctx || !history) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_reset: null argument");
    if (!history_known(ctx, history)) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_reset: not a history of this context");
    history->reset();
    return ORT_OK;
}

int ort_history_get_info(const ort_history* history, ort_history_info* info) {
    if (!history || !info) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_history_get_info: null argument");
    info->width = history->width;
    info->rows = history->rows;
    info->updates = history->updates;
    long long bytes = 0;
    each_history_buffer(const_cast<ort_history*>(history), [&](DevBuf& b) { bytes += (long long)b.bytes; });
    info->device_bytes = bytes;
    return ORT_OK;
}

int ort_history_last_update_ms(ort_ctx* ctx, ort_history* history, float* ms) {
    if (!ctx || !history || !ms) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_last_update_ms: null argument");
    if (!history_known(ctx, history))
        return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_last_update_ms: not a history of this context");
    if (!history->ev.timed) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_last_update_ms: no update launched yet");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, history->ev.elapsed(ms));
    return ORT_OK;
}

int ort_history_free(ort_ctx* ctx, ort_history* history) {
    if (!history) return ORT_OK;
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_history_free: null ctx");
    const auto it = std::find(ctx->histories.begin(), ctx->histories.end(), history);
    if (it == ctx->histories.end()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_history_free: not a history of this context");
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ctx->histories.erase(it);
    free_history(history);
    return ORT_OK;
}

}  // extern "C"

#if ORT_ANALYSIS
namespace {

// One update on the CPU, one pixel after another through reproject_pixel<kMotion>.  The record planes
// and the sphere arrays are copied into aligned arrays (and the planes back).  f has been checked.
template <bool kMotion>
int debug_history_update(const ort_params* prev_params, int32_t prev_x0, int32_t prev_y0, const float* prev_a,
                         const float* prev_b, const ort_history_frame* f, const float* now, const float* snap, int32_t n_sph,
                         float* next_a, float* next_b) {
    try {
        if (f->on_device) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_update: host pointers only");
        const size_t W = (size_t)f->tile->width, rows = (size_t)f->tile->rows, n = W * rows;
        if ((long long)n > kHistoryMaxPixels) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_update: at most 2^30 pixels");
        if (n == 0) return ORT_OK;
        if (!next_a || !next_b || (prev_params && (!prev_a || !prev_b)))
            return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_update: null record planes");
        std::vector<float4> pa(prev_params ? n : 0), pb(prev_params ? n : 0), na(n), nb(n);
        std::vector<float> var(n);
        if (prev_params) {
            std::memcpy(pa.data(), prev_a, 16 * n);
            std::memcpy(pb.data(), prev_b, 16 * n);
        }
        ReprojFrame K = reproj_frame(prev_params, prev_x0, prev_y0, f);
        ReprojIn I;
        std::vector<float4> vnow, vsnap;
        I.now = I.snap = nullptr;
        if (kMotion) {
            vnow.resize((size_t)n_sph);
            if (n_sph > 0) std::memcpy(vnow.data(), now, 16 * (size_t)n_sph);
            if (snap) {
                vsnap.resize((size_t)n_sph);
                if (n_sph > 0) std::memcpy(vsnap.data(), snap, 16 * (size_t)n_sph);
            }
            K.has_snap = snap ? 1 : 0;
            K.n_sph = n_sph;
            I.now = vnow.data();
            I.snap = vsnap.data();
        }
        I.color = reinterpret_cast<const unsigned char*>(f->color);
        I.pitch = f->color_pitch_bytes ? (long long)f->color_pitch_bytes : 12ll * (long long)W;
        I.rays = reinterpret_cast<const float*>(f->rays);
        I.hits = reinterpret_cast<const int*>(f->hits);
        I.pa = pa.data();
        I.pb = pb.data();
        for (size_t j = 0; j < rows; ++j)
            for (size_t c = 0; c < W; ++c) {
                const ReprojPixel R = reproject_pixel<kMotion>(K, I, (int)c, (int)j);
                const size_t p = j * W + c;
                na[p] = R.a;
                nb[p] = R.b;
                var[p] = R.var;
            }
        for (size_t p = 0; p < n; ++p) {
            if (f->out_color) {
                f->out_color[3 * p] = na[p].x;
                f->out_color[3 * p + 1] = na[p].y;
                f->out_color[3 * p + 2] = na[p].z;
            }
            if (f->out_variance) f->out_variance[p] = var[p];
            if (f->out_length) f->out_length[p] = na[p].w;
        }
        std::memcpy(next_a, na.data(), 16 * n);
        std::memcpy(next_b, nb.data(), 16 * n);
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

}  // namespace

extern "C" {

// TEST-ONLY host emulations (ort_internal.h).
int ort_debug_history_update(const ort_params* prev_params, int32_t prev_x0, int32_t prev_y0, const float* prev_a,
                             const float* prev_b, const ort_history_frame* f, float* next_a, float* next_b) {
    if (!f || !f->tile) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_update: null frame or tile");
    const std::string bad = check_history_frame(f->tile->width, f->tile->rows, f);
    if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_update: " + bad);
    return debug_history_update<false>(prev_params, prev_x0, prev_y0, prev_a, prev_b, f, nullptr, nullptr, 0, next_a, next_b);
}

int ort_debug_history_update_ex(const ort_params* prev_params, int32_t prev_x0, int32_t prev_y0, const float* prev_a,
                                const float* prev_b, const ort_history_frame_ex* f, const float* now, const float* snap,
                                int32_t n_spheres, float* next_a, float* next_b) {
    if (!f || !f->base.tile) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_update_ex: null frame or tile");
    const std::string bad = check_history_frame_ex(f->base.tile->width, f->base.tile->rows, f);
    if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_update_ex: " + bad);
    ort_history_frame base = f->base;
    base.flags = 0;
    if (!(f->base.flags & ORT_HISTORY_MOTION))
        return debug_history_update<false>(prev_params, prev_x0, prev_y0, prev_a, prev_b, &base, nullptr, nullptr, 0, next_a, next_b);
    if (!now) return fail(nullptr, ORT_ERR_NO_SCENE, "ort_debug_history_update_ex: ORT_HISTORY_MOTION needs the scene's spheres");
    if (n_spheres < 0) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_update_ex: negative sphere count");
    return debug_history_update<true>(prev_params, prev_x0, prev_y0, prev_a, prev_b, &base, now, snap, n_spheres, next_a, next_b);
}

int ort_debug_history_state(int64_t* st, int32_t op, int32_t n_spheres, int32_t* reads_snapshot) {
    if (!st || op < 0 || op > 3) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_history_state: null state or unknown op");
    HistoryState h;
    h.updates = st[0];
    h.has_prev = st[1] != 0;
    h.stale = st[2] != 0;
    h.stale_updates = st[3];
    h.has_snap = st[4] != 0;
    h.snap_n = (int)st[5];
    bool reads = false;
    if (op == 0) h.scene_replaced();
    else if (op == 1) h.reset();
    else {
        if (op == 2) h.forget_motion();
        else reads = h.motion_begin(n_spheres);
        h.updated();
        h.has_snap = op == 3;
        h.snap_n = op == 3 ? n_spheres : h.snap_n;
    }
    if (reads_snapshot) *reads_snapshot = reads ? 1 : 0;
    st[0] = h.updates;
    st[1] = h.has_prev;
    st[2] = h.stale;
    st[3] = h.stale_updates;
    st[4] = h.has_snap;
    st[5] = h.snap_n;
    return ORT_OK;
}

}  // extern "C"
#endif  // ORT_ANALYSIS
