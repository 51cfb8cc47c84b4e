// denoise.inc -- the guided denoiser (ort_denoise): an edge-avoiding a-trous wavelet filter (Dammertz
// et al. 2010) over a caller's RGB32F image, guided by ort_trace_camera's hit records and normals.
// Included last by ort_kernel.hip (its kernels follow every other kernel in the code object, whose
// code is unchanged).  It needs no scene and touches no render, accumulation or query state: its
// buffers and events are ort_ctx::denoise.
//   ort_denoise_pack        reads the caller's colour, hits and normals once and writes two 16-byte
//                           records per pixel: {r, g, b, sphere id} and {normal, t}.  The id rides in
//                           the colour record's fourth word, which the taps load anyway: a miss is
//                           recognised from that record (id < 0) and ORT_DENOISE_SAME_SPHERE needs
//                           no plane of its own.  Every later load is an aligned 16-byte load.
//   ort_denoise_iter<FMT>   one iteration: a wave owns 64 consecutive pixels of a row, so every tap
//                           row is one coalesced run of records whatever the step; each lane loads
//                           its 25 taps from global memory, a tap row's five together.  FMT 0
//                           writes the next colour records
//                           (the two internal buffers ping-pong), 1 and 2 the caller's RGB32F and
//                           RGBA8 (the last iteration).
//   ort_denoise_pack_var    ort_denoise_ex with a variance: the caller's variance plane through the
//                           3 x 3 binomial prefilter into the first of two float planes
//   ort_denoise_iter_ex<FMT, VAR>  an iteration with the variance-guided term (VAR: the variances read
//                           per tap from their own plane -- 4 bytes beside a 16-byte record, one
//                           coalesced run per tap row like the records -- and the next ones written
//                           to the other plane) and, on the last iteration, the optional gamma.
//                           Named after ort_denoise_iter's instances, which keep their code;
//                           ort_denoise_ex without variance and gamma launches those alone.
// denoise_pixel<VAR> is the arithmetic (include/ort.h), shared by the kernel and the host emulation.
// A second form of the iteration kernel, a rolling window of the five tap rows in LDS, was built,
// passed the same tests and lost: 1.45 times the direct form's time at 3840 x 2160, 5 iterations
// (DESIGN.md 4.14, profiles/denoise/ab.md).  It is not in the tree.

namespace {

constexpr int kDenoiseBlock = 256;
constexpr long long kDenoiseMaxPixels = 1ll << 30;

// What an iteration needs beside the records: the image, the step and the terms' constants (made
// on the host, once, for the kernel and the emulation alike: denoise_iter).
struct DenoiseIter {
    int W, H;
    int s;                 // 2^i
    int npow;              // normal_power
    int same;              // ORT_DENOISE_SAME_SPHERE
    int use_color, use_depth;
    float inv_c, inv_z;
};

DenoiseIter denoise_iter(const ort_denoise_desc* d, int i) {
    DenoiseIter K;
    std::memset(&K, 0, sizeof(K));
    K.W = d->width;
    K.H = d->rows;
    K.s = 1 << i;
    K.npow = d->normal_power;
    K.same = (d->flags & ORT_DENOISE_SAME_SPHERE) != 0;
    K.use_color = d->sigma_color > 0.0f;
    K.use_depth = d->sigma_depth > 0.0f;
    if (K.use_color) {
        const float sc = d->sigma_color * (1.0f / (float)K.s);  // 2^-i exactly
        K.inv_c = 1.0f / (sc * sc);
    }
    if (K.use_depth) K.inv_z = 1.0f / (d->sigma_depth * (float)K.s);
    return K;
}

ORT_FN float dn_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

ORT_FN bool dn_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

ORT_FN bool dn_finite3(const float4& c) { return dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z); }

ORT_FN float dn_h(int k) { return k == 2 ? 0.375f : ((k == 1 || k == 3) ? 0.25f : 0.0625f); }

// The colour record {r, g, b, sphere id} and the guide record {normal, t} of a pixel.
ORT_FN float4 dn_color_record(float r, float g, float b, int32_t sphere) {
    float4 c;
    c.x = r;
    c.y = g;
    c.z = b;
    c.w = __builtin_bit_cast(float, sphere);
    return c;
}

// valid(x) of the variance term: finite and >= 0.
ORT_FN bool dn_valid(float v) { return dn_finite(v) && v >= 0.0f; }

ORT_FN float dn_lum(const float4& c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// Pixel (x, y) of one iteration: the next colour record (the id carried on).  cur and guide hold
// K.W * K.H records, row-major.  VAR (ort_denoise_ex with a variance): var holds the previous
// iteration's variances, sv2 is sigma_variance squared and next_var receives the pixel's next one.
template <bool VAR>
ORT_FN float4 denoise_pixel(const DenoiseIter& K, const float4* cur, const float4* guide, int x, int y,
                            const float* var = nullptr, float sv2 = 0.0f, float* next_var = nullptr) {
    const size_t ip = (size_t)y * (size_t)K.W + (size_t)x;
    const float4 cp = cur[ip];
    float vp = 0.0f, inv_v = 0.0f, lp = 0.0f, sv = 0.0f;
    bool vok = false;
    if (VAR) {
        vp = var[ip];
        *next_var = vp;  // a pixel copied through, or without an estimate, keeps it
        vok = dn_valid(vp);
    }
    if (!dn_finite3(cp)) return cp;  // copied through
    if (VAR && vok) {
        inv_v = 1.0f / (sv2 * vp + 1e-12f);
        lp = dn_lum(cp);
    }
    const int32_t idp = __builtin_bit_cast(int32_t, cp.w);
    const bool hp = idp >= 0;
    const float4 gp = guide[ip];
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * K.s;
        if (qy < 0 || qy >= K.H) continue;
        const float hy = dn_h(dy + 2);
        const size_t row = (size_t)qy * (size_t)K.W;
        // the row's five taps loaded together (a tap outside the image reads the lane's own column
        // and is dropped below), the guide records where p is a hit
        float4 cq5[5], gq5[5];
        float vq5[5];
        bool in5[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int qx = x + (k - 2) * K.s;
            in5[k] = qx >= 0 && qx < K.W;
            const size_t iq = row + (size_t)(in5[k] ? qx : x);
            cq5[k] = cur[iq];
            if (hp) gq5[k] = guide[iq];
            if (VAR && vok) vq5[k] = var[iq];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (!in5[k]) continue;
            const float4 cq = cq5[k];
            const int32_t idq = __builtin_bit_cast(int32_t, cq.w);
            const bool hq = idq >= 0;
            // the taps that add nothing: w = 0, and a non-finite cur_q is never multiplied
            if (hp != hq || (K.same && idp != idq) || !dn_finite3(cq)) continue;
            float w = hy * dn_h(k);
            if (hp) {  // (and hq)
                const float4 gq = gq5[k];
                float a = dn_clamp01((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
                for (int e = 0; e < K.npow; ++e) a = a * a;
                w = w * a;
                if (K.use_depth) w = w * dn_clamp01(1.0f - fabsf(gp.w - gq.w) * K.inv_z);
            }
            if (K.use_color) {
                const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
                const float dc = (dr * dr + dg * dg) + db * db;
                const float wc = dn_clamp01(1.0f - dc * K.inv_c);
                w = w * (wc * wc);
            }
            if (VAR && vok) {
                const float dl = lp - dn_lum(cq);
                w = w * dn_clamp01(1.0f - (dl * dl) * inv_v);
                const float vq = vq5[k];
                sv = sv + (w * w) * (dn_valid(vq) ? vq : 0.0f);
            }
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
        }
    }
    float4 o;
    o.x = sr / sw;
    o.y = sg / sw;
    o.z = sb / sw;
    o.w = cp.w;
    if (VAR && vok) *next_var = sv / (sw * sw);
    return o;
}

struct DenoisePackArgs {
    const unsigned char* color;  // RGB32F rows, pitch bytes apart
    long long pitch;
    const int* hits;             // {t bits, sphere} pairs (4-byte aligned: read as two words)
    const float* normals;
    float4* col;
    float4* guide;
    int W;
    long long n;                 // pixels
};

__global__ void __launch_bounds__(kDenoiseBlock) ort_denoise_pack(DenoisePackArgs A) {
    const long long i = (long long)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (i >= A.n) return;
    const long long row = i / A.W;
    const int x = (int)(i - row * A.W);
    const float* c = reinterpret_cast<const float*>(A.color + (size_t)row * (size_t)A.pitch) + 3 * (size_t)x;
    const int h_t = A.hits[2 * (size_t)i], h_sphere = A.hits[2 * (size_t)i + 1];
    const float* nrm = A.normals + 3 * (size_t)i;
    A.col[i] = dn_color_record(c[0], c[1], c[2], h_sphere);
    float4 g;
    g.x = nrm[0];
    g.y = nrm[1];
    g.z = nrm[2];
    g.w = __int_as_float(h_t);
    A.guide[i] = g;
}

struct DenoiseIterArgs {
    DenoiseIter K;
    const float4* cur;
    const float4* guide;
    void* out;            // FMT 0: the next colour records; 1, 2: the caller's rows
    long long out_pitch;  // FMT 1, 2
    int segs;             // 256-pixel segments of a row
};

template <int FMT>
__device__ __forceinline__ void denoise_write(const DenoiseIterArgs& A, int x, int row, const float4& o) {
    if (FMT == 0) {
        static_cast<float4*>(A.out)[(size_t)row * (size_t)A.K.W + (size_t)x] = o;
    } else if (FMT == 1) {
        float* p = reinterpret_cast<float*>(static_cast<unsigned char*>(A.out) + (size_t)row * (size_t)A.out_pitch) + 3 * (size_t)x;
        p[0] = o.x;
        p[1] = o.y;
        p[2] = o.z;
    } else {
        uint32_t* p = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(A.out) + (size_t)row * (size_t)A.out_pitch) + (size_t)x;
        *p = ort::pack_rgba8(ort::mk(o.x, o.y, o.z));
    }
}

// Block b: row b / segs, pixels 256 (b % segs) .. of it; a wave's 64 lanes are 64 consecutive pixels.
template <int FMT>
__global__ void __launch_bounds__(kDenoiseBlock) ort_denoise_iter(DenoiseIterArgs A) {
    const int row = (int)(blockIdx.x / (unsigned)A.segs);
    const int x = (int)(blockIdx.x - (unsigned)row * (unsigned)A.segs) * kDenoiseBlock + (int)threadIdx.x;
    if (x >= A.K.W) return;
    const float4 o = denoise_pixel<false>(A.K, A.cur, A.guide, x, row);
    denoise_write<FMT>(A, x, row, o);
}

// ort_denoise_ex's pack pass beside ort_denoise_pack: the variance plane through the 3 x 3 binomial
// prefilter (include/ort.h), shared with the emulation.  v holds W * H floats.
ORT_FN float denoise_prefilter(const float* v, int W, int H, int x, int y) {
    const float vp = v[(size_t)y * (size_t)W + (size_t)x];
    if (!dn_valid(vp)) return vp;
    float ws = 0.0f, vs = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const float vq = v[(size_t)qy * (size_t)W + (size_t)qx];
            if (!dn_valid(vq)) continue;
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            ws = ws + k;
            vs = vs + k * vq;
        }
    }
    return vs / ws;
}

__global__ void __launch_bounds__(kDenoiseBlock) ort_denoise_pack_var(const float* v, float* out, int W, int H) {
    const long long i = (long long)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (i >= (long long)W * H) return;
    const int y = (int)(i / W);
    out[i] = denoise_prefilter(v, W, H, (int)(i - (long long)y * W), y);
}

// An iteration of ort_denoise_ex: ort_denoise_iter with the variance term (VAR: the variances are a
// float plane of their own beside the colour records, read per tap and ping-ponged like them) and,
// on the last iteration, the optional gamma.
struct DenoiseIterExArgs {
    DenoiseIterArgs base;
    const float* var;     // VAR: the previous iteration's variances (the prefiltered input for i = 0)
    float* next_var;      // VAR, FMT 0: the next ones
    float sv2;            // sigma_variance squared
    int gamma;            // FMT 1, 2: ORT_DENOISE_GAMMA
};

template <int FMT, bool VAR>
__global__ void __launch_bounds__(kDenoiseBlock) ort_denoise_iter_ex(DenoiseIterExArgs A) {
    const int row = (int)(blockIdx.x / (unsigned)A.base.segs);
    const int x = (int)(blockIdx.x - (unsigned)row * (unsigned)A.base.segs) * kDenoiseBlock + (int)threadIdx.x;
    if (x >= A.base.K.W) return;
    float nv = 0.0f;
    float4 o = denoise_pixel<VAR>(A.base.K, A.base.cur, A.base.guide, x, row, A.var, A.sv2, &nv);
    if (VAR && FMT == 0) A.next_var[(size_t)row * (size_t)A.base.K.W + (size_t)x] = nv;
    if (FMT != 0 && A.gamma) {
        const ort::V3 g = ort::finish_pixel(ort::mk(o.x, o.y, o.z), 1);
        o.x = g.x;
        o.y = g.y;
        o.z = g.z;
    }
    denoise_write<FMT>(A.base, x, row, o);
}

// What ort_denoise refuses (ORT_ERR_INVALID_ARG), the emulation too; flags: the bits the call knows.
std::string check_denoise(const ort_denoise_desc* d, const ort_output* o, int flags = ORT_DENOISE_SAME_SPHERE) {
    if (!d || !o) return "null description or output";
    if (d->width < 0 || d->rows < 0) return "negative image size";
    const long long n = (long long)d->width * (long long)d->rows;
    if (n > kDenoiseMaxPixels) return "an image of at most 2^30 pixels";
    if (d->iterations < 1 || d->iterations > 6) return "iterations must be 1 .. 6";
    if (d->normal_power < 0 || d->normal_power > 7) return "normal_power must be 0 .. 7";
    if (!(d->sigma_color >= 0.0f) || !(d->sigma_depth >= 0.0f)) return "sigma_color and sigma_depth must be >= 0";
    if (d->flags & ~flags) return "unknown flag bits";
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return "reserved must be 0";
    if (((uintptr_t)d->color & 3) || ((uintptr_t)d->hits & 3) || ((uintptr_t)d->normals & 3))
        return "color, hits and normals must be 4-byte aligned";
    const long long row_bytes = 12ll * d->width;
    if (d->color_pitch_bytes != 0 &&
        (d->color_pitch_bytes % 4 != 0 || d->color_pitch_bytes < row_bytes || d->color_pitch_bytes > 0x7fffffffLL))
        return "color_pitch_bytes must be 0 or a multiple of 4, at least 12 * width and below 2^31";
    if (row_bytes > 0x7fffffffLL) return "a row of at most 2^31 - 1 bytes";
    if (o->placement == ORT_PLACE_FRAME) return "output placement: ORT_PLACE_TILE only (the tile is the image)";
    // what ort_render_ex refuses of an output, for a tile of this width
    ort_params p;
    ort_tile t;
    std::memset(&p, 0, sizeof(p));
    std::memset(&t, 0, sizeof(t));
    p.width = t.width = d->width;
    const std::string bad = check_output(&p, &t, o);
    if (!bad.empty()) return bad;
    if ((d->on_device != 0) != (o->is_device != 0)) return "on_device and output->is_device must agree";
    if (n > 0 && (!d->color || !d->hits || !d->normals || !o->data)) return "null color, hits, normals or output data";
    return "";
}

hipError_t launch_denoise_iter(int fmt, long long blocks, hipStream_t s, const DenoiseIterArgs& a) {
    pick<0, 1, 2>(fmt, [&](auto FMT) {
        hipLaunchKernelGGL((ort_denoise_iter<ORT_V(FMT)>), dim3((unsigned)blocks), dim3(kDenoiseBlock), 0, s, a);
    });
    return hipGetLastError();
}

// What ort_denoise_ex refuses beyond check_denoise.
std::string check_denoise_ex(const ort_denoise_desc_ex* x, const ort_output* o) {
    if (!x) return "null description or output";
    const std::string bad = check_denoise(&x->base, o, ORT_DENOISE_SAME_SPHERE | ORT_DENOISE_GAMMA);
    if (!bad.empty()) return bad;
    if (x->reserved[0] != 0 || x->reserved[1] != 0 || x->reserved[2] != 0) return "reserved must be 0";
    if ((uintptr_t)x->variance & 3) return "variance must be 4-byte aligned";
    if (x->variance && !(x->sigma_variance > 0.0f)) return "sigma_variance must be > 0 with a variance";
    if (!x->variance && !(x->sigma_variance == 0.0f)) return "sigma_variance must be 0 without a variance";
    return "";
}

hipError_t launch_denoise_iter_ex(int fmt, bool var, long long blocks, hipStream_t s, const DenoiseIterExArgs& a) {
    pick<0, 1, 2, 3, 4>(var ? fmt : 2 + fmt, [&](auto V) {  // (without the variance: the last iteration only)
        constexpr int FMT = ORT_V(V) < 3 ? ORT_V(V) : ORT_V(V) - 2;
        hipLaunchKernelGGL((ort_denoise_iter_ex<FMT, (ORT_V(V) < 3)>), dim3((unsigned)blocks), dim3(kDenoiseBlock), 0, s, a);
    });
    return hipGetLastError();
}

// ort_denoise (variance NULL, gamma false: its launches and nothing else) and ort_denoise_ex.
int denoise_impl(ort_ctx* ctx, const ort_denoise_desc* d, const float* variance, float sigma_variance, bool gamma,
                 const ort_output* o, void* stream) {
    const size_t n = (size_t)d->width * (size_t)d->rows;
    if (n == 0) return ORT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DenoiseState& ds = ctx->denoise;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const bool host = d->on_device == 0;
    const size_t W = (size_t)d->width, rows = (size_t)d->rows;
    const size_t in_row = 12 * W, out_row = (size_t)format_bpp(o->format) * W;
    const size_t in_pitch = d->color_pitch_bytes ? (size_t)d->color_pitch_bytes : in_row;
    const size_t out_pitch = o->row_pitch_bytes ? (size_t)o->row_pitch_bytes : out_row;
    int rc;
    if ((rc = ensure(ctx, ds.guide, 16 * n)) || (rc = ensure(ctx, ds.col_a, 16 * n)) ||
        (d->iterations > 1 && (rc = ensure(ctx, ds.col_b, 16 * n))))
        return rc;
    if (host && ((rc = ensure(ctx, ds.in_color, 12 * n)) || (rc = ensure(ctx, ds.in_hits, 8 * n)) ||
                 (rc = ensure(ctx, ds.in_normals, 12 * n)) || (rc = ensure(ctx, ds.out, out_row * rows))))
        return rc;
    if (variance && ((rc = ensure(ctx, ds.var_a, 4 * n)) || (d->iterations > 1 && (rc = ensure(ctx, ds.var_b, 4 * n))) ||
                     (host && (rc = ensure(ctx, ds.in_var, 4 * n)))))
        return rc;
    HIPCHK(ctx, ds.ev.create());
    if (host) {  // the inputs, tight on the device
        HIPCHK(ctx, hipMemcpy2DAsync(ds.in_color.p, in_row, d->color, in_pitch, in_row, rows, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(ds.in_hits.p, d->hits, 8 * n, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(ds.in_normals.p, d->normals, 12 * n, hipMemcpyHostToDevice, s));
        if (variance) HIPCHK(ctx, hipMemcpyAsync(ds.in_var.p, variance, 4 * n, hipMemcpyHostToDevice, s));
    }
    HIPCHK(ctx, ds.ev.begin(s));
    DenoisePackArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.color = host ? (const unsigned char*)ds.in_color.p : (const unsigned char*)d->color;
    pa.pitch = host ? (long long)in_row : (long long)in_pitch;
    pa.hits = host ? (const int*)ds.in_hits.p : (const int*)d->hits;
    pa.normals = host ? (const float*)ds.in_normals.p : d->normals;
    pa.col = (float4*)ds.col_a.p;
    pa.guide = (float4*)ds.guide.p;
    pa.W = d->width;
    pa.n = (long long)n;
    hipError_t e;
    hipLaunchKernelGGL(ort_denoise_pack, dim3((unsigned)((n + kDenoiseBlock - 1) / kDenoiseBlock)), dim3(kDenoiseBlock), 0, s, pa);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_denoise_pack launch");
    if (variance) {
        hipLaunchKernelGGL(ort_denoise_pack_var, dim3((unsigned)((n + kDenoiseBlock - 1) / kDenoiseBlock)), dim3(kDenoiseBlock), 0,
                           s, host ? (const float*)ds.in_var.p : variance, (float*)ds.var_a.p, d->width, d->rows);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_denoise_pack_var launch");
    }
    DenoiseIterExArgs xa;
    std::memset(&xa, 0, sizeof(xa));
    xa.sv2 = sigma_variance * sigma_variance;
    DenoiseIterArgs& a = xa.base;
    a.guide = (const float4*)ds.guide.p;
    a.segs = (int)((W + kDenoiseBlock - 1) / kDenoiseBlock);
    const long long blocks = (long long)a.segs * (long long)rows;  // at most 2^30: a 1-D grid
    for (int i = 0; i < d->iterations; ++i) {
        const bool last = i + 1 == d->iterations;
        a.K = denoise_iter(d, i);
        a.cur = (const float4*)((i & 1) ? ds.col_b.p : ds.col_a.p);
        if (!last) {
            a.out = (i & 1) ? ds.col_a.p : ds.col_b.p;
            a.out_pitch = 0;
        } else {
            a.out = host ? ds.out.p : o->data;
            a.out_pitch = host ? (long long)out_row : (long long)out_pitch;
        }
        const int fmt = !last ? 0 : (o->format == ORT_FORMAT_RGBA8 ? 2 : 1);
        if (variance || (last && gamma)) {
            xa.var = (const float*)((i & 1) ? ds.var_b.p : ds.var_a.p);
            xa.next_var = last ? nullptr : (float*)((i & 1) ? ds.var_a.p : ds.var_b.p);
            xa.gamma = last && gamma;
            if ((e = launch_denoise_iter_ex(fmt, variance != nullptr, blocks, s, xa)) != hipSuccess)
                return hip_fail(ctx, e, "ort_denoise_iter_ex launch");
            continue;
        }
        if ((e = launch_denoise_iter(fmt, blocks, s, a)) != hipSuccess) return hip_fail(ctx, e, "ort_denoise_iter launch");
    }
    HIPCHK(ctx, ds.ev.end(s));
    if (host) {
        HIPCHK(ctx, hipMemcpy2DAsync(o->data, out_pitch, ds.out.p, out_row, out_row, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    } else if (!stream) {
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return ORT_OK;
}

}  // namespace

extern "C" {

int ort_denoise(ort_ctx* ctx, const ort_denoise_desc* d, const ort_output* output, void* stream) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_denoise: null ctx");
    try {
        const std::string bad = check_denoise(d, output);
        if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_denoise: " + bad);
        return denoise_impl(ctx, d, nullptr, 0.0f, false, output, stream);
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_denoise: ") + ex.what());
    }
}

int ort_denoise_ex(ort_ctx* ctx, const ort_denoise_desc_ex* d, const ort_output* output, void* stream) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_denoise_ex: null ctx");
    try {
        const std::string bad = check_denoise_ex(d, output);
        if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_denoise_ex: " + bad);
        return denoise_impl(ctx, &d->base, d->variance, d->sigma_variance, (d->base.flags & ORT_DENOISE_GAMMA) != 0, output,
                            stream);
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_denoise_ex: ") + ex.what());
    }
}

int ort_last_denoise_ms(ort_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_last_denoise_ms: null argument");
    if (!ctx->denoise.ev.timed) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_last_denoise_ms: no denoise launched yet");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, ctx->denoise.ev.elapsed(ms));
    return ORT_OK;
}

#if ORT_ANALYSIS
}  // extern "C"
namespace {
// TEST-ONLY host emulation (ort_internal.h): the pack pass and every iteration on the CPU, one pixel
// after another through denoise_pixel; d's pointers and output->data are host pointers.  variance
// (NULL: the term off), sigma_variance and gamma are ort_denoise_ex's.
int debug_denoise_impl(const ort_denoise_desc* d, const float* variance, float sigma_variance, bool gamma, const ort_output* o) {
    const size_t W = (size_t)d->width, rows = (size_t)d->rows, n = W * rows;
    if (n == 0) return ORT_OK;
    const size_t in_pitch = d->color_pitch_bytes ? (size_t)d->color_pitch_bytes : 12 * W;
    const size_t out_pitch = o->row_pitch_bytes ? (size_t)o->row_pitch_bytes : (size_t)format_bpp(o->format) * W;
    std::vector<float4> guide(n), a(n), b(d->iterations > 1 ? n : 0);
    std::vector<float> va(variance ? n : 0), vb(variance && d->iterations > 1 ? n : 0);
    const float sv2 = sigma_variance * sigma_variance;
    for (size_t i = 0; variance && i < n; ++i)  // ort_denoise_pack_var
        va[i] = denoise_prefilter(variance, (int)W, (int)rows, (int)(i % W), (int)(i / W));
    for (size_t i = 0; i < n; ++i) {  // ort_denoise_pack
        const size_t row = i / W, x = i - row * W;
        const float* c = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(d->color) + row * in_pitch) + 3 * x;
        a[i] = dn_color_record(c[0], c[1], c[2], d->hits[i].sphere);
        guide[i].x = d->normals[3 * i];
        guide[i].y = d->normals[3 * i + 1];
        guide[i].z = d->normals[3 * i + 2];
        guide[i].w = d->hits[i].t;
    }
    for (int it = 0; it < d->iterations; ++it) {
        const DenoiseIter K = denoise_iter(d, it);
        const float4* cur = (it & 1) ? b.data() : a.data();
        float4* next = (it & 1) ? a.data() : b.data();
        const float* var = (it & 1) ? vb.data() : va.data();
        float* next_var = (it & 1) ? va.data() : vb.data();
        const bool last = it + 1 == d->iterations;
        for (size_t y = 0; y < rows; ++y)
            for (size_t x = 0; x < W; ++x) {
                float nv = 0.0f;
                float4 v = variance ? denoise_pixel<true>(K, cur, guide.data(), (int)x, (int)y, var, sv2, &nv)
                                    : denoise_pixel<false>(K, cur, guide.data(), (int)x, (int)y);
                if (last && gamma) {
                    const ort::V3 g = ort::finish_pixel(ort::mk(v.x, v.y, v.z), 1);
                    v.x = g.x;
                    v.y = g.y;
                    v.z = g.z;
                }
                if (!last) {
                    next[y * W + x] = v;
                    if (variance) next_var[y * W + x] = nv;
                } else if (o->format == ORT_FORMAT_RGBA8) {
                    reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(o->data) + y * out_pitch)[x] =
                        ort::pack_rgba8(ort::mk(v.x, v.y, v.z));
                } else {
                    float* p = reinterpret_cast<float*>(static_cast<unsigned char*>(o->data) + y * out_pitch) + 3 * x;
                    p[0] = v.x;
                    p[1] = v.y;
                    p[2] = v.z;
                }
            }
    }
    return ORT_OK;
}
}  // namespace
extern "C" {

int ort_debug_denoise(const ort_denoise_desc* d, const ort_output* o) {
    try {
        const std::string bad = check_denoise(d, o);
        if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_denoise: " + bad);
        if (d->on_device) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_denoise: host pointers only");
        return debug_denoise_impl(d, nullptr, 0.0f, false, o);
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

// TEST-ONLY host emulation of ort_denoise_ex (ort_internal.h): the same loops with the prefilter,
// denoise_pixel<true> and the gamma.
int ort_debug_denoise_ex(const ort_denoise_desc_ex* d, const ort_output* o) {
    try {
        const std::string bad = check_denoise_ex(d, o);
        if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_denoise_ex: " + bad);
        if (d->base.on_device) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_denoise_ex: host pointers only");
        return debug_denoise_impl(&d->base, d->variance, d->sigma_variance, (d->base.flags & ORT_DENOISE_GAMMA) != 0, o);
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}
#endif  // ORT_ANALYSIS

}  // extern "C"
