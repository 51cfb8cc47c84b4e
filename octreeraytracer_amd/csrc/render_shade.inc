// Piece of render_core.h, not to be included alone: shading -- random directions, bsdf, camera rays, trace_ray, shade_pixel.
namespace ort {
struct HitRec {
    float t;
    V3 point, normal;
    int mat;
    V3 albedo;
    float fuzz, ri;
};

// --- random directions (glsl:104-173) ---
ORT_FN V3 random_in_unit_disk(ort_rng& st) {
    const float PI_F = (float)3.14159265359;
    const float spx = 2.0f * ort_rand2D(&st) - 1.0f;
    const float spy = 2.0f * ort_rand2D(&st) - 1.0f;
    // the four branches of glsl:109-131 with their one division hoisted out (divergent
    // branches each ran a full IEEE division): q = num / den, then the branch's phi from q
    const bool right = spx > -spy;
    const bool xbig = right ? (spx > spy) : (spx < spy);  // |spx| dominates: phi from spy / spx
    const float r = right ? (xbig ? spx : spy) : (xbig ? -spx : -spy);
    const float q = (xbig ? spy : spx) / (xbig ? spx : spy);
    float phi;
    if (xbig) phi = right ? q : 4.0f + q;
    else phi = right ? 2.0f - q : (spy != 0.0f ? 6.0f - q : 0.0f);
    phi *= PI_F / 4.0f;
    float sp, cp;
    ort_sincosf(phi, &sp, &cp);  // = ort_sinf(phi), ort_cosf(phi): one reduction
    return mk(r * cp, r * sp, 0.0f);
}
ORT_FN V3 random_in_unit_sphere(ort_rng& st) {
    const float PI_F = (float)3.14159265359;
    const float z = 2.0f * ort_rand2D(&st) - 1.0f;
    const float phi = 2.0f * PI_F * ort_rand2D(&st);
    const float r = ort_powf(ort_rand2D(&st), 1.0f / 3.0f);
    const float s = sqrtf(1.0f - z * z);
    float sp, cp;
    ort_sincosf(phi, &sp, &cp);
    return mk(r * s * cp, r * s * sp, r * z);
}
ORT_FN V3 random_cosine_direction(ort_rng& st) {
    const float PI_F = (float)3.14159265359;
    const float r1 = ort_rand2D(&st);
    const float r2 = ort_rand2D(&st);
    const float phi = 2.0f * PI_F * r1;
    const float sr2 = sqrtf(r2);
    float sp, cp;
    ort_sincosf(phi, &sp, &cp);
    return mk(cp * sr2, sp * sr2, sqrtf(1.0f - r2));
}

ORT_FN bool refract_vec(V3 v, V3 n, float ni_over_nt, V3& refracted) {
    const V3 uv = normalize(v);
    const float dt = dot(uv, n);
    const float disc = 1.0f - ni_over_nt * ni_over_nt * (1.0f - dt * dt);
    if (disc > 0.0f) {
        const float sq = sqrtf(disc);
        refracted = mk(ni_over_nt * (uv.x - n.x * dt) - n.x * sq, ni_over_nt * (uv.y - n.y * dt) - n.y * sq,
                       ni_over_nt * (uv.z - n.z * dt) - n.z * sq);
        return true;
    }
    return false;
}
ORT_FN float schlick(float cosine, float ri) {
    float r0 = (1.0f - ri) / (1.0f + ri);
    r0 = r0 * r0;
    return r0 + (1.0f - r0) * ort_powf(1.0f - cosine, 5.0f);
}

// Material_bsdf (glsl:525-589)
// FINAL: nothing after this bounce reads the scattered ray or the RNG state (last bounce of
// the last sample), so only what reaches the pixel is computed: Lambert and dielectric
// attenuations do not depend on the sampled direction (their sampling is skipped); metal
// still samples, its absorption test needs the direction.
template <bool FINAL = false>
ORT_FN bool bsdf(const HitRec& h, const Ray& wo, Ray& wi, V3& att, ort_rng& st) {
    wi.o = h.point;
    if (FINAL && (h.mat == 0 || h.mat == 2)) {
        att = h.mat == 0 ? h.albedo : mk(1.0f, 1.0f, 1.0f);
        wi.d = wo.d;
        return true;
    }
    switch (h.mat) {
        case 0: {
            const V3 ld = random_cosine_direction(st);
            const V3 w = h.normal;
            const V3 a = (fabsf(w.x) > 0.1f) ? mk(0.0f, 1.0f, 0.0f) : mk(1.0f, 0.0f, 0.0f);
            const V3 u = normalize(cross(a, w));
            const V3 v = cross(w, u);
            wi.d = normalize(mk((ld.x * u.x + ld.y * v.x) + ld.z * w.x, (ld.x * u.y + ld.y * v.y) + ld.z * w.y,
                                (ld.x * u.z + ld.y * v.z) + ld.z * w.z));
            att = h.albedo;
            return true;
        }
        case 1: {
            const float fuzz = h.fuzz;
            const V3 refl = reflect(normalize(wo.d), h.normal);
            const V3 rs = random_in_unit_sphere(st);
            wi.d = mk(refl.x + fuzz * rs.x, refl.y + fuzz * rs.y, refl.z + fuzz * rs.z);
            att = h.albedo;
            return dot(wi.d, h.normal) > 0.0f;
        }
        case 2: {
            V3 outward;
            float ni_over_nt, cosine;
            const float ri = h.ri;
            att = mk(1.0f, 1.0f, 1.0f);
            if (dot(wo.d, h.normal) > 0.0f) {
                outward = mk(-h.normal.x, -h.normal.y, -h.normal.z);
                ni_over_nt = ri;
                cosine = dot(wo.d, h.normal) / length(wo.d);
                cosine = sqrtf(1.0f - ri * ri * (1.0f - cosine * cosine));
            } else {
                outward = h.normal;
                ni_over_nt = 1.0f / ri;
                cosine = -dot(wo.d, h.normal) / length(wo.d);
            }
            V3 refracted = mk(0.0f, 0.0f, 0.0f);
            const bool can = refract_vec(wo.d, outward, ni_over_nt, refracted);
            const float prob = can ? schlick(cosine, ri) : 1.0f;
            if (ort_rand2D(&st) < prob) wi.d = reflect(wo.d, h.normal);
            else wi.d = refracted;
            return true;
        }
        default:
            return false;
    }
}

ORT_FN V3 sky_color(const Ray& r) {
    const float t = 0.5f * (r.d.y + 1.0f);
    return mk((1.0f - t) * 1.0f + t * 0.5f, (1.0f - t) * 1.0f + t * 0.7f, (1.0f - t) * 1.0f + t * 1.0f);
}

// Camera_getRay (glsl:205-221)
ORT_FN Ray camera_ray(const KCamera& c, float s, float t, float W, float H, ort_rng& st) {
    const float pixelRadius = 0.5f / ort_maxf(W, H);
    const float jx = pixelRadius * (ort_rand2D(&st) - 0.5f);
    const float jy = pixelRadius * (ort_rand2D(&st) - 0.5f);
    const V3 rdd = random_in_unit_disk(st);
    const V3 rd = mk(c.lensRadius * rdd.x, c.lensRadius * rdd.y, c.lensRadius * rdd.z);
    const V3 off = mk(c.u.x * rd.x + c.v.x * rd.y, c.u.y * rd.x + c.v.y * rd.y, c.u.z * rd.x + c.v.z * rd.y);
    Ray r;
    r.o = add(c.origin, off);
    const float a = s + jx, b = t + jy;
    r.d = normalize(mk((((c.lowerLeft.x + a * c.horizontal.x) + b * c.vertical.x) - c.origin.x) - off.x,
                       (((c.lowerLeft.y + a * c.horizontal.y) + b * c.vertical.y) - c.origin.y) - off.y,
                       (((c.lowerLeft.z + a * c.horizontal.z) + b * c.vertical.z) - c.origin.z) - off.z));
    return r;
}

// ---------------------------------------------------------------------------------------
// Path steps.  The GPU runs them as a wavefront pipeline (ort_kernel.hip: trace kernel ->
// rare exact-walk kernel -> shade kernel, per bounce); shade_pixel below chains the same
// steps for one pixel (host emulation / reference order).  Both orders give identical
// pixels because every path is independent and each step is a pure function of its state.

struct PixelParams {
    KCamera cam;
    int W, H, ns, maxDepth;
};

// main() prologue + the sample-s part of its loop up to radiance()'s first line
// (glsl:640, 647-654, 602): consumes 2 + 4 rand2D, returns the normalised camera ray.
// st must hold the pixel's RNG state at the start of sample s (FragCoord/iResolution for s=0).
ORT_FN void pixel_rng_init(const PixelParams& P, int px, int py, ort_rng& st) {
    st.x = ((float)px + 0.5f) / (float)P.W;
    st.y = ((float)py + 0.5f) / (float)P.H;
}
ORT_FN Ray primary_ray(const PixelParams& P, int px, int py, int s, ort_rng& st) {
    const float W = (float)P.W, H = (float)P.H;
    const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
    const int sqrt_ns = (int)sqrtf((float)P.ns);
    const int i = s % sqrt_ns;
    const int j = s / sqrt_ns;
    // x / 1.0f == x exactly: one sample per pixel (the benchmark) skips both divisions
    const float ru = (float)i + ort_rand2D(&st);
    const float u = (fx + (sqrt_ns == 1 ? ru : ru / (float)sqrt_ns)) / W;
    const float rv = (float)j + ort_rand2D(&st);
    const float v = (fy + (sqrt_ns == 1 ? rv : rv / (float)sqrt_ns)) / H;
    Ray ray = camera_ray(P.cam, u, v, W, H, st);
    ray.d = normalize(ray.d);
    return ray;
}

#define ORT_TRACE_MISS 0
#define ORT_TRACE_HIT 1
#define ORT_TRACE_DEFER 2

// intersectScene(ray, 0.001, MAXFLOAT) (glsl:500-506, 607).  MODE: 0 compact octree,
// 1 explicit octree, 2 brute force.  With MODE 0 and allow_defer, a ray the fast walk
// cannot take (some 1/d component not finite) is reported as DEFER instead of walking
// it exactly here, so the exact walk's registers stay out of the hot kernel.
// bounce: the ray of a bounce >= 1 -- walked like the GPU's bounce kernel does (Masks64Plain /
// Masks96Lean: no inline leaf children, the rejected-sphere skip; at depth 9-10 over the plane
// tables planes_b in the Masks96Lean layout), same result.
template <int MODE, bool COUNT, class Frames>
ORT_FN int trace_ray(const KScene& S, const float* planes, const uint8_t* rank_lut, const Ray& r, bool allow_defer,
                     float& t, int& entry, Frames& fr, int* snode, float* stmin, Counters& cnt, bool bounce = false,
                     const float* planes_b = nullptr) {
    bool hit;
    entry = -1;
    t = 0.0f;
    if (MODE == 0) {
        V3 inv = mk(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
        if (rank_lut && fast_prepare(S, r, inv)) {
            if (COUNT) cnt.v[5] += 1;
            if (!bounce)
                hit = traverse_fast<COUNT>(S, planes, rank_lut, r, inv, 0.001f, ORT_MAXFLOAT, entry, t, fr, cnt);
            else if (S.depth <= 8)
                hit = traverse_fast_t<COUNT, Masks64Plain>(S, planes, rank_lut, r, inv, 0.001f, ORT_MAXFLOAT, entry, t, fr, cnt);
            else
                hit = traverse_fast_t<COUNT, Masks96Lean>(S, planes_b, rank_lut, r, inv, 0.001f, ORT_MAXFLOAT, entry, t, fr, cnt);
        } else if (allow_defer) {
            return ORT_TRACE_DEFER;
        } else {
            if (COUNT) cnt.v[5] += 1;
            hit = traverse_compact<COUNT>(S, planes, r, 0.001f, ORT_MAXFLOAT, entry, t, fr, cnt);
        }
    } else if (MODE == 1) {
        if (COUNT) cnt.v[5] += 1;
        hit = traverse_explicit<COUNT>(S, r, 0.001f, ORT_MAXFLOAT, entry, t, snode, stmin, cnt);
    } else {
        if (COUNT) cnt.v[5] += 1;
        hit = traverse_brute<COUNT>(S, r, 0.001f, ORT_MAXFLOAT, entry, t, cnt);
    }
    return hit ? ORT_TRACE_HIT : ORT_TRACE_MISS;
}

// The IntersectInfo Sphere_hit fills for the accepted hit (glsl:240-251).
template <int MODE>
ORT_FN HitRec hit_record(const KScene& S, const Ray& r, float t, int entry) {
    int sidx;
    float4 sp;
    if (MODE == 0) {
        sidx = S.leaf_idx[entry];
        sp = S.sph_cr[sidx];  // (leaf_sph holds radius^2)
    } else if (MODE == 1) {
        sidx = S.indices[entry];
        sp = S.sph_cr[sidx];
    } else {
        sidx = entry;
        sp = S.sph_cr[sidx];
    }
    HitRec h;
    h.t = t;
    h.point = mk(r.o.x + t * r.d.x, r.o.y + t * r.d.y, r.o.z + t * r.d.z);
    h.normal = mk((h.point.x - sp.x) / sp.w, (h.point.y - sp.y) / sp.w, (h.point.z - sp.z) / sp.w);
    const float4 ma = S.sph_ma[sidx];
    const float2 fr2 = S.sph_fr[sidx];
    h.mat = (int)ma.x;
    h.albedo = mk(ma.y, ma.z, ma.w);
    h.fuzz = fr2.x;
    h.ri = fr2.y;
    return h;
}

// One iteration of radiance()'s bounce loop after intersectScene (glsl:607-627).
// Returns true when the path ends here (absorbed, or escaped to the sky).
template <bool FINAL = false>
ORT_FN bool shade_bounce(bool hit, const HitRec& h, Ray& ray, V3& c, float& importance, ort_rng& st) {
    if (hit) {
        Ray wi;
        wi.d = ray.d;
        V3 att = mk(0.0f, 0.0f, 0.0f);
        const bool scattered = bsdf<FINAL>(h, ray, wi, att, st);
        ray.o = wi.o;
        ray.d = wi.d;
        if (!scattered) {
            c = mul(c, mk(0.0f, 0.0f, 0.0f));
            return true;
        }
        c = mul(c, att);
        importance *= ort_maxf(att.x, ort_maxf(att.y, att.z));
        return false;
    }
    c = mul(c, sky_color(ray));
    return true;
}

// col /= float(numSamples); pow(col, 1/2.2) (glsl:659-661)
ORT_FN V3 finish_pixel(V3 col, int ns) {
    const float fns = (float)ns;
    if (ns != 1) col = mk(col.x / fns, col.y / fns, col.z / fns);  // x / 1.0f == x exactly
    const float g = 1.0f / 2.2f;
    return mk(ort_powf(col.x, g), ort_powf(col.y, g), ort_powf(col.z, g));
}

// One channel as the 8-bit default framebuffer holds it -- image.to_srgb8 in float32: NaN -> 0,
// clamp to [0, 1], one multiply by 255, one add of 0.5 (two roundings, as numpy's), truncate.
ORT_FN uint32_t quantise8(float x) {
    if (!(x == x)) x = 0.0f;
    x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    const float s = x * 255.0f;
    return (uint32_t)(int)(s + 0.5f);
}

// The finished pixel as one RGBA8 word: memory bytes R, G, B, A with A = 255 (ORT_FORMAT_RGBA8).
ORT_FN uint32_t pack_rgba8(V3 v) {
    return quantise8(v.x) | quantise8(v.y) << 8 | quantise8(v.z) << 16 | 0xFF000000u;
}

// main() of the fragment shader (glsl:636-664) for pixel (px, py), py = 0 the bottom row,
// as one sequential chain of the steps above (host emulation).
// planes_b: the bounce walk's plane tables (trace_ray).
// done: the samples taken, P.ns by default; fewer is the picture an accumulation shows after
// `done` samples (ort_accum_render): the first `done` samples of the P.ns-sample chain, in P.ns's
// strata, divided by `done`.
// sum_out, m2_out (host emulation of ort_accum_read_moments): the linear colour sum of those
// samples and the sum of their squared luminances, as a moments pass keeps them.
template <int MODE, bool COUNT, class Frames>
ORT_FN V3 shade_pixel(const PixelParams& P, const KScene& S, const float* planes, const float* planes_b,
                      const uint8_t* rank_lut, Frames& fr, int* snode, float* stmin, int px, int py, Counters& cnt,
                      int done = -1, V3* sum_out = nullptr, float* m2_out = nullptr) {
    if (done < 0) done = P.ns;
    float m2 = 0.0f;
    ort_rng st;
    pixel_rng_init(P, px, py, st);
    V3 col = mk(0.0f, 0.0f, 0.0f);
    for (int s = 0; s < done; ++s) {
        Ray ray = primary_ray(P, px, py, s, st);
        V3 c = mk(1.0f, 1.0f, 1.0f);
        float importance = 1.0f;
        for (int b = 0; b < P.maxDepth; ++b) {
            if (importance < 0.01f) break;
            float t;
            int entry;
            const int tr = trace_ray<MODE, COUNT>(S, planes, rank_lut, ray, false, t, entry, fr, snode, stmin, cnt, b > 0, planes_b);
            HitRec h;
            if (tr == ORT_TRACE_HIT) h = hit_record<MODE>(S, ray, t, entry);
            const bool hit = tr == ORT_TRACE_HIT;
            const bool fin = b == P.maxDepth - 1 && s == done - 1;  // the RNG state is dead after it
            if (fin ? shade_bounce<true>(hit, h, ray, c, importance, st) : shade_bounce(hit, h, ray, c, importance, st))
                break;
        }
        col = add(col, c);
        if (m2_out) {
            const float l = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
            m2 = m2 + l * l;
        }
    }
    if (sum_out) *sum_out = col;
    if (m2_out) *m2_out = m2;
    return finish_pixel(col, done);
}
}  // namespace ort
