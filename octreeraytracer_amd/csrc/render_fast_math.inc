// Piece of render_core.h, not to be included alone: the fast walk's rank order, preconditions and device helpers.
namespace ort {
// ---------------------------------------------------------------------------------------
// Fast path of traverse_compact for rays whose direction has no zero (or denormal-reciprocal)
// component, i.e. 1/d is finite on every axis.  Then no slab value can be NaN and, per
// axis, t(p) = inv*(p - o) is monotone in p, so every GLSL min/max of the reference is
// decided by the sign of d alone:
//   * the entry/exit of a child slab are its near/far planes' t (no compare needed); the
//     plane tables are read in ray order (index i -> table[g ? 2^D - i : i], g = d < 0), so
//     a node's near plane is its lower ray-order index and rank bit = "far half";
//   * the traversal order (glsl:352-447) of an all-non-zero sign vector is
//     order[r] = perm(r) ^ m, m = (d.z<0)<<2 | (d.x<0)<<1 | (d.y<0), perm = identity for
//     d.x > 0 and "swap bits 0,1" for d.x < 0 (checked for all 8 tables), so children are
//     evaluated directly in traversal-rank space with static role axes
//     A = rank bit 1 (x, or y when swapped), B = rank bit 0, C = rank bit 2 (z);
//   * IEEE max3/min3 equal the GLSL chains (no NaN); a +0/-0 tie can pick the other zero,
//     which is harmless because every tmin is only ever compared (never divided by).
// The reference pushes max(childTMin, node_tmin).  A child box lies inside its parent's
// (midpoint splits; checked at upload, layout.cpp), so its entry t on every axis is >= the
// parent's (fl is monotone), hence by induction node_tmin = max(max3(entries), t_min) for
// every node below the root: no per-level tmin has to be kept, and the push test
// (tmax >= tmin && !(tmax < node_tmin) && !(tmin > closest)) becomes
// min(tmax, t_max) >= max(tmin, t_min).  Results are bit-identical to the exact walk
// (tests/test_emulation.py forces both on the same rays).
//
// Stack: the reference stack holds exactly the unvisited surviving siblings of every
// ancestor in traversal order, i.e. per tree level a set of ranks plus the level's children
// offset.  Ranks are kept as "rank-reversed" bytes (rank r of level L = bit 8L + 7 - r) so the
// next node -- lowest rank of the deepest non-empty level -- is the highest set bit, and a
// descent is the same pop as a backtrack: every visited internal node pushes all its
// surviving children, then one uniform pop picks the next node.
//
// rank_lut[m*256 + childMask] maps the node's octant-space child mask to reversed rank space.
ORT_FN uint32_t rank_perm(uint32_t r, uint32_t m) {
    const uint32_t swap = (m >> 1) & 1u;  // perm = swap bits 0,1 when d.x < 0
    const uint32_t p = swap ? ((r & 4u) | ((r & 1u) << 1) | ((r >> 1) & 1u)) : r;
    return p ^ m;
}
ORT_FN uint8_t rank_lut_entry(uint32_t m, uint32_t cmask) {
    uint32_t out = 0;
    for (uint32_t r = 0; r < 8; ++r)
        if ((cmask >> rank_perm(r, m)) & 1u) out |= 0x80u >> r;
    return (uint8_t)out;
}

ORT_FN bool a_in_qdiv_range(float a) { return a >= 0.125f && a <= 8.0f; }
// The fast walk's t_min (the shader's only one, glsl:hit(r, 0.001, ...)) is a literal in the
// instruction stream rather than a per-ray register.
constexpr float kFastTMin = 0.001f;
// The fast walk's preconditions: finite 1/d and origin (no slab value can be NaN), a
// positive t_min and finite t_max (the push test below relies on both), dot(d,d) in
// qdiv's range.
ORT_FN bool fast_path_ok(const Ray& r, V3 inv, float t_min, float t_max) {
    return fabsf(inv.x) <= ORT_MAXFLOAT && fabsf(inv.y) <= ORT_MAXFLOAT && fabsf(inv.z) <= ORT_MAXFLOAT &&
           fabsf(r.o.x) <= ORT_MAXFLOAT && fabsf(r.o.y) <= ORT_MAXFLOAT && fabsf(r.o.z) <= ORT_MAXFLOAT &&
           t_min == kFastTMin && t_max <= ORT_MAXFLOAT && a_in_qdiv_range(dot(r.d, r.d));
}

// Rays with a zero (or tiny denormal) direction component have an infinite 1/d there.  Their
// slab values on that axis are +-inf (never NaN unless the origin lies exactly on one of the
// axis's split planes), and a box's [min, max] interval on it is (-inf, +inf) or empty
// whichever sign the infinity has -- so the box tests do not depend on that sign.  What does
// depend on it is the traversal order: the shader picks it from the sign vector with zeros
// (glsl:342-447), and each of those 26 vectors' table equals perm(r) ^ m' for one full sign
// mask m' whose non-zero components agree with the ray's (checked against the shader's tables,
// tests/test_math.py).  So such a ray walks the fast path with inv = +-inf on its zero axes,
// signed by m'.  kGlslOrderM: m' by (sx+1)*9 + (sy+1)*3 + (sz+1), 3 bits each, 9 per word.
constexpr uint32_t kGlslOrderM[3] = {0x259bedfu, 0x2518edfu, 0x90984du};
ORT_FN uint32_t glsl_order_m(float dx, float dy, float dz) {
    const int sx = dx < 0.0f ? 0 : (dx > 0.0f ? 2 : 1), sy = dy < 0.0f ? 0 : (dy > 0.0f ? 2 : 1),
              sz = dz < 0.0f ? 0 : (dz > 0.0f ? 2 : 1);
    const int idx = sx * 9 + sy * 3 + sz;
    return (kGlslOrderM[idx / 9] >> (3 * (idx % 9))) & 7u;
}
// Is v exactly one of the split planes of one axis (2^D + 1 entries)?  The table holds NaN
// where no node uses a plane (layout.cpp), so search it like the tree splits it: the planes
// inside (lo, hi) can be used only if the interval's mid plane is (a node with a boundary
// inside has an ancestor spanning (lo, hi) that was split there), and the used planes are
// ascending.  D steps; run only for the rare rays with a zero direction component.
ORT_FN bool on_split_plane(const float* P, int D, float v) {
    int lo = 0, hi = 1 << D;
    if (P[lo] == v || P[hi] == v) return true;
    if (!(v > P[lo] && v < P[hi])) return false;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const float pm = P[mid];
        if (!(pm == pm)) return false;
        if (pm == v) return true;
        if (v < pm) hi = mid;
        else lo = mid;
    }
    return false;
}
// The fast walk for a ray fast_path_ok refused only because some 1/d component is infinite:
// returns whether it may take the fast walk, with those components of inv signed by the
// shader's order (see above).  Refused: a zero direction vector (the shader leaves its order
// undefined), an origin on a split plane of a zero axis (NaN slabs), the other fast_path_ok
// conditions.
ORT_FN bool fast_zero_axes(const KScene& S, const Ray& r, V3& inv, float t_min, float t_max) {
    if (!(fabsf(r.o.x) <= ORT_MAXFLOAT && fabsf(r.o.y) <= ORT_MAXFLOAT && fabsf(r.o.z) <= ORT_MAXFLOAT) ||
        t_min != kFastTMin || !(t_max <= ORT_MAXFLOAT) || !a_in_qdiv_range(dot(r.d, r.d)))
        return false;
    if (r.d.x == 0.0f && r.d.y == 0.0f && r.d.z == 0.0f) return false;
    if (!(inv.x == inv.x) || !(inv.y == inv.y) || !(inv.z == inv.z)) return false;
    const uint32_t m = glsl_order_m(r.d.x, r.d.y, r.d.z);
    const int P1 = (1 << S.depth) + 1;
    float inf;
    const uint32_t inf_bits = 0x7f800000u;
    __builtin_memcpy(&inf, &inf_bits, 4);
    float* c[3] = {&inv.x, &inv.y, &inv.z};
    const float o[3] = {r.o.x, r.o.y, r.o.z};
    const uint32_t neg[3] = {(m >> 1) & 1u, m & 1u, (m >> 2) & 1u};
    for (int a = 0; a < 3; ++a) {
        if (fabsf(*c[a]) <= ORT_MAXFLOAT) continue;
        if (on_split_plane(S.planes + a * P1, S.depth, o[a])) return false;
        *c[a] = neg[a] ? -inf : inf;
    }
    return true;
}

// fast_path_ok, or else fast_zero_axes (rare: a zero direction component): inv may be re-signed.
ORT_FN bool fast_prepare(const KScene& S, const Ray& r, V3& inv) {
    if (fast_path_ok(r, inv, kFastTMin, ORT_MAXFLOAT)) return true;
    return fast_zero_axes(S, r, inv, kFastTMin, ORT_MAXFLOAT);
}

// 24-bit signed multiply (plane indices are < 2^11): one full-rate VALU op on the device.
ORT_FN int imul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// min/max for NaN-free operands.  On the device these are the raw VALU instructions: the
// libm-style fmaxf would first canonicalise every operand the compiler cannot prove
// canonical (one v_max x,x each), which the fast walk never needs.
#if defined(__HIP_DEVICE_COMPILE__)
ORT_FN float fmax2(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
ORT_FN float fmin2(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
ORT_FN float fmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
ORT_FN float fmin3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// max(x, kFastTMin) with the constant as an instruction literal (0x3a83126f = 0.001f)
ORT_FN float fmax_tmin(float x) { float r; asm("v_max_f32 %0, 0x3a83126f, %1" : "=v"(r) : "v"(x)); return r; }
#else
ORT_FN float fmax_tmin(float x) { return fmaxf(x, kFastTMin); }
ORT_FN float fmax2(float a, float b) { return fmaxf(a, b); }
ORT_FN float fmin2(float a, float b) { return fminf(a, b); }
ORT_FN float fmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
ORT_FN float fmin3(float a, float b, float c) { return fminf(fminf(a, b), c); }
#endif

// Correctly rounded n / a given y = RN(1/a): q0 = n*y is faithful, r = n - a*q0 is exact
// (fma), and RN(q0 + r*y) = RN(n/a) (Markstein's theorem; no division is ever exactly a
// midpoint).  Valid without underflow/overflow in r and q: |n| in [2^-60, 2^100] and
// a in [2^-3, 2^3] (checked per ray by fast_path_ok); otherwise the IEEE division.
// 2.56e9 random (n, a) pairs in those ranges were checked bitwise against n / a on the host
// (no artefact of that run is kept under profiles/; what the suite holds is tests/root_sets.py's
// families against the oracle, tests/test_root_edges.py and tests/test_gpu_root_edges.py).
// any_lane(p): p on any active lane of the wave (a wave-uniform branch: no exec-mask juggling
// around a path that is almost never taken); p itself on the host.
ORT_FN bool any_lane(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(p) != 0;
#else
    return p;
#endif
}
// n / a for the fast walk's sphere roots (callers: t_min >= kFastTMin).  Below |n| = 2^-60 the
// Markstein step may miss the correct rounding, but then |n / a| < 2^-57 (a >= 1/8) is far
// below t_min and the root is rejected whatever its last bit, so only |n| > 2^100 (and NaN)
// takes the IEEE division.
ORT_FN float qdiv(float n, float a, float y) {
    const float q0 = n * y;
    float q = fmaf(fmaf(-q0, a, n), y, q0);
    const float an = fabsf(n);
    const bool slow = !(an <= 0x1p100f);
    if (any_lane(slow)) q = slow ? n / a : q;
    return q;
}
// Correctly rounded sqrt for x in [2^-96, 2^100]: the hardware estimate corrected by the
// two residual tests of the compiler's own IEEE expansion, minus its denormal scaling and
// special-value handling (not needed in that range); otherwise sqrtf.
ORT_FN float qsqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u);
    const float sp = __uint_as_float(__float_as_uint(s) + 1u);
    float r = (fmaf(-sm, s, x) <= 0.0f) ? sm : s;
    r = (fmaf(-sp, s, x) > 0.0f) ? sp : r;
    // x in [2^-96, 2^100] as one unsigned compare of the bits (x > 0 here: disc > 0)
    const bool slow = f2u(x) - f2u(0x1p-96f) > f2u(0x1p100f) - f2u(0x1p-96f);
    if (any_lane(slow)) {
        // the volatile asm keeps this a real (wave-uniform) branch: left alone, the compiler
        // if-converts it and evaluates sqrtf's IEEE expansion on every call
        asm volatile("" ::: "memory");
        r = slow ? sqrtf(x) : r;
    }
    return r;
#else
    return sqrtf(x);
#endif
}

// Sphere_hit_t with the fast division/sqrt (ya = RN(1 / a)); same results.
ORT_FN bool sphere_hit_fast(const Ray& r, float a, float ya, float4 sp, float t_min, float t_max, float& t) {
    const V3 oc = mk(r.o.x - sp.x, r.o.y - sp.y, r.o.z - sp.z);
    const float half_b = dot(oc, r.d);
    const float c = dot(oc, oc) - sp.w;  // leaf_sph: .w = radius * radius
    const float disc = half_b * half_b - a * c;
    if (disc > 0.0f) {
        // both roots, no branch between them: the near one if in range, else the far one
        const float sq = qsqrt(disc);
        const float t1 = qdiv(-half_b - sq, a, ya);
        const float t2 = qdiv(-half_b + sq, a, ya);
        const bool ok1 = t1 < t_max && t1 > t_min;
        const bool ok2 = t2 < t_max && t2 > t_min;
        t = ok1 ? t1 : t2;
        return ok1 || ok2;
    }
    return false;
}
}  // namespace ort
