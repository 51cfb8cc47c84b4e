// Piece of render_core.h, not to be included alone: the exact, explicit and brute-force walks.
namespace ort {
// Frame storage for traverse_compact: device = LDS columns, host = local arrays.
struct LdsFrames {
    int* co;     // co[level * stride + lane]
    float* tm;
    int stride;
    int lane;
    ORT_FN void set(int L, int c, float t) { co[L * stride + lane] = c; tm[L * stride + lane] = t; }
    ORT_FN void setCo(int L, int c) { co[L * stride + lane] = c; }
    ORT_FN int getCo(int L) const { return co[L * stride + lane]; }
    ORT_FN float getTm(int L) const { return tm[L * stride + lane]; }
};
struct LocalFrames {
    int co[ORT_COMPACT_MAX_DEPTH + 1];
    float tm[ORT_COMPACT_MAX_DEPTH + 1];
    ORT_FN void set(int L, int c, float t) { co[L] = c; tm[L] = t; }
    ORT_FN void setCo(int L, int c) { co[L] = c; }
    ORT_FN int getCo(int L) const { return co[L]; }
    ORT_FN float getTm(int L) const { return tm[L]; }
};

// Per-level masks of remaining children (rank space), levels 0..11 in 96 bits.
struct LevelMasks {
    uint64_t lo;  // levels 0..7, one byte each
    uint32_t hi;  // levels 8..11
    ORT_FN void clear() { lo = 0; hi = 0; }
    ORT_FN void put(int L, uint32_t m) {
        if (L < 8) lo |= (uint64_t)m << (8 * L);
        else hi |= m << (8 * (L - 8));
    }
    ORT_FN int top() const {
        if (hi) return 8 + ((31 - __builtin_clz(hi)) >> 3);
        if (lo) return (63 - __builtin_clzll(lo)) >> 3;
        return -1;
    }
    // pops the lowest rank of level L; returns the rank
    ORT_FN int pop(int L) {
        if (L < 8) {
            const uint32_t m = (uint32_t)(lo >> (8 * L)) & 0xffu;
            const int r = __builtin_ctz(m);
            lo &= ~((uint64_t)1 << (8 * L + r));
            return r;
        }
        const uint32_t m = (hi >> (8 * (L - 8))) & 0xffu;
        const int r = __builtin_ctz(m);
        hi &= ~(1u << (8 * (L - 8) + r));
        return r;
    }
};

// Child-box entry t of octant `oct` for a node at depth `dep` with cell (cx,cy,cz):
// recomputes the reference's rayBoxIntersection for that child (tmin only + hit flag).
ORT_FN float plane_t(float inv, float p, float o) { return inv * (p - o); }

template <bool COUNT, class Frames>
ORT_FN bool traverse_compact(const KScene& S, const float* planes, const Ray& r, float t_min, float t_max,
                             int& hitEntry, float& hitT, Frames& fr, Counters& cnt) {
    const int D = S.depth;
    const int S1 = fast_axis_floats(D);  // fast_plane_floats layout: forward tables at a * S1
    const float* PX = planes;
    const float* PY = planes + S1;
    const float* PZ = planes + 2 * S1;
    const V3 inv = mk(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
    const float a = dot(r.d, r.d);
    {
        float t0, t1;
        const V3 bmin = mk(PX[0], PY[0], PZ[0]);
        const V3 bmax = mk(PX[1 << D], PY[1 << D], PZ[1 << D]);
        if (!ray_box(r, inv, bmin, bmax, t0, t1)) return false;
    }
    const uint32_t ocode = order_code(r.d);
    int node = 0, depth = 0;
    uint32_t cx = 0, cy = 0, cz = 0;
    float ntmin = t_min;
    const float closest0 = t_max;
    float closest = t_max;
    bool hit = false;
    LevelMasks masks;
    masks.clear();
    for (;;) {
        const uint2 rec = S.node[node];
        if (COUNT) cnt.v[0] += 1;
        if (rec.y & ORT_INTERNAL_FLAG) {
            const int co = (int)rec.x;
            const uint32_t cmask = rec.y & 0xffu;
            if (COUNT) {
                const long long rem = (long long)S.n_nodes - (long long)co;
                cnt.v[1] += (unsigned long long)(rem >= 8 ? 8 : (rem > 0 ? rem : 0));
            }
            const int s = D - depth;  // >= 1 for an internal node
            const float tx0 = plane_t(inv.x, PX[cx << s], r.o.x);
            const float tx1 = plane_t(inv.x, PX[(2 * cx + 1) << (s - 1)], r.o.x);
            const float tx2 = plane_t(inv.x, PX[(cx + 1) << s], r.o.x);
            const float ty0 = plane_t(inv.y, PY[cy << s], r.o.y);
            const float ty1 = plane_t(inv.y, PY[(2 * cy + 1) << (s - 1)], r.o.y);
            const float ty2 = plane_t(inv.y, PY[(cy + 1) << s], r.o.y);
            const float tz0 = plane_t(inv.z, PZ[cz << s], r.o.z);
            const float tz1 = plane_t(inv.z, PZ[(2 * cz + 1) << (s - 1)], r.o.z);
            const float tz2 = plane_t(inv.z, PZ[(cz + 1) << s], r.o.z);
            float xa0, xa1, xb0, xb1, ya0, ya1, yb0, yb1, za0, za1, zb0, zb1;
            slab(tx0, tx1, xa0, xa1);  // lower x half: min = mid-split plane order bot/top
            slab(tx1, tx2, xb0, xb1);
            slab(ty0, ty1, ya0, ya1);
            slab(ty1, ty2, yb0, yb1);
            slab(tz0, tz1, za0, za1);
            slab(tz1, tz2, zb0, zb1);
            uint32_t rmask = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int oct = (int)((ocode >> (3 * k)) & 7u);
                if ((cmask >> oct) & 1u) {
                    const bool xh = (oct >> 1) & 1, yh = oct & 1, zh = (oct >> 2) & 1;
                    const float cmin = ort_maxf(ort_maxf(xh ? xb0 : xa0, yh ? yb0 : ya0), zh ? zb0 : za0);
                    const float cmax = ort_minf(ort_minf(xh ? xb1 : xa1, yh ? yb1 : ya1), zh ? zb1 : za1);
                    const bool keep = (cmax >= cmin) && !(cmax < ntmin) && !(cmin > closest0);
                    if (keep) rmask |= 1u << k;
                }
            }
            if (rmask) {
                masks.put(depth, rmask);
                fr.set(depth, co, ntmin);
            }
        } else {
            const int off = (int)rec.x;
            const int n = (int)rec.y;
            for (int i = 0; i < n; ++i) {
                const float4 sp = S.leaf_sph[off + i];
                if (COUNT) cnt.v[2] += 1;
                float t;
                if (sphere_hit_t<true>(r, a, sp, ntmin, closest, t)) {  // leaf_sph: .w = r^2
                    hit = true;
                    closest = t;
                    hitEntry = off + i;
                    if (COUNT) cnt.v[3] += 1;
                }
            }
            if (hit) break;  // glsl:336: the walk ends after the leaf that produced a hit
        }
        const int L = masks.top();
        if (L < 0) break;
        const int rk = masks.pop(L);
        const int oct = (int)((ocode >> (3 * rk)) & 7u);
        const int sh = depth - L;  // current node is at `depth`; its ancestor at level L
        cx = ((cx >> sh) << 1) | (uint32_t)((oct >> 1) & 1);
        cy = ((cy >> sh) << 1) | (uint32_t)(oct & 1);
        cz = ((cz >> sh) << 1) | (uint32_t)((oct >> 2) & 1);
        depth = L + 1;
        node = fr.getCo(L) + oct;
        // the tmin the reference pushed: max(childTMin, parent node_tmin) (glsl:474)
        const int s = D - depth;
        float xl, xu, yl, yu, zl, zu;
        slab(plane_t(inv.x, PX[cx << s], r.o.x), plane_t(inv.x, PX[(cx + 1) << s], r.o.x), xl, xu);
        slab(plane_t(inv.y, PY[cy << s], r.o.y), plane_t(inv.y, PY[(cy + 1) << s], r.o.y), yl, yu);
        slab(plane_t(inv.z, PZ[cz << s], r.o.z), plane_t(inv.z, PZ[(cz + 1) << s], r.o.z), zl, zu);
        const float cmin = ort_maxf(ort_maxf(xl, yl), zl);
        ntmin = ort_maxf(cmin, fr.getTm(L));
    }
    hitT = closest;
    return hit;
}

// Literal restatement of traverseOctree (glsl:290-481) over the reference record layout
// (boxes read from memory, 200-entry stack).  Used for trees the compact layout cannot
// represent.  `stack_node`/`stack_tmin` point at ORT_MAX_STACK entries owned by the lane.
template <bool COUNT>
ORT_FN bool traverse_explicit(const KScene& S, const Ray& r, float t_min, float t_max, int& hitEntry, float& hitT,
                              int* stack_node, float* stack_tmin, Counters& cnt) {
    const V3 inv = mk(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
    const float a = dot(r.d, r.d);
    int sp = 0;
    stack_node[0] = 0;
    stack_tmin[0] = t_min;
    bool hit = false;
    float closest = t_max;
    {
        const float4 A = S.nodeA[0], B = S.nodeB[0];
        float t0, t1;
        if (!ray_box(r, inv, mk(A.x, A.y, A.z), mk(B.x, B.y, B.z), t0, t1)) return false;
    }
    const uint32_t ocode = order_code(r.d);
    // bounded so that a malformed (cyclic) upload cannot hang the GPU
    for (long long guard = 0; sp >= 0 && guard < (1ll << 26); ++guard) {
        const int nodeIdx = stack_node[sp];
        const float ntmin = stack_tmin[sp];
        --sp;
        if (COUNT) cnt.v[0] += 1;
        const float4 A = S.nodeA[nodeIdx], B = S.nodeB[nodeIdx];
        const int co = f2i(A.w);
        const int oo = f2i(B.w);
        const int objectCount = S.count[nodeIdx];
        if (co == -1) {
            for (int i = 0; i < objectCount; ++i) {
                const int e = oo + i;
                const float4 spr = S.sph_cr[S.indices[e]];
                if (COUNT) cnt.v[2] += 1;
                float t;
                if (sphere_hit_t(r, a, spr, ntmin, closest, t)) {
                    hit = true;
                    closest = t;
                    hitEntry = e;
                    sp = -1;
                    if (COUNT) cnt.v[3] += 1;
                }
            }
        } else {
            for (int i = 7; i >= 0; --i) {
                const int oct = (int)((ocode >> (3 * i)) & 7u);
                const int childIdx = co + oct;
                if (childIdx >= S.n_nodes) continue;
                if (COUNT) cnt.v[1] += 1;
                const float4 CA = S.nodeA[childIdx], CB = S.nodeB[childIdx];
                float cmin, cmax;
                const bool boxhit = ray_box(r, inv, mk(CA.x, CA.y, CA.z), mk(CB.x, CB.y, CB.z), cmin, cmax);
                if (!boxhit || cmax < ntmin || cmin > closest ||
                    (f2i(CA.w) == -1 && f2i(CB.w) == -1))
                    continue;
                if (sp < ORT_MAX_STACK - 1) {
                    ++sp;
                    stack_node[sp] = childIdx;
                    stack_tmin[sp] = ort_maxf(cmin, ntmin);
                }
            }
        }
    }
    hitT = closest;
    return hit;
}

// bruteForceIntersect (glsl:484-498): exact closest hit over all spheres.
template <bool COUNT>
ORT_FN bool traverse_brute(const KScene& S, const Ray& r, float t_min, float t_max, int& hitSphere, float& hitT,
                           Counters& cnt) {
    const float a = dot(r.d, r.d);
    bool hit = false;
    float closest = t_max;
#if defined(__HIP_DEVICE_COMPILE__)
    // the fast walk's sphere test (per-ray correctly rounded 1/a, Markstein quotient, guarded
    // sqrt: the same roots) whenever its preconditions hold for the wave, and the spheres read
    // with scalar loads -- every lane tests sphere i at once, so the address is wave-uniform
    if (!COUNT && !any_lane(!(t_min == kFastTMin && a_in_qdiv_range(a)))) {
        const float ya = 1.0f / a;
        typedef __attribute__((address_space(4))) const float4 ConstF4;
        ConstF4* sph = (ConstF4*)S.sph_cr;
        for (int i = 0; i < S.n_spheres; ++i) {
            const float4 s4 = sph[i];
            float t;
            // (radius^2 as sphere_hit_t computes it: one rounded product)
            if (sphere_hit_fast(r, a, ya, make_float4(s4.x, s4.y, s4.z, s4.w * s4.w), t_min, closest, t)) {
                hit = true;
                closest = t;
                hitSphere = i;
            }
        }
        hitT = closest;
        return hit;
    }
#endif
    for (int i = 0; i < S.n_spheres; ++i) {
        float t;
        if (COUNT) cnt.v[2] += 1;
        if (sphere_hit_t(r, a, S.sph_cr[i], t_min, closest, t)) {
            hit = true;
            closest = t;
            hitSphere = i;
            if (COUNT) cnt.v[3] += 1;
        }
    }
    hitT = closest;
    return hit;
}
}  // namespace ort
