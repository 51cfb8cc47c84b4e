// Piece of render_core.h, not to be included alone: ray queries -- query_ray, the mode walk and the _q traversals.
namespace ort {
// --- ray queries (ort_trace_rays): a caller's ray -> {t, sphere, normal} ---
// What intersectScene(ray, 0.001, MAXFLOAT) finds, as the caller sees it: t, the index of the
// hit sphere in the uploaded arrays and IntersectInfo.normal; a miss is {0, -1, (0, 0, 0)}.
struct RayHit {
    float t;
    int sphere;
    V3 normal;
};

// The record of a finished walk (hit, t, entry as the traversals return them).  sphere and the
// normal are hit_record's: the same index by layout, the same float32 operations in the same
// order.  want_normal: the three divisions only where the caller asked for normals.
template <int MODE>
ORT_FN RayHit query_hit(const KScene& S, const Ray& r, bool hit, float t, int entry, bool want_normal) {
    RayHit q;
    q.t = 0.0f;
    q.sphere = -1;
    q.normal = mk(0.0f, 0.0f, 0.0f);
    if (!hit) return q;
    q.t = t;
    q.sphere = MODE == 0 ? S.leaf_idx[entry] : (MODE == 1 ? S.indices[entry] : entry);
    if (want_normal) {
        const float4 sp = S.sph_cr[q.sphere];
        const V3 p = mk(r.o.x + t * r.d.x, r.o.y + t * r.d.y, r.o.z + t * r.d.z);
        q.normal = mk((p.x - sp.x) / sp.w, (p.y - sp.y) / sp.w, (p.z - sp.z) / sp.w);
    }
    return q;
}

// One ray query, whole: the walk a bounce ray of the render path takes (trace_ray, bounce: the
// fast walk without inline leaf children where rank_lut is given and fast_prepare takes the ray,
// the literal exact walk otherwise; the explicit layout's stack walk; brute force) and its
// record.  The host emulation and the per-lane / exact query kernels call this; the persistent
// query kernel runs the same fast walk a step at a time and ends in query_hit.
template <int MODE, class Frames>
ORT_FN RayHit query_ray(const KScene& S, const float* planes, const float* planes_b, const uint8_t* rank_lut,
                        const Ray& r, Frames& fr, int* snode, float* stmin, bool want_normal) {
    Counters cnt;
    for (int k = 0; k < 6; ++k) cnt.v[k] = 0;
    float t;
    int entry;
    const int tr = trace_ray<MODE, false>(S, planes, rank_lut, r, false, t, entry, fr, snode, stmin, cnt, true, planes_b);
    return query_hit<MODE>(S, r, tr == ORT_TRACE_HIT, t, entry, want_normal);
}

// --- query modes (ort_trace_rays_ex): the nearest hit / any hit inside the ray's own interval ---
// c_k = what Sphere_hit(k, ray, t_min, t_max) accepts for sphere k alone (its near root if inside
// the open interval, else its far root if that one is).  NEAREST: the minimum of c_k over all
// spheres, the lowest k attaining it.  ANY: {c_k, k} of the first sphere found with one.  The tree
// is acceleration only: the walks below visit every leaf the ray touches inside the interval and
// test its spheres against the ray's (t_min, closest), never the node's entry -- unlike the
// shader's walk (traverse_compact / traverse_explicit), which leaves after the first leaf with a
// hit and so reports the sphere that is drawn.
#define ORT_QM_NEAREST 1
#define ORT_QM_ANY 2

// The interval as the walks take it: 0 <= t_min < t_max (anything else, NaN included, is a miss
// without a walk), t_max = +inf taken as MAXFLOAT.
ORT_FN bool query_interval(float t_min, float& t_max) {
    if (!(t_min >= 0.0f && t_min < t_max)) return false;
    if (t_max > ORT_MAXFLOAT) t_max = ORT_MAXFLOAT;
    return true;
}

// rayBoxIntersection on one axis with the zero-axis rule: where the direction component is +-0
// the box constrains the ray only by min <= origin <= max (closed), and contributes (-inf, +inf)
// to entry and exit -- the shader's inf * 0 = NaN, which makes its min/max drop the box for an
// origin exactly on a box plane, is never formed.  A ray outside the slab gets the empty
// (+inf, -inf).  Every other axis is the shader's arithmetic (slab).
ORT_FN void slab_q(float d, float inv, float o, float p0, float p1, float& lo, float& hi) {
    if (d == 0.0f) {
        const bool in = p0 <= o && o <= p1;
        lo = in ? -__builtin_inff() : __builtin_inff();
        hi = in ? __builtin_inff() : -__builtin_inff();
    } else {
        slab(inv * (p0 - o), inv * (p1 - o), lo, hi);
    }
}
ORT_FN bool ray_box_q(const Ray& r, V3 inv, V3 bmin, V3 bmax, float& tmin, float& tmax) {
    float x0, x1, y0, y1, z0, z1;
    slab_q(r.d.x, inv.x, r.o.x, bmin.x, bmax.x, x0, x1);
    slab_q(r.d.y, inv.y, r.o.y, bmin.y, bmax.y, y0, y1);
    slab_q(r.d.z, inv.z, r.o.z, bmin.z, bmax.z, z0, z1);
    tmin = ort_maxf(ort_maxf(x0, y0), z0);
    tmax = ort_minf(ort_minf(x1, y1), z1);
    return tmax >= tmin;
}

// Sphere_hit against (t_min, closest] while closest shrinks: 1 = c_k < closest, 2 = c_k == closest
// (the caller keeps the lower sphere index; before the first hit closest is the open t_max and a
// tie is no hit), 0 = neither.  The roots are sphere_hit_t's, operation for operation.  A near
// root beyond closest leaves the far root beyond it too, and a rejected tie of the near root can
// only tie again, so the result is c_k whenever c_k <= closest.
template <bool R2>
ORT_FN int sphere_hit_q(const Ray& r, float a, float4 sp, float t_min, float closest, float& t) {
    const V3 oc = mk(r.o.x - sp.x, r.o.y - sp.y, r.o.z - sp.z);
    const float half_b = dot(oc, r.d);
    const float c = dot(oc, oc) - (R2 ? sp.w : sp.w * sp.w);
    const float disc = half_b * half_b - a * c;
    if (disc > 0.0f) {
        const float sq = sqrtf(disc);
        float temp = (-half_b - sq) / a;
        if (temp <= closest && temp > t_min) { t = temp; return temp < closest ? 1 : 2; }
        temp = (-half_b + sq) / a;
        if (temp <= closest && temp > t_min) { t = temp; return temp < closest ? 1 : 2; }
    }
    return 0;
}

// One sphere of a leaf (or of the brute-force loop) in mode QM.  entry: the sphere's place as
// query_hit<MODE> resolves it; idx(entry) its index in the uploaded arrays, read only on a tie.
// Returns true when the walk is over (ANY: the first accepted root).
template <int QM, bool R2, class Idx>
ORT_FN bool query_test_sphere(const Ray& r, float a, float4 sp, int entry, float t_min, float t_max, bool& hit,
                              float& closest, int& hitEntry, Idx idx) {
    float t;
    if (QM == ORT_QM_ANY) {
        if (sphere_hit_t<R2>(r, a, sp, t_min, t_max, t)) {
            hit = true;
            closest = t;
            hitEntry = entry;
            return true;
        }
        return false;
    }
    const int code = sphere_hit_q<R2>(r, a, sp, t_min, closest, t);
    if (code == 1 || (code == 2 && hit && idx(entry) < idx(hitEntry))) {
        hit = true;
        closest = t;
        hitEntry = entry;
    }
    return false;
}

// The compact layout's walk in mode QM: traverse_compact's frames and masks, with
//   - every box test under the zero-axis rule (slab_q), the root's included;
//   - a child kept when its box is hit, its exit is not before the ray's t_min and its entry not
//     beyond closest -- the current one, which NEAREST shrinks;
//   - a leaf's spheres tested against the ray's (t_min, closest);
//   - no early exit in NEAREST; ANY returns on the first accepted root;
//   - at the pop, a child pushed before closest shrank is skipped when its entry now exceeds it.
// As a state and a step of one node (mode_walk_begin / mode_walk_step), so that the persistent
// kernel can refill a lane whose ray is done; traverse_compact_q runs the same steps to the end.
struct ModeWalk {
    Ray r;
    V3 inv;
    float a, t_min, t_max, closest;
    uint32_t ocode, cx, cy, cz;
    int node, depth, hitEntry;
    bool hit;
    LevelMasks masks;
};

// False: the ray misses the root box (nothing to walk, a miss).
ORT_FN bool mode_walk_begin(const KScene& S, const float* planes, const Ray& r, float t_min, float t_max, ModeWalk& w) {
    const int D = S.depth;
    const int S1 = fast_axis_floats(D);
    const float* PX = planes;
    const float* PY = planes + S1;
    const float* PZ = planes + 2 * S1;
    w.r = r;
    w.inv = mk(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
    w.a = dot(r.d, r.d);
    w.t_min = t_min;
    w.t_max = t_max;
    w.closest = t_max;
    w.ocode = order_code(r.d);
    w.cx = w.cy = w.cz = 0;
    w.node = 0;
    w.depth = 0;
    w.hitEntry = -1;
    w.hit = false;
    w.masks.clear();
    float t0, t1;
    return ray_box_q(r, w.inv, mk(PX[0], PY[0], PZ[0]), mk(PX[1 << D], PY[1 << D], PZ[1 << D]), t0, t1);
}

// One node: an internal node pushes its surviving children, a leaf tests its spheres; then the
// pop.  True: the walk is over (w.hit, w.closest, w.hitEntry hold the result).
template <int QM, class Frames>
ORT_FN bool mode_walk_step(const KScene& S, const float* planes, ModeWalk& w, Frames& fr) {
    const int D = S.depth;
    const int S1 = fast_axis_floats(D);
    const float* PX = planes;
    const float* PY = planes + S1;
    const float* PZ = planes + 2 * S1;
    const Ray& r = w.r;
    const V3 inv = w.inv;
    const auto idx = [&S](int e) { return S.leaf_idx[e]; };
    const uint2 rec = S.node[w.node];
    if (rec.y & ORT_INTERNAL_FLAG) {
        const int co = (int)rec.x;
        const uint32_t cmask = rec.y & 0xffu;
        const uint32_t cx = w.cx, cy = w.cy, cz = w.cz;
        const int s = D - w.depth;  // >= 1 for an internal node
        const float px0 = PX[cx << s], px1 = PX[(2 * cx + 1) << (s - 1)], px2 = PX[(cx + 1) << s];
        const float py0 = PY[cy << s], py1 = PY[(2 * cy + 1) << (s - 1)], py2 = PY[(cy + 1) << s];
        const float pz0 = PZ[cz << s], pz1 = PZ[(2 * cz + 1) << (s - 1)], pz2 = PZ[(cz + 1) << s];
        float xa0, xa1, xb0, xb1, ya0, ya1, yb0, yb1, za0, za1, zb0, zb1;
        slab_q(r.d.x, inv.x, r.o.x, px0, px1, xa0, xa1);
        slab_q(r.d.x, inv.x, r.o.x, px1, px2, xb0, xb1);
        slab_q(r.d.y, inv.y, r.o.y, py0, py1, ya0, ya1);
        slab_q(r.d.y, inv.y, r.o.y, py1, py2, yb0, yb1);
        slab_q(r.d.z, inv.z, r.o.z, pz0, pz1, za0, za1);
        slab_q(r.d.z, inv.z, r.o.z, pz1, pz2, zb0, zb1);
        uint32_t rmask = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int oct = (int)((w.ocode >> (3 * k)) & 7u);
            if ((cmask >> oct) & 1u) {
                const bool xh = (oct >> 1) & 1, yh = oct & 1, zh = (oct >> 2) & 1;
                const float cmin = ort_maxf(ort_maxf(xh ? xb0 : xa0, yh ? yb0 : ya0), zh ? zb0 : za0);
                const float cmax = ort_minf(ort_minf(xh ? xb1 : xa1, yh ? yb1 : ya1), zh ? zb1 : za1);
                const bool keep = (cmax >= cmin) && !(cmax < w.t_min) && !(cmin > w.closest);
                if (keep) rmask |= 1u << k;
            }
        }
        if (rmask) {
            w.masks.put(w.depth, rmask);
            fr.setCo(w.depth, co);
        }
    } else {
        const int off = (int)rec.x;
        const int n = (int)rec.y;
        for (int i = 0; i < n; ++i) {
            const float4 sp = S.leaf_sph[off + i];  // leaf_sph: .w = r^2
            if (query_test_sphere<QM, true>(r, w.a, sp, off + i, w.t_min, w.t_max, w.hit, w.closest, w.hitEntry, idx))
                return true;
        }
    }
    for (;;) {
        const int L = w.masks.top();
        if (L < 0) return true;
        const int rk = w.masks.pop(L);
        const int oct = (int)((w.ocode >> (3 * rk)) & 7u);
        const int sh = w.depth - L;  // the current node is at `depth`; its ancestor at level L
        w.cx = ((w.cx >> sh) << 1) | (uint32_t)((oct >> 1) & 1);
        w.cy = ((w.cy >> sh) << 1) | (uint32_t)(oct & 1);
        w.cz = ((w.cz >> sh) << 1) | (uint32_t)((oct >> 2) & 1);
        w.depth = L + 1;
        w.node = fr.getCo(L) + oct;
        if (QM != ORT_QM_NEAREST || !w.hit) return false;
        // pushed under an earlier closest: the child's entry again, against the current one
        const int s = D - w.depth;
        float xl, xu, yl, yu, zl, zu;
        slab_q(r.d.x, inv.x, r.o.x, PX[w.cx << s], PX[(w.cx + 1) << s], xl, xu);
        slab_q(r.d.y, inv.y, r.o.y, PY[w.cy << s], PY[(w.cy + 1) << s], yl, yu);
        slab_q(r.d.z, inv.z, r.o.z, PZ[w.cz << s], PZ[(w.cz + 1) << s], zl, zu);
        if (!(ort_maxf(ort_maxf(xl, yl), zl) > w.closest)) return false;
    }
}

template <int QM, class Frames>
ORT_FN bool traverse_compact_q(const KScene& S, const float* planes, const Ray& r, float t_min, float t_max,
                               int& hitEntry, float& hitT, Frames& fr) {
    ModeWalk w;
    if (!mode_walk_begin(S, planes, r, t_min, t_max, w)) return false;
    while (!mode_walk_step<QM>(S, planes, w, fr)) {
    }
    hitEntry = w.hitEntry;
    hitT = w.closest;
    return w.hit;
}

// The explicit layout's stack walk in mode QM, by the same rules (boxes read from memory; the
// stack keeps a child's entry for the test at the pop).  As in traverse_explicit a push beyond
// ORT_MAX_STACK entries is dropped and the loop is bounded against a cyclic upload.
template <int QM>
ORT_FN bool traverse_explicit_q(const KScene& S, const Ray& r, float t_min, float t_max, int& hitEntry, float& hitT,
                                int* stack_node, float* stack_tmin) {
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
        if (!ray_box_q(r, inv, mk(A.x, A.y, A.z), mk(B.x, B.y, B.z), t0, t1)) return false;
    }
    const uint32_t ocode = order_code(r.d);
    const auto idx = [&S](int e) { return S.indices[e]; };
    for (long long guard = 0; sp >= 0 && guard < (1ll << 26); ++guard) {
        const int nodeIdx = stack_node[sp];
        const float entry_t = stack_tmin[sp];
        --sp;
        if (entry_t > closest) continue;  // pushed before closest shrank
        const float4 A = S.nodeA[nodeIdx], B = S.nodeB[nodeIdx];
        const int co = f2i(A.w);
        const int oo = f2i(B.w);
        if (co == -1) {
            const int objectCount = S.count[nodeIdx];
            for (int i = 0; i < objectCount; ++i) {
                const int e = oo + i;
                const float4 spr = S.sph_cr[S.indices[e]];
                if (query_test_sphere<QM, false>(r, a, spr, e, t_min, t_max, hit, closest, hitEntry, idx)) {
                    hitT = closest;
                    return true;
                }
            }
        } else {
            for (int i = 7; i >= 0; --i) {
                const int oct = (int)((ocode >> (3 * i)) & 7u);
                const int childIdx = co + oct;
                if (childIdx >= S.n_nodes) continue;
                const float4 CA = S.nodeA[childIdx], CB = S.nodeB[childIdx];
                float cmin, cmax;
                const bool boxhit = ray_box_q(r, inv, mk(CA.x, CA.y, CA.z), mk(CB.x, CB.y, CB.z), cmin, cmax);
                if (!boxhit || cmax < t_min || cmin > closest || (f2i(CA.w) == -1 && f2i(CB.w) == -1)) continue;
                if (sp < ORT_MAX_STACK - 1) {
                    ++sp;
                    stack_node[sp] = childIdx;
                    stack_tmin[sp] = cmin;
                }
            }
        }
    }
    hitT = closest;
    return hit;
}

// Brute force in mode QM: bruteForceIntersect with the ray's interval; spheres in index order and
// a strict <, so the lowest index among equals stays; ANY leaves at the first accepted root.
template <int QM>
ORT_FN bool traverse_brute_q(const KScene& S, const Ray& r, float t_min, float t_max, int& hitSphere, float& hitT) {
    const float a = dot(r.d, r.d);
    bool hit = false;
    float closest = t_max;
    const auto idx = [](int e) { return e; };
    for (int i = 0; i < S.n_spheres; ++i)
        if (query_test_sphere<QM, false>(r, a, S.sph_cr[i], i, t_min, t_max, hit, closest, hitSphere, idx)) break;
    hitT = closest;
    return hit;
}

// One query of mode QM (ORT_QM_*), whole: the interval rule, the walk by MODE (0 compact, 1
// explicit, 2 brute force) and the record.  The query-mode kernels and the host emulation
// (ort_debug_query_rays_ex) call this.
template <int MODE, int QM, class Frames>
ORT_FN RayHit query_ray_mode(const KScene& S, const float* planes, const Ray& r, float t_min, float t_max, Frames& fr,
                             int* snode, float* stmin, bool want_normal) {
    float t = 0.0f;
    int entry = -1;
    bool hit = false;
    if (query_interval(t_min, t_max)) {
        if (MODE == 0) hit = traverse_compact_q<QM>(S, planes, r, t_min, t_max, entry, t, fr);
        else if (MODE == 1) hit = traverse_explicit_q<QM>(S, r, t_min, t_max, entry, t, snode, stmin);
        else hit = traverse_brute_q<QM>(S, r, t_min, t_max, entry, t);
    }
    return query_hit<MODE>(S, r, hit, t, entry, want_normal);
}
}  // namespace ort
