// Piece of render_core.h, not to be included alone: vectors, KScene, Counters, order codes, slab, box and exact sphere tests.
namespace ort {
struct V3 {
    float x, y, z;
};
ORT_FN int f2i(float f) { int i; __builtin_memcpy(&i, &f, 4); return i; }
ORT_FN uint32_t f2u(float f) { uint32_t i; __builtin_memcpy(&i, &f, 4); return i; }
ORT_FN float u2f(uint32_t i) { float f; __builtin_memcpy(&f, &i, 4); return f; }
ORT_FN V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
ORT_FN V3 add(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
ORT_FN V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
ORT_FN V3 mul(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
ORT_FN V3 scl(float s, V3 a) { return mk(s * a.x, s * a.y, s * a.z); }
ORT_FN float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
ORT_FN V3 normalize(V3 v) {
    const float s = 1.0f / sqrtf(dot(v, v));
    return mk(v.x * s, v.y * s, v.z * s);
}
ORT_FN float length(V3 v) { return sqrtf(dot(v, v)); }
ORT_FN V3 cross(V3 a, V3 b) { return mk(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }
// GLSL reflect(I, N) = I - 2.0 * dot(N, I) * N
ORT_FN V3 reflect(V3 I, V3 N) {
    const float k = 2.0f * dot(N, I);
    return mk(I.x - k * N.x, I.y - k * N.y, I.z - k * N.z);
}

struct KCamera {
    V3 origin, lowerLeft, horizontal, vertical, u, v, w;
    float lensRadius;
};

struct Ray {
    V3 o, d;
};

// Device view of an uploaded scene (pointers into one context's buffers).
struct KScene {
    const float4* sph_cr;    // center.xyz, radius          (binding 0)
    const float4* sph_ma;    // float(material), albedo     (binding 1)
    const float2* sph_fr;    // fuzz, refraction index      (binding 2 .xy)
    int n_spheres;
    int n_nodes;
    // compact layout
    const uint2* node;       // internal: {childrenOffset, FLAG|childMask}; leaf: {objectsOffset, objectCount}
    const float4* leaf_sph;  // per objectIndices entry: the sphere's center.xyz, radius^2 (as float r*r)
    const int* leaf_idx;     // per entry: sphere index (= objectIndices)
    const float* planes;     // 3 x (2^depth + 1) split-plane coordinates (global copy)
    const uint4* lds_img;    // the workgroup LDS image (fast plane tables | rank LUT), built once
    int lds_img_n16;         // per scene; its size in 16-byte chunks (planes part: lds_img_p16)
    int lds_img_p16;
    const uint4* lds_rev;    // depth 9-10: the reversed-table image (fast_rev_planes), lds_rev_n16 chunks
    int lds_rev_n16;
    int depth;               // tree depth D (root = 0)
    uint32_t node_bytes;     // buffer sizes for the range-checked buffer loads (< 2^32)
    uint32_t leaf_bytes;
    const uint2* kid;        // per node: rejected-sphere skip entry (kid_table.h), or null (off)
    const uint4* nk;         // per node: {record, kid entry} interleaved (one 16-byte load), or null
    uint32_t nk_bytes;
    uint32_t tail_base;      // = n_indices: a one-sphere leaf's objectsOffset is tail_base + sphere
    const uint4* leaf16;     // depth <= 8: per node id the 16-byte leaf record (leaf16_record), or null
    uint32_t leaf16_bytes;
    uint32_t cam_bytes;
    const uint2* cam_node;   // depth <= 8: node[] with the leaf-children nodes' repeat masks (cam_record), or null
    // walks with Masks::kLdsScene (ort_pixel_paths on small scenes): LDS byte addresses of
    // workgroup copies of nk[] and leaf_sph[] (set inside the kernel)
    uint32_t lds_nk, lds_sph;
    // explicit (reference) layout
    const float4* nodeA;     // min.xyz, int bits of childrenOffset (binding 3)
    const float4* nodeB;     // max.xyz, int bits of objectsOffset  (binding 4)
    const int* count;        // objectCount                         (binding 5)
    const int* indices;      // objectIndices                       (binding 6)
};

struct Counters {
    unsigned long long v[6];
};

// Sign-vector -> octant traversal order, glsl:341-447, as 8 x 3-bit codes (rank r at bits 3r).
// Index = (sx+1)*9 + (sy+1)*3 + (sz+1), s in {-1,0,1}.  (0,0,0) cannot occur for a normalised
// direction; the reference leaves traversalOrder uninitialised there, we use the identity.
ORT_FN uint32_t pack_order(int a, int b, int c, int d, int e, int f, int g, int h) {
    return (uint32_t)a | ((uint32_t)b << 3) | ((uint32_t)c << 6) | ((uint32_t)d << 9) | ((uint32_t)e << 12) |
           ((uint32_t)f << 15) | ((uint32_t)g << 18) | ((uint32_t)h << 21);
}
ORT_FN uint32_t order_code(V3 d) {
    const int sx = (d.x < 0.0f) ? -1 : ((d.x > 0.0f) ? 1 : 0);
    const int sy = (d.y < 0.0f) ? -1 : ((d.y > 0.0f) ? 1 : 0);
    const int sz = (d.z < 0.0f) ? -1 : ((d.z > 0.0f) ? 1 : 0);
    const uint32_t CYAN = pack_order(0, 1, 2, 3, 4, 5, 6, 7);
    const uint32_t YELLOW = pack_order(2, 0, 3, 1, 6, 4, 7, 5);
    const uint32_t RED = pack_order(3, 1, 2, 0, 7, 5, 6, 4);
    const uint32_t DPURPLE = pack_order(1, 0, 3, 2, 5, 4, 7, 6);
    const uint32_t BLUE = pack_order(4, 5, 6, 7, 0, 1, 2, 3);
    const uint32_t PURPLE = pack_order(6, 4, 7, 5, 2, 0, 3, 1);
    const uint32_t GREEN = pack_order(7, 5, 6, 4, 3, 1, 2, 0);
    const uint32_t BLACK = pack_order(5, 4, 7, 6, 1, 0, 3, 2);
    // the if/else-if chain of glsl:352-447, in the same order
    if (sx == 1 && sy == 1 && sz == 1) return CYAN;
    if ((sx == -1 && sy == 1 && sz == 1) || (sx == -1 && sy == 1 && sz == 0) || (sx == 0 && sy == 1 && sz == 0) ||
        (sx == 0 && sy == 1 && sz == 1))
        return YELLOW;
    if ((sx == -1 && sy == -1 && sz == 1) || (sx == -1 && sy == 0 && sz == 1) || (sx == 0 && sy == 0 && sz == 1) ||
        (sx == 0 && sy == -1 && sz == 1) || (sx == -1 && sy == -1 && sz == 0) || (sx == 0 && sy == -1 && sz == 0) ||
        (sx == -1 && sy == 0 && sz == 0))
        return RED;
    if ((sx == 1 && sy == -1 && sz == 1) || (sx == 1 && sy == 0 && sz == 1) || (sx == 1 && sy == -1 && sz == 0) ||
        (sx == 1 && sy == 0 && sz == 0))
        return DPURPLE;
    if ((sx == 1 && sy == 1 && sz == -1) || (sx == 1 && sy == 0 && sz == -1) || (sx == 0 && sy == 1 && sz == -1) ||
        (sx == 1 && sy == 1 && sz == 0))
        return BLUE;
    if (sx == -1 && sy == 1 && sz == -1) return PURPLE;
    if ((sx == -1 && sy == -1 && sz == -1) || (sx == -1 && sy == 0 && sz == -1) || (sx == 0 && sy == -1 && sz == -1) ||
        (sx == 0 && sy == 0 && sz == -1))
        return GREEN;
    if (sx == 1 && sy == -1 && sz == -1) return BLACK;
    return CYAN;
}

// rayBoxIntersection (glsl:276-288) on one axis: GLSL min/max semantics, bot/top order kept.
ORT_FN void slab(float tbot, float ttop, float& tmin, float& tmax) {
    tmin = ort_minf(tbot, ttop);
    tmax = ort_maxf(tbot, ttop);
}
ORT_FN bool ray_box(const Ray& r, V3 inv, V3 bmin, V3 bmax, float& tmin, float& tmax) {
    const float bx = inv.x * (bmin.x - r.o.x), by = inv.y * (bmin.y - r.o.y), bz = inv.z * (bmin.z - r.o.z);
    const float ux = inv.x * (bmax.x - r.o.x), uy = inv.y * (bmax.y - r.o.y), uz = inv.z * (bmax.z - r.o.z);
    float x0, x1, y0, y1, z0, z1;
    slab(bx, ux, x0, x1);
    slab(by, uy, y0, y1);
    slab(bz, uz, z0, z1);
    tmin = ort_maxf(ort_maxf(x0, y0), z0);
    tmax = ort_minf(ort_minf(x1, y1), z1);
    return tmax >= tmin;
}

// Sphere_hit (glsl:224-273) returning only the accepted t; a = dot(d,d) precomputed.
// R2: sp.w already holds radius * radius (the compact layout's leaf_sph), else the radius.
template <bool R2 = false>
ORT_FN bool sphere_hit_t(const Ray& r, float a, float4 sp, float t_min, float t_max, float& t) {
    const V3 oc = mk(r.o.x - sp.x, r.o.y - sp.y, r.o.z - sp.z);
    const float half_b = dot(oc, r.d);
    const float c = dot(oc, oc) - (R2 ? sp.w : sp.w * sp.w);
    const float disc = half_b * half_b - a * c;
    if (disc > 0.0f) {
        const float sq = sqrtf(disc);
        float temp = (-half_b - sq) / a;
        if (temp < t_max && temp > t_min) { t = temp; return true; }
        temp = (-half_b + sq) / a;
        if (temp < t_max && temp > t_min) { t = temp; return true; }
    }
    return false;
}
}  // namespace ort
