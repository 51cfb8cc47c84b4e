// Piece of render_core.h, not to be included alone: the fast walk's level masks (Masks*) and per-lane state (FastStateT).
namespace ort {
// Rank-reversed level masks (see render_fast_math.inc).  pop() returns hb = 8L + 7 - rank.
struct Masks64 {  // levels 0..7: trees of depth <= 8
    static constexpr bool kLdsScene = false;  // records / leaf spheres from global memory
    // test the leaf children of a LEAFKIDS node inline (fast_step); pays for its registers on
    // depth <= 8 trees (all leaves at the bottom level with maxSpheresPerNode 0), not deeper
    static constexpr bool kInlineLeaves = true;
    static constexpr bool kRevPlanes = true;  // depth <= 8: reversed plane tables (fast_rev_planes)
    // the pop also reads the popped node's mid planes (FastStateT::tMA..), so their LDS reads
    // overlap the record load instead of following it (most pops here are internal nodes: the
    // leaves are tested inline)
    static constexpr bool kPreMid = true;
    // rejected-sphere skip (kid_table.h): off in the depth <= 8 camera-ray walk, whose inline
    // leaf children already avoid most leaf pops (C3 was 5 % slower with it); on in the bounce
    // walks and the deep camera walk (Masks96)
    static constexpr bool kKidSkip = false;
    // the pop's level arithmetic read from the image's pop tables (lds_layout) instead of
    // computed per lane and step (fast_pop); false: the ALU pop.  Needs kInlineLeaves: the tables
    // have no entries for level-D leaves.  (C3 frame 1.645 -> 1.520 ms in interleaved A/B; with
    // table 1 alone, the widths and the bit's mask still computed, it was 1.551 ms: dropped.)
    static constexpr bool kPopTable = true;
    // a leaf child's record read from KScene::leaf16 (leaf16_record): a one-sphere leaf's
    // sphere comes with it, so the sphere's own load, which nothing in the wave overlaps,
    // is gone for such a leaf (leaf_kids); false: the record from node[], every sphere from
    // leaf_sph[].  Not with the rejected-sphere skip, which wants a rejected leaf's entry.
    static constexpr bool kLeafInline = true;
    // a sphere shared by sibling leaves tested once per node: the pop's record comes from
    // KScene::cam_node, whose leaf-children nodes carry repeat masks (leaf_repeat_masks), and once
    // a member of mask A has had its trip of leaf_kids the mask's other members are dropped.
    // false: the record from node[], every surviving child tested.  C3 in interleaved A/B was
    // 1.4826 ms without, 1.4213 ms with mask A and 1.4339 ms with A and B -- B dropped a few more
    // children but cost every trip three more instructions and every leaf-children node a second
    // LUT read (profiles/leaf_dedup/ab.md) -- so the walk reads A alone; cam_node keeps B.
    static constexpr bool kLeafDedup = true;
    // the non-counting walk's child test from twelve order bits and two 64-byte order tables
    // (child_order_keep, render_lds_image.inc) instead of eight min3/max3 tests (child_drops);
    // false: child_drops everywhere
    static constexpr bool kOrderBits = true;
    uint64_t m;
    ORT_FN void clear() { m = 0; }
    ORT_FN bool empty() const { return m == 0; }
    ORT_FN void put(int L, uint32_t rev) { m |= (uint64_t)rev << (8 * L); }
    ORT_FN int pop() {
        const int hb = 63 - __builtin_clzll(m);
        m ^= (uint64_t)1 << hb;
        return hb;
    }
    // (kPopTable) pop() in two halves: the bit's index, then its mask from the table
    ORT_FN int peek() const { return 63 - __builtin_clzll(m); }
    ORT_FN void drop(uint32_t lo, uint32_t hi) { m ^= ((uint64_t)hi << 32) | lo; }
    // clears bit hb (= 8L + 7 - rank) and returns whether it was set
    ORT_FN bool take(int hb) {
        const uint64_t b = (uint64_t)1 << hb;
        const bool t = (m & b) != 0;
        m &= ~b;
        return t;
    }    // device: re-assert wave-uniformity (the value is uniform; this only helps the compiler)
    ORT_FN void uniform() {
#if defined(__HIP_DEVICE_COMPILE__)
        m = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) |
            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
#endif
    }
};
struct Masks96 {  // levels 0..9 (ORT_COMPACT_MAX_DEPTH 10)
    static constexpr bool kLdsScene = false;
    // a leaf-children node's leaves tested inline (as in the depth <= 8 walk): C5 camera rays
    // 14.11 -> 14.86 ms (the rejected-sphere skip already drops most of them): off.  (Testing
    // only a node's leading leaf children inline was dropped too: with the skip on, C5's
    // camera walk was 16.60 ms with them and 15.37 ms without, tools/ab_stream.py.)
    static constexpr bool kInlineLeaves = false;
    static constexpr bool kLeafInline = false;  // (KScene::leaf16 is built for depth <= 8 only)
    static constexpr bool kLeafDedup = false;   // (... and KScene::cam_node)
    static constexpr bool kPreMid = false;
    static constexpr bool kRevPlanes = false;
    static constexpr bool kPopTable = false;  // (the depth <= 8 image's: Masks64)
    static constexpr bool kOrderBits = false;  // (the depth <= 8 camera walk's child test: Masks64)
    // the rejected-sphere skip here too: with the kid entry loaded in the pop, C5's camera
    // walk went 17.52 -> 16.41 ms in A/B (no gain while the entry was loaded in the node's step)
    static constexpr bool kKidSkip = true;
    // levels 2..9 in lo (bits 8(L-2)..), levels 0..1 in hi: the deep levels a walk spends
    // nearly all its steps at share one word, so the put/pop branches below are taken alike
    // by almost every lane of a wave (with levels 8.. in hi, lanes split over them often)
    static constexpr int kSplit = 2;  // first level held in lo
    uint64_t lo;
    uint32_t hi;
    ORT_FN void clear() { lo = 0; hi = 0; }
    ORT_FN bool empty() const { return (lo | hi) == 0; }
    ORT_FN void put(int L, uint32_t rev) {
        if (L >= kSplit) lo |= (uint64_t)rev << (8 * (L - kSplit));
        else hi |= rev << (8 * L);
    }
    ORT_FN int pop() {
        if (lo) {
            const int hb = 63 - __builtin_clzll(lo);
            lo ^= (uint64_t)1 << hb;
            return 8 * kSplit + hb;
        }
        const int hb = 31 - __builtin_clz(hi);
        hi ^= 1u << hb;
        return hb;
    }
    ORT_FN bool take(int hb) {
        if (hb >= 8 * kSplit) {
            const uint64_t b = (uint64_t)1 << (hb - 8 * kSplit);
            const bool t = (lo & b) != 0;
            lo &= ~b;
            return t;
        }
        const uint32_t b = 1u << hb;
        const bool t = (hi & b) != 0;
        hi &= ~b;
        return t;
    }    ORT_FN void uniform() {
#if defined(__HIP_DEVICE_COMPILE__)
        lo = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(lo >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)lo);
        hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
#endif
    }
};

// Resumable per-lane state of the fast walk (so a persistent kernel can interleave rays).
// Registers are what limits the walk (7 waves/SIMD at 72 VGPRs), so nothing derivable is
// kept: the world-axis origin comes back from the role-axis one (swap = bit 1 of otab's
// nibble 0, which is m), dot(d, d) is recomputed per leaf, the half width from depth, the
// LUT row from m, and "hit" is hitEntry >= 0.
template <class Masks>
struct FastStateT {
    // what the traits rely on, for every walk type (the derived ones too)
    static_assert(!Masks::kPreMid || (Masks::kRevPlanes && Masks::kInlineLeaves), "mid planes in the pop: never a level-D leaf");
    static_assert(!Masks::kPopTable || (Masks::kRevPlanes && Masks::kInlineLeaves), "the pop table has no level-D entries");
    static_assert(!Masks::kLeafInline || (Masks::kInlineLeaves && !Masks::kKidSkip), "leaf16 records: inline leaf children, no skip");
    static_assert(!Masks::kLeafDedup || Masks::kLeafInline, "repeat masks: the leaf16 records");
    // (the order tables are device memory, not part of the reversed-plane image -- render_lds_image.inc says
    // why -- so the trait asks nothing of the image; it asks for the camera walk, whose root fast_begin handles)
    static_assert(!Masks::kOrderBits || Masks::kLeafDedup, "order bits: the depth <= 8 camera walk (fast_begin's CAM)");
    V3 d;            // original-axis direction (Sphere_hit)
    float ya;        // RN(1 / dot(d, d))
    float oA, oB, oC, iA, iB, iC;  // role-axis origin / 1/d
    // kRevPlanes: byte offsets from pl0 of the current node's near plane per role axis (table
    // start, a multiple of 4T bytes, + 4 * index; see fast_rev_planes)
    const float* pl0;
    uint32_t aA, aB, aC;
    uint32_t h4;      // half the current node's width, in bytes of plane table (4 * 2^(D-1-depth))
#if defined(__HIP_DEVICE_COMPILE__)
    // device: the offsets are absolute LDS byte addresses (the table image sits in LDS, at a
    // 1 KiB-aligned start), so a read is one ds_read with no base add -- the dynamic LDS
    // symbol's address is a link-time constant the compiler would otherwise add every time
    ORT_FN float plane(uint32_t a) const { return *(const __attribute__((address_space(3))) float*)(size_t)a; }
    static ORT_FN uint32_t table_base(const float* planes) {
        return (uint32_t)(size_t)(const __attribute__((address_space(3))) float*)planes;
    }
    // a 16-byte pop table entry (lds_layout), addressed like a plane
    ORT_FN uint4 entry(uint32_t a) const { return *(const __attribute__((address_space(3))) uint4*)(size_t)a; }
#else
    ORT_FN float plane(uint32_t off) const { return *(const float*)((const char*)pl0 + off); }
    ORT_FN uint4 entry(uint32_t off) const {
        uint4 e;
        __builtin_memcpy(&e, (const char*)pl0 + off, 16);
        return e;
    }
    static ORT_FN uint32_t table_base(const float*) { return 0u; }
#endif
    // otherwise: the ray-order plane table of each role axis, plane(i) = *(pA + sA * i bytes)
    const float* pA;
    const float* pB;
    const float* pC;
    int sA, sB, sC;   // +-4
    float tNA, tFA, tNB, tFB, tNC, tFC;  // near/far plane t of the current node's box
    float tMA, tMB, tMC;                 // (kPreMid: the depth <= 8 camera walk) its mid planes' t
    uint32_t cP;     // (not kRevPlanes) ray-order index of the current node's near plane, 10 bits per axis
    uint32_t otab;   // nibble r = octant of rank r; nibble 0 = m
    int node, depth;
    uint2 kd;        // (kKidSkip) kid entry of `node`, loaded in the pop beside rec: its latency
                     // hides behind the pop's plane reads
    uint2 rec;       // node record of `node`, loaded as soon as the pop knows it (its latency
                     // overlaps the pop's plane reads instead of opening the next step)
    float closest;   // (t_min is kFastTMin)
    int hitEntry;    // -1: no hit yet
    // the last rejected one-sphere leaf: its sphere and tmin (kid_table.h; ~0u = none)
    uint32_t kc_id;
    float kc_e;
    Masks masks;
    ORT_FN bool hit() const { return hitEntry >= 0; }
    ORT_FN float pl(const float* p, int s, int idx) const { return *at(p, s, idx); }
    // (not kRevPlanes) near planes of the current node (set by the pop): its mid plane is h steps further
    const float* nA;
    const float* nB;
    const float* nC;
    ORT_FN const float* at(const float* p, int s, int idx) const {
        return (const float*)((const char*)p + imul24(s, idx));
    }
    ORT_FN float plA(int idx) const { return pl(pA, sA, idx); }
    ORT_FN float plB(int idx) const { return pl(pB, sB, idx); }
    ORT_FN float plC(int idx) const { return pl(pC, sC, idx); }
    ORT_FN int cA() const { return (int)(cP & 1023u); }
    ORT_FN int cB() const { return (int)((cP >> 10) & 1023u); }
    ORT_FN int cC() const { return (int)(cP >> 20); }
    ORT_FN Ray ray() const {
        const bool swap = (otab >> 1) & 1u;
        Ray r;
        r.o = mk(swap ? oB : oA, swap ? oA : oB, oC);
        r.d = d;
        return r;
    }
};
using FastState = FastStateT<Masks96>;
// The persistent bounce kernel's walk at depth 9-10: the reversed plane tables (fast_rev_planes)
// there too -- the kernel runs 512-thread workgroups, whose LDS holds them at 6 waves/SIMD --
// so a lane's state across refills is the three offsets aA.., with no near-plane pointers.
struct Masks96Lean : Masks96 {
    static constexpr bool kRevPlanes = true;
};
// Depth <= 8 walk without the inline leaf children: the persistent bounce kernel's walk
// (inline leaves pay off on coherent camera rays, not on scattered bounce rays).
struct Masks64Plain : Masks64 {
    static constexpr bool kInlineLeaves = false;
    static constexpr bool kLeafInline = false;
    static constexpr bool kLeafDedup = false;
    static constexpr bool kPopTable = false;  // pops level-D leaves, which the table does not hold
    static constexpr bool kPreMid = false;
    static constexpr bool kOrderBits = false;
    static constexpr bool kKidSkip = true;
};
// ... reading node records and leaf spheres from the workgroup's LDS copies of nk[] / leaf_sph[]
// (KScene::lds_nk / lds_sph): whole-pixel paths on scenes that fit (ort_pixel_paths)
struct Masks64PlainLds : Masks64Plain {
    static constexpr bool kLdsScene = true;
};

// The split walk's level masks (traverse_split): no leaf children tested inline (the lanes
// must pop every level-`level` node themselves, to count it) and no rejected-sphere skip (each
// lane's skip state depends on the subtrees it walked, and a skipped level-`level` leaf would
// shift that lane's subtree count against the others').
struct Masks64Split : Masks64Plain {
    static constexpr bool kKidSkip = false;
};
struct Masks96Split : Masks96 {
    static constexpr bool kKidSkip = false;
};
}  // namespace ort
