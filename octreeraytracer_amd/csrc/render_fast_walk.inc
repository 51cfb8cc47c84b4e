// Piece of render_core.h, not to be included alone: the fast walk -- fast_begin .. fast_pop, traverse_fast_t, traverse_split.
namespace ort {
#if defined(__HIP_DEVICE_COMPILE__)
ORT_FN uint4 lds_u4(uint32_t a) { return *(const __attribute__((address_space(3))) uint4*)(size_t)a; }
#endif
// Node i's record into st.rec and, with kid (the rejected-sphere skip), its kid entry into
// st.kd: both from the interleaved copy S.nk in one 16-byte load when the context built it
// (build_nk), else from the two arrays.
// CAM (Masks::kLeafDedup, the non-counting walk): the record from S.cam_node, with the repeat masks.
template <bool CAM = false, class Masks>
ORT_FN void fetch_rec(const KScene& S, int i, bool kid, FastStateT<Masks>& st) {
    if constexpr (CAM) {
        static_assert(!Masks::kKidSkip && !Masks::kLdsScene, "cam_node: the depth <= 8 camera walk, no kid entries");
        st.rec = fetch_cam(S, i);
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (Masks::kLdsScene) {  // the workgroup's copy of nk[] (ort_pixel_paths)
        const uint4 v = lds_u4(S.lds_nk + 16u * (uint32_t)i);
        st.rec = make_uint2(v.x, v.y);
        st.kd = make_uint2(v.z, v.w);
        return;
    }
#endif
    if (Masks::kKidSkip && kid && S.nk) {
        const uint4 v = fetch_nk(S, i);
        st.rec = make_uint2(v.x, v.y);
        st.kd = make_uint2(v.z, v.w);
        return;
    }
    st.rec = fetch_node(S, i);
    if (kid) st.kd = fetch_kid(S, i);
}

#if ORT_ANALYSIS
// analysis library, host walks only
// (ort_debug_child_order) internal-node visits of the host's order-bit walks (Masks::kOrderBits):
// {visits, those breaking tN <= tM <= tF on A or B or nN <= nF or cN <= cF, those below the root
// with X < E, those where child_order_keep and child_drops keep different children, internal roots
// whose premise X >= E failed under the folds (fast_begin)}
inline unsigned long long g_order_visits[5];
#endif

// Root test and state setup (glsl:296-311).  Returns false when the root box is missed.
// CAM: the root's record from KScene::cam_node (fetch_rec) -- by default where the walk has repeat
// masks (Masks::kLeafDedup); 0 for a counting walk, which reads node[] throughout.
template <int CAM = -1, class Masks>
ORT_FN bool fast_begin(const KScene& S, const float* planes, const uint8_t* rank_lut, const Ray& r, V3 inv, float t_min,
                       float t_max, FastStateT<Masks>& st) {
    const int D = S.depth;
    const int top = 1 << D;
    // the signs of 1/d (= of d, except on zero axes, where fast_zero_axes chose them)
    const uint32_t nx = f2u(inv.x) >> 31, ny = f2u(inv.y) >> 31, nz = f2u(inv.z) >> 31;
    const uint32_t m = (nz << 2) | (nx << 1) | ny;
    const bool swap = nx != 0;
    const uint32_t gA = swap ? ny : nx, gB = swap ? nx : ny, gC = nz;
    st.d = r.d;
    st.ya = 1.0f / dot(r.d, r.d);
    st.oA = swap ? r.o.y : r.o.x;
    st.oB = swap ? r.o.x : r.o.y;
    st.oC = r.o.z;
    st.iA = swap ? inv.y : inv.x;
    st.iB = swap ? inv.x : inv.y;
    st.iC = inv.z;
    // nibble k = rank_perm(k, m): the identity (or, swap, bits 0/1 exchanged) XOR m per nibble
    st.otab = (swap ? 0x75643120u : 0x76543210u) ^ (m * 0x11111111u);
    // planes: fast_plane_floats(D) floats (fill_fast_planes)
    if (Masks::kRevPlanes) {  // per axis: forward table, reversed one T floats further
        st.pl0 = planes;
        const uint32_t b0 = FastStateT<Masks>::table_base(planes);  // 4T-byte-aligned (ort_kernel.hip)
        const uint32_t T = (uint32_t)fast_rev_T(D), S3 = 3u * T;
        st.aA = b0 + 4u * ((swap ? S3 : 0u) + (gA ? T : 0u));
        st.aB = b0 + 4u * ((swap ? 0u : S3) + (gB ? T : 0u));
        st.aC = b0 + 4u * (2u * S3 + (gC ? T : 0u));
        st.h4 = 2u * (uint32_t)top;
        const uint32_t t4 = 4u * (uint32_t)top;
        st.tNA = st.iA * (st.plane(st.aA) - st.oA);
        st.tFA = st.iA * (st.plane(st.aA + t4) - st.oA);
        st.tNB = st.iB * (st.plane(st.aB) - st.oB);
        st.tFB = st.iB * (st.plane(st.aB + t4) - st.oB);
        st.tNC = st.iC * (st.plane(st.aC) - st.oC);
        st.tFC = st.iC * (st.plane(st.aC + t4) - st.oC);
        if (Masks::kPreMid) {
            const uint32_t hm = st.h4 & ~3u;  // (a depth-0 root is a leaf: 2 bytes, unused)
            st.tMA = st.iA * (st.plane(st.aA + hm) - st.oA);
            st.tMB = st.iB * (st.plane(st.aB + hm) - st.oB);
            st.tMC = st.iC * (st.plane(st.aC + hm) - st.oC);
        }
    } else {
        const int S1 = fast_axis_floats(D);
        st.pA = planes + (swap ? S1 : 0) + (gA ? top : 0);
        st.pB = planes + (swap ? 0 : S1) + (gB ? top : 0);
        st.pC = planes + 2 * S1 + (gC ? top : 0);
        st.sA = gA ? -4 : 4;
        st.sB = gB ? -4 : 4;
        st.sC = gC ? -4 : 4;
        st.tNA = st.iA * (st.plA(0) - st.oA);
        st.tFA = st.iA * (st.plA(top) - st.oA);
        st.tNB = st.iB * (st.plB(0) - st.oB);
        st.tFB = st.iB * (st.plB(top) - st.oB);
        st.tNC = st.iC * (st.plC(0) - st.oC);
        st.tFC = st.iC * (st.plC(top) - st.oC);
        st.cP = 0;
        st.nA = st.pA;
        st.nB = st.pB;
        st.nC = st.pC;
    }
    st.node = 0;
    fetch_rec<(CAM < 0 ? Masks::kLeafDedup : CAM != 0)>(S, 0, Masks::kKidSkip && S.kid, st);
    st.depth = 0;
    st.closest = t_max;
    st.hitEntry = -1;
    st.kc_id = ~0u;
    st.kc_e = 0.0f;
    st.masks.clear();
    if constexpr (Masks::kOrderBits && (CAM < 0 ? Masks::kLeafDedup : CAM != 0)) {
        // The order-bit child test (child_order_keep) stands on X >= E under the folds, which the
        // test below, without them, does not give the root (a box behind t_min, or beyond t_max).
        // The premise is a condition of the root's visit: where it fails child_drops keeps no
        // child -- every child's entry is >= E > X >= its exit -- so an internal root loses its
        // child mask here, once per ray, and its visit keeps none either.
        const float E = fmax3(st.tNA, st.tNB, fmax_tmin(st.tNC)), X = fmin3(st.tFA, st.tFB, fmin2(st.tFC, t_max));
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
        g_order_visits[4] += (st.rec.y & ORT_INTERNAL_FLAG) && !(X >= E);
#endif
        if ((st.rec.y & ORT_INTERNAL_FLAG) && !(X >= E)) st.rec.y &= ~0xffu;
    }
    return fmin3(st.tFA, st.tFB, st.tFC) >= fmax3(st.tNA, st.tNB, st.tNC);
}

#if ORT_ANALYSIS
// analysis library, host walks only (ort_debug_leaf_forms): sphere tests and accepted hits of
// the kLeafInline walk per record form: {inline tests, inline hits, list tests, list hits}
// (g_leaf_list_call: leaf_tests is running a list-form record of leaf16_tests)
inline unsigned long long g_leaf_forms[4];
// (ort_debug_leaf_dedup) leaf children of the non-counting kLeafInline walk: {tested (trips of
// leaf_kids), dropped untested by a repeat mask (Masks::kLeafDedup) on a trip that did not hit}
inline unsigned long long g_leaf_dedup[2];
inline bool g_leaf_list_call = false;
#endif

// Sphere_hit over one leaf's objects (glsl:327-338) in the range (ntmin, closest); returns
// true if one was accepted (the walk then ends after this leaf).
template <bool COUNT, class Masks>
ORT_FN bool leaf_tests(const KScene& S, FastStateT<Masks>& st, int off, int n, float ntmin, Counters& cnt) {
    const Ray r = st.ray();
    const float a = dot(r.d, r.d);  // as fast_begin computed it
    for (int i = 0; i < n; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
        float4 sp;
        if constexpr (Masks::kLdsScene) {
            const uint4 v = lds_u4(S.lds_sph + 16u * (uint32_t)(off + i));
            sp = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        } else {
            sp = fetch_sphere(S, off + i);
        }
#else
        const float4 sp = fetch_sphere(S, off + i);
#endif
        if (COUNT) cnt.v[2] += 1;
        float t;
        const bool h = sphere_hit_fast(r, a, st.ya, sp, ntmin, st.closest, t);
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
        if (g_leaf_list_call) {
            g_leaf_forms[2] += 1;
            g_leaf_forms[3] += h ? 1 : 0;
        }
#endif
        if (h) {
            st.closest = t;
            st.hitEntry = off + i;
            if (COUNT) cnt.v[3] += 1;
        }
    }
    if (!COUNT && Masks::kKidSkip) {  // a rejected one-sphere leaf: remember its sphere (kid_table.h)
        const bool rej = n == 1 && !st.hit();
        st.kc_id = rej ? (uint32_t)off - S.tail_base : st.kc_id;
        st.kc_e = rej ? ntmin : st.kc_e;
    }
    return st.hit();
}

// Drop bits of a node's eight children, rank order (rank 0 ends at bit 7: the reversed
// layout), from its per-axis slab values N (near), M (mid), F (far); t_min is folded into the
// C entries (nN, nF) and t_max into the C exits (cN, cF).  Keep child R <=> exit >= entry, with
// entry >= t_min > 0 and exit <= t_max finite, so exit - entry is never NaN and is +0 when
// equal: its sign bit is "drop" -- one v_max3 + v_min3 + v_sub + v_alignbit per child.
ORT_FN uint32_t child_drops(float tNA, float tNB, float tMA, float tMB, float tFA, float tFB, float nN, float nF,
                            float cN, float cF) {
    uint32_t drop = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    // the eight tests as ONE asm block: separate min3/max3 asm statements each made the
    // compiler's hazard recognizer put an s_nop before their consumer
    float e, x;
#define ORT_C(EA, EB, EC, XA, XB, XC)                                                         \
    "v_max3_f32 %[e], " EA ", " EB ", " EC "\n\tv_min3_f32 %[x], " XA ", " XB ", " XC "\n\t" \
    "v_sub_f32 %[x], %[x], %[e]\n\tv_alignbit_b32 %[d], %[d], %[x], 31\n\t"
    asm("v_mov_b32 %[d], 0\n\t"
        ORT_C("%[NA]", "%[NB]", "%[nN]", "%[MA]", "%[MB]", "%[cN]")  // rank 0: A near, B near, C near
        ORT_C("%[NA]", "%[MB]", "%[nN]", "%[MA]", "%[FB]", "%[cN]")  // rank 1: B far
        ORT_C("%[MA]", "%[NB]", "%[nN]", "%[FA]", "%[MB]", "%[cN]")  // rank 2: A far
        ORT_C("%[MA]", "%[MB]", "%[nN]", "%[FA]", "%[FB]", "%[cN]")  // rank 3
        ORT_C("%[NA]", "%[NB]", "%[nF]", "%[MA]", "%[MB]", "%[cF]")  // ranks 4-7: C far
        ORT_C("%[NA]", "%[MB]", "%[nF]", "%[MA]", "%[FB]", "%[cF]")
        ORT_C("%[MA]", "%[NB]", "%[nF]", "%[FA]", "%[MB]", "%[cF]")
        ORT_C("%[MA]", "%[MB]", "%[nF]", "%[FA]", "%[FB]", "%[cF]")
        : [d] "=&v"(drop), [e] "=&v"(e), [x] "=&v"(x)
        : [NA] "v"(tNA), [NB] "v"(tNB), [MA] "v"(tMA), [MB] "v"(tMB), [FA] "v"(tFA), [FB] "v"(tFB), [nN] "v"(nN),
          [nF] "v"(nF), [cN] "v"(cN), [cF] "v"(cF));
#undef ORT_C
#else
#define ORT_CHILD(EA, EB, EC, XA, XB, XC) drop = (drop << 1) | (f2u(fmin3(XA, XB, XC) - fmax3(EA, EB, EC)) >> 31);
    ORT_CHILD(tNA, tNB, nN, tMA, tMB, cN)  // rank 0: A near, B near, C near
    ORT_CHILD(tNA, tMB, nN, tMA, tFB, cN)  // rank 1: B far
    ORT_CHILD(tMA, tNB, nN, tFA, tMB, cN)  // rank 2: A far
    ORT_CHILD(tMA, tMB, nN, tFA, tFB, cN)  // rank 3
    ORT_CHILD(tNA, tNB, nF, tMA, tMB, cF)  // ranks 4-7: C far
    ORT_CHILD(tNA, tMB, nF, tMA, tFB, cF)
    ORT_CHILD(tMA, tNB, nF, tFA, tMB, cF)
    ORT_CHILD(tMA, tMB, nF, tFA, tFB, cF)
#undef ORT_CHILD
#endif
    return drop;
}

// The same test from twelve order bits (Masks::kOrderBits: the depth <= 8 camera walk's, not the
// counting kernels'): the kept ranks of the eight children, reversed layout, before the child mask.
// With E = max3(tNA, tNB, nN), the node's entry, and X = min3(tFA, tFB, cF), its exit, the eight
// min3/max3 tests of child_drops compare nothing but tMA, tMB, nF, cN with each other and with E
// and X: the twelve conditions of the order tables (render_lds_image.inc: g_order_tables), a false one killing a fixed
// set of ranks.  When X >= E, child R passes child_drops' test -- each of its nine (exit, entry)
// pairs has exit >= entry -- exactly when no false condition kills it (DESIGN.md 4.2 has the
// proof; it needs tN <= tM <= tF per axis, nN <= nF and cN <= cF, which hold because the planes
// are read in ray order, the rounding is monotone and the folds are).  X >= E holds at every
// popped node: its parent kept it by this very test on the same floats, and closest does not
// change before a hit ends the walk; the root, whose test in fast_begin has no folds, is handled
// there.  A sign bit per condition (a - b of finite floats: set exactly when a < b, +0 on a tie,
// child_drops' own rule), six to an index, the first shifted in ending at bit 5; the two table
// bytes (render_lds_image.inc: g_order_tables) ANDed.  12 x (v_sub + v_alignbit) + v_max3 + v_min3 instead of 8 x (v_max3 + v_min3 +
// v_sub + v_alignbit).
ORT_FN void child_order_index(float tNA, float tNB, float tMA, float tMB, float tFA, float tFB, float nN, float nF,
                              float cN, float cF, uint32_t& i1, uint32_t& i2) {
    const float E = fmax3(tNA, tNB, nN), X = fmin3(tFA, tFB, cF);
    uint32_t a = 0, b = 0;
#define ORT_BIT(I, P, Q) I = (I << 1) | (f2u((P) - (Q)) >> 31);
    ORT_BIT(a, tMA, E)    //  1: tMA >= E, else no A-near child
    ORT_BIT(a, tMB, E)    //  2
    ORT_BIT(a, cN, E)     //  3
    ORT_BIT(a, X, tMA)    //  4: X >= tMA, else no A-far child
    ORT_BIT(a, X, tMB)    //  5
    ORT_BIT(a, X, nF)     //  6
    ORT_BIT(b, tMA, tMB)  //  7: else none A near and B far
    ORT_BIT(b, tMB, tMA)  //  8: A far, B near
    ORT_BIT(b, tMA, nF)   //  9: A near, C far
    ORT_BIT(b, cN, tMA)   // 10: A far, C near
    ORT_BIT(b, tMB, nF)   // 11: B near, C far
    ORT_BIT(b, cN, tMB)   // 12: B far, C near
#undef ORT_BIT
    i1 = a;
    i2 = b;
}
ORT_FN uint32_t child_order_keep(float tNA, float tNB, float tMA, float tMB, float tFA, float tFB, float nN, float nF,
                                 float cN, float cF) {
#if defined(__HIP_DEVICE_COMPILE__)
    // one asm block, as child_drops is.  Each index opens with a plain shift of its first sign bit
    // (v_lshrrev: no v_mov 0) and takes five more by v_alignbit; a2 serves as scratch (X) before
    // its own six bits, e afterwards.  The two table bytes come from g_order_tables (device
    // memory: two cache lines), the second table 64 bytes behind the first.
    uint32_t a1, a2;
    float e;
#define ORT_B0(I, T, P, Q) "v_sub_f32 " T ", " P ", " Q "\n\tv_lshrrev_b32 " I ", 31, " T "\n\t"
#define ORT_B(I, T, P, Q) "v_sub_f32 " T ", " P ", " Q "\n\tv_alignbit_b32 " I ", " I ", " T ", 31\n\t"
    asm("v_max3_f32 %[e], %[NA], %[NB], %[nN]\n\t"
        ORT_B0("%[a1]", "%[a2]", "%[MA]", "%[e]")
        ORT_B("%[a1]", "%[a2]", "%[MB]", "%[e]")
        ORT_B("%[a1]", "%[a2]", "%[cN]", "%[e]")
        "v_min3_f32 %[a2], %[FA], %[FB], %[cF]\n\t"
        ORT_B("%[a1]", "%[e]", "%[a2]", "%[MA]")
        ORT_B("%[a1]", "%[e]", "%[a2]", "%[MB]")
        ORT_B("%[a1]", "%[e]", "%[a2]", "%[nF]")
        ORT_B0("%[a2]", "%[e]", "%[MA]", "%[MB]")
        ORT_B("%[a2]", "%[e]", "%[MB]", "%[MA]")
        ORT_B("%[a2]", "%[e]", "%[MA]", "%[nF]")
        ORT_B("%[a2]", "%[e]", "%[cN]", "%[MA]")
        ORT_B("%[a2]", "%[e]", "%[MB]", "%[nF]")
        ORT_B("%[a2]", "%[e]", "%[cN]", "%[MB]")
        : [a1] "=&v"(a1), [a2] "=&v"(a2), [e] "=&v"(e)
        : [NA] "v"(tNA), [NB] "v"(tNB), [MA] "v"(tMA), [MB] "v"(tMB), [FA] "v"(tFA), [FB] "v"(tFB), [nN] "v"(nN),
          [nF] "v"(nF), [cN] "v"(cN), [cF] "v"(cF));
#undef ORT_B0
#undef ORT_B
    return (uint32_t)g_order_tables.b[a1] & (uint32_t)g_order_tables.b[(size_t)a2 + 64];  // (64-bit sum: an immediate offset)
#else
    uint32_t i1, i2;
    child_order_index(tNA, tNB, tMA, tMB, tFA, tFB, nN, nF, cN, cF, i1, i2);
    return (uint32_t)kOrderTablesHost.b[i1] & (uint32_t)kOrderTablesHost.b[64u + i2];
#endif
}

// leaf_tests for the inline leaf child `kid` given its leaf16 record lr (Masks::kLeafInline; never
// with the rejected-sphere skip: FastStateT's static_assert).  An inline-form record is the leaf's
// one sphere, tested at once; a list-form one names the leaf's entries, tested by leaf_tests as
// before.  (One sphere loop for both forms, an inline record as its single trip without the load,
// was 2.8 % slower than no leaf records at all at C3: profiles/leaf_inline/ab.md.)
template <class Masks>
ORT_FN bool leaf16_tests(const KScene& S, FastStateT<Masks>& st, int kid, uint4 lr, float ntmin, Counters& cnt) {
    if (!(lr.w >> 31)) {
        const Ray r = st.ray();
        const float a = dot(r.d, r.d);  // as fast_begin computed it
        float t;
        const bool h = sphere_hit_fast(r, a, st.ya, make_float4(u2f(lr.x), u2f(lr.y), u2f(lr.z), u2f(lr.w)), ntmin,
                                       st.closest, t);
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
        g_leaf_forms[0] += 1;
        g_leaf_forms[1] += h ? 1 : 0;
#endif
        if (h) {
            st.closest = t;
            st.hitEntry = kid | kLeafIdFlag;
        }
        return st.hit();
    }
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
    g_leaf_list_call = true;
    const bool hl = leaf_tests<false>(S, st, (int)lr.x, (int)lr.y, ntmin, cnt);
    g_leaf_list_call = false;
    return hl;
#else
    return leaf_tests<false>(S, st, (int)lr.x, (int)lr.y, ntmin, cnt);
#endif
}

// The surviving leaf children (keep, rank-reversed bits) of a leaf-children node whose
// children start at co, tested in rank order -- the order the reference pops them -- each
// with the tmin the reference pushed for it (max(max3(child entries), t_min), t_min folded
// into the C entries nN / nF; max is exact, so the order does not matter).  A hit ends the
// walk after its leaf (glsl:336): no later sibling is tested.  Returns whether one hit.
// Masks::kLeafInline (not the counting kernels, which keep the reference's loads): the child's
// record comes from S.leaf16 instead of S.node (leaf16_tests).
//
// Masks::kLeafDedup: rep = the node's repeat mask A as rank bits (leaf_repeat_masks through the
// rank LUT).  The trip of a member of A drops A's other members from todo: they hold the same
// sphere, bit for bit, and need no test.
// Why that changes nothing.  Take two surviving children r < r' in rank order.  They differ on some
// axis where r is the near half and r' the far half, so exit_r <= tM <= entry_r' on that axis'
// mid-plane value tM, and entry_r <= exit_r because r survived child_drops: the ntmin of the trips
// below never decreases along the loop -- for the very floats compared here, t_min and closest
// folded into the C axis as child_drops has them.  closest does not change until a hit, and a hit
// ends the loop.  So a sphere rejected over (ntmin, closest) -- disc <= 0 or NaN, or no root inside
// the interval -- is rejected over every later (ntmin' >= ntmin, closest): dropping the later
// siblings whose inline record is the same four words changes no hit, no hitEntry and no t.  If
// the member tested hit instead, the loop is over and what is dropped does not matter.
template <bool COUNT, class Masks>
ORT_FN bool leaf_kids(const KScene& S, FastStateT<Masks>& st, int co, uint32_t keep, float tNA, float tMA, float tNB,
                      float tMB, float nN, float nF, uint32_t rep, Counters& cnt) {
    uint32_t todo = keep;
    while (todo) {
        const int hb = 31 - __builtin_clz(todo);
        todo ^= 1u << hb;
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
        int dropped = 0;  // (ort_debug_leaf_dedup: counted below unless this trip hits)
#endif
        if constexpr (!COUNT && Masks::kLeafDedup) {
            // (before the trip: its record's load covers these; a hit clears todo below anyway)
#if defined(__HIP_DEVICE_COMPILE__)
            // bitwise selects, as for the entries below: no v_cmp + v_cndmask
            uint32_t a;
            asm("v_bfe_i32 %[a], %[rep], %[hb], 1\n\tv_and_b32 %[a], %[a], %[rep]\n\t"
                "v_bfi_b32 %[t], %[a], 0, %[t]"
                : [a] "=&v"(a), [t] "+v"(todo)
                : [rep] "v"(rep), [hb] "v"(hb));
#else
            const uint32_t cut = ((rep >> hb) & 1u) ? rep : 0u;
#if ORT_ANALYSIS
            dropped = __builtin_popcount(todo & cut);
#endif
            todo &= ~cut;
#endif
        }
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
        if (!COUNT && Masks::kLeafInline) g_leaf_dedup[0] += 1;
#endif
        const uint32_t R = 7u - (uint32_t)hb;
        const int kid = co + (int)((st.otab >> (4 * R)) & 15u);
        constexpr bool kRec16 = !COUNT && Masks::kLeafInline;
        uint4 lr = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (kRec16) {
            lr = fetch_leaf16(S, kid);
        } else {
            const uint2 lrec = fetch_node(S, kid);
            lr.x = lrec.x;
            lr.y = lrec.y;
        }
        if (COUNT) cnt.v[0] += 1;
#if defined(__HIP_DEVICE_COMPILE__)
        // bitwise selects (v_bfe_i32 + v_bfi_b32) in one asm block: the compiler turns a
        // plain select into v_cmp + s_nop + v_cndmask
        float eA, eB, eC;
        {
            uint32_t m;
            asm("v_bfe_i32 %[m], %[R], 1, 1\n\tv_bfi_b32 %[a], %[m], %[MA], %[NA]\n\t"
                "v_bfe_i32 %[m], %[R], 0, 1\n\tv_bfi_b32 %[b], %[m], %[MB], %[NB]\n\t"
                "v_bfe_i32 %[m], %[R], 2, 1\n\tv_bfi_b32 %[c], %[m], %[CF], %[CN]"
                : [a] "=&v"(eA), [b] "=&v"(eB), [c] "=&v"(eC), [m] "=&v"(m)
                : [R] "v"(R), [MA] "v"(tMA), [NA] "v"(tNA), [MB] "v"(tMB), [NB] "v"(tNB), [CF] "v"(nF), [CN] "v"(nN));
        }
#else
        const float eA = (R & 2u) ? tMA : tNA, eB = (R & 1u) ? tMB : tNB, eC = (R & 4u) ? nF : nN;
#endif
        const float ntmin = fmax3(eA, eB, eC);
        bool h;
        if constexpr (kRec16) h = leaf16_tests(S, st, kid, lr, ntmin, cnt);
        else h = leaf_tests<COUNT>(S, st, (int)lr.x, (int)lr.y, ntmin, cnt);
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
        g_leaf_dedup[1] += h ? 0ull : (unsigned long long)dropped;
#endif
        todo = h ? 0u : todo;
    }
    return st.hit();
}

// Visit st.node: push its surviving children, or test its spheres.  Returns true when a hit
// ends the walk (glsl:336).
template <bool COUNT, class Masks, class Frames>
ORT_FN bool fast_visit(const KScene& S, const uint8_t* rank_lut, FastStateT<Masks>& st, Frames& fr, Counters& cnt) {
    const int D = S.depth;
    const uint2 rec = st.rec;
    if (COUNT) cnt.v[0] += 1;
    if (rec.y & ORT_INTERNAL_FLAG) {
        const int co = (int)rec.x;
        if (COUNT) {
            const long long rem = (long long)S.n_nodes - (long long)co;
            cnt.v[1] += (unsigned long long)(rem >= 8 ? 8 : (rem > 0 ? rem : 0));
        }
        // rejected-sphere skip (kid_table.h): one-sphere leaf children holding the sphere this
        // lane last rejected, at a tmin <= this node's (<= theirs), cannot end the walk; not
        // in the counting kernels, which count the reference walk's work.  The LUT maps octant
        // bits to rank bits one for one, so the skipped octants are cleared from the child mask
        // before its one LUT read (lut[c & ~s] = lut[c] & ~lut[s]), branch-free.
        uint32_t cm = rec.y & 0xffu;
        if (!COUNT && Masks::kKidSkip && S.kid) {
            const uint2 kd = st.kd;  // (loaded in the pop: fetch_rec)
            const uint32_t m = (((kd.x & 0xffffffu) == st.kc_id) ? (kd.x >> 24) : 0u) |
                               (((kd.y & 0xffffffu) == st.kc_id) ? (kd.y >> 24) : 0u);
            const float ptmin = fmax_tmin(fmax3(st.tNA, st.tNB, st.tNC));
            cm &= ~(m & (0u - (uint32_t)(st.kc_e <= ptmin)));
        }
        const uint32_t rcm = rank_lut[((st.otab & 7u) << 8) | cm];  // LUT row m
        const int h = 1 << (D - 1 - st.depth);  // half the node's width, in plane steps
        float tMA, tMB, tMC;
        if (Masks::kPreMid) {
            tMA = st.tMA;
            tMB = st.tMB;
            tMC = st.tMC;
        } else if (Masks::kRevPlanes) {
            const uint32_t h4 = st.h4;
            tMA = st.iA * (st.plane(st.aA + h4) - st.oA);
            tMB = st.iB * (st.plane(st.aB + h4) - st.oB);
            tMC = st.iC * (st.plane(st.aC + h4) - st.oC);
        } else {
            tMA = st.iA * (*st.at(st.nA, st.sA, h) - st.oA);
            tMB = st.iB * (*st.at(st.nB, st.sB, h) - st.oB);
            tMC = st.iC * (*st.at(st.nC, st.sC, h) - st.oC);
        }
        const float tNA = st.tNA, tNB = st.tNB, tNC = st.tNC, tFA = st.tFA, tFB = st.tFB, tFC = st.tFC;
        // child R enters at max3 of its axis entries (near half: tN, far half: tM) and exits at
        // min3 of its exits (tM / tF); t_min and t_max are folded into the C axis.
        const float nN = fmax_tmin(tNC), nF = fmax_tmin(tMC);
        const float cN = fmin2(tMC, st.closest), cF = fmin2(tFC, st.closest);  // closest == t_max here
        // keep child R <=> exit >= entry, with entry >= t_min > 0 and exit <= t_max finite, so
        // exit - entry is never NaN and is +0 when equal: its sign bit is "drop".  The drop
        // bits are shifted in rank order (rank 0 ends at bit 7: the reversed layout) -- one
        // v_max3 + v_min3 + v_sub + v_alignbit per child, no compare/select.
        // (Masks::kOrderBits, not the counting kernels: the same keep bits from twelve order bits
        // and two order-table bytes, child_order_keep)
        uint32_t keep;
        if constexpr (!COUNT && Masks::kOrderBits) {
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
            g_order_visits[0] += 1;
            g_order_visits[1] += !(tNA <= tMA && tMA <= tFA && tNB <= tMB && tMB <= tFB && nN <= nF && cN <= cF);
            g_order_visits[2] += st.depth > 0 && !(fmin3(tFA, tFB, cF) >= fmax3(tNA, tNB, nN));
            g_order_visits[3] += (rcm & child_order_keep(tNA, tNB, tMA, tMB, tFA, tFB, nN, nF, cN, cF)) !=
                                 (rcm & ~child_drops(tNA, tNB, tMA, tMB, tFA, tFB, nN, nF, cN, cF) & 0xffu);
#endif
            keep = rcm & child_order_keep(tNA, tNB, tMA, tMB, tFA, tFB, nN, nF, cN, cF);
        } else {
            keep = rcm & ~child_drops(tNA, tNB, tMA, tMB, tFA, tFB, nN, nF, cN, cF) & 0xffu;
        }
        if (Masks::kInlineLeaves && (rec.y & ORT_LEAFKIDS_FLAG)) {
            // Every existing child is a leaf, so the reference pops the surviving ones next,
            // consecutively in rank order (a leaf pushes nothing): test them right here.
            uint32_t rep = 0;
            if constexpr (!COUNT && Masks::kLeafDedup) {
                // repeat mask A (st.rec came from cam_node: fetch_rec) as rank bits, LUT row m
                rep = rank_lut[((st.otab & 7u) << 8) | ((rec.y >> 8) & 0xffu)];
            }
            if (leaf_kids<COUNT>(S, st, co, keep, tNA, tMA, tNB, tMB, nN, nF, rep, cnt)) return true;
        } else {
            // level depth holds nothing yet (every deeper level is empty), so both writes are
            // harmless when no child survives
            st.masks.put(st.depth, keep);
            fr.setCo(st.depth, co);
        }
    } else {
        const float ntmin = st.depth == 0 ? kFastTMin : fmax_tmin(fmax3(st.tNA, st.tNB, st.tNC));
        if (leaf_tests<COUNT>(S, st, (int)rec.x, (int)rec.y, ntmin, cnt)) return true;  // glsl:336
    }
    return false;
}

#if ORT_ANALYSIS
// analysis library, host walks only (ort_debug_pop_coverage): how often the depth <= 8 camera
// walk popped mask bit hb ([hb]) and under which direction-sign mask m ([64 + m])
inline unsigned long long g_pop_cover[72];
#endif

// Pop the next node -- the lowest remaining rank of the deepest level with one left (the masks
// must not be empty) -- and load its record and box planes.
template <bool COUNT, class Masks, class Frames>
ORT_FN void fast_pop(const KScene& S, FastStateT<Masks>& st, Frames& fr);

// One node of the walk: visit st.node (push its surviving children, or test its spheres),
// then pop the next node.  Returns true when the walk is over (hit found, or stack empty).
template <bool COUNT, class Masks, class Frames>
ORT_FN bool fast_step(const KScene& S, const uint8_t* rank_lut, FastStateT<Masks>& st, Frames& fr, Counters& cnt) {
    if (fast_visit<COUNT>(S, rank_lut, st, fr, cnt)) return true;
    if (st.masks.empty()) return true;
    fast_pop<COUNT>(S, st, fr);
    return false;
}

template <bool COUNT, class Masks, class Frames>
ORT_FN void fast_pop(const KScene& S, FastStateT<Masks>& st, Frames& fr) {
    const int D = S.depth;
    // next node: lowest remaining rank of the deepest level with one left
    int hb;
    if constexpr (Masks::kPopTable) hb = st.masks.peek();  // (the bit is cleared with the table's mask below)
    else hb = st.masks.pop();
    const int L = hb >> 3;
    const uint32_t rk = (uint32_t)(~hb) & 7u;
    const int w = 1 << (D - 1 - L);  // child width in plane steps
    st.depth = L + 1;
    st.node = fr.getCo(L) + (int)((st.otab >> (4 * rk)) & 15u);
    fetch_rec<(!COUNT && Masks::kLeafDedup)>(S, st.node, !COUNT && Masks::kKidSkip && S.kid, st);
#if ORT_ANALYSIS && !defined(__HIP_DEVICE_COMPILE__)
    if (Masks::kInlineLeaves && Masks::kRevPlanes) {  // ort_debug_pop_coverage: the camera walk's pops
        g_pop_cover[hb & 63] += 1;
        g_pop_cover[64 + (st.otab & 7u)] += 1;
    }
#endif
    if (Masks::kRevPlanes) {
        // near plane of the level-(L+1) child: the level-L ancestor's (offset bits below 8w
        // cleared; the table start is a multiple of 4T >= 8w bytes) plus w planes on the axes
        // where the child is the far half
        uint32_t w4;
        if constexpr (Masks::kPopTable) {
            // the image's pop tables (lds_layout), two 16-byte reads: m8 and the three offsets;
            // the widths and the popped bit's mask
            const uint32_t ta = FastStateT<Masks>::table_base(st.pl0) + (uint32_t)kPopTableOff + 16u * (uint32_t)hb;
            const uint4 e = st.entry(ta);
            st.aA = (st.aA & e.x) | e.y;
            st.aB = (st.aB & e.x) | e.z;
            st.aC = (st.aC & e.x) | e.w;
            const uint4 e2 = st.entry(ta + (uint32_t)kPopTable2);
            w4 = e2.x;
            st.h4 = e2.y;
            st.masks.drop(e2.z, e2.w);
        } else {
            w4 = 4u << (D - 1 - L);
            st.h4 = w4 >> 1;
            const uint32_t m8 = ~(2u * w4 - 1u);
            const uint32_t s = (uint32_t)(D + 1 - L);  // log2(w4)
            st.aA = (st.aA & m8) | (((rk >> 1) & 1u) << s);
            st.aB = (st.aB & m8) | ((rk & 1u) << s);
            st.aC = (st.aC & m8) | (((rk >> 2) & 1u) << s);
        }
        st.tNA = st.iA * (st.plane(st.aA) - st.oA);
        st.tFA = st.iA * (st.plane(st.aA + w4) - st.oA);
        st.tNB = st.iB * (st.plane(st.aB) - st.oB);
        st.tFB = st.iB * (st.plane(st.aB + w4) - st.oB);
        st.tNC = st.iC * (st.plane(st.aC) - st.oC);
        st.tFC = st.iC * (st.plane(st.aC + w4) - st.oC);
        if (Masks::kPreMid) {
            // h4 is 2 bytes (a misaligned plane offset) only for a level-D node, a leaf; the
            // kPreMid walk tests its leaves inline (kInlineLeaves), so it never pops one
            st.tMA = st.iA * (st.plane(st.aA + st.h4) - st.oA);
            st.tMB = st.iB * (st.plane(st.aB + st.h4) - st.oB);
            st.tMC = st.iC * (st.plane(st.aC + st.h4) - st.oC);
        }
    } else {
        const int keep = -2 * w;  // clears the offsets below the level-L ancestor
        {   // per 10-bit field: (c & keep) | (axis bit of rk ? w : 0)
            const uint32_t k3 = ((uint32_t)keep & 1023u) * 0x100401u;
            const uint32_t bits = ((rk >> 1) & 1u) | ((rk & 1u) << 10) | (((rk >> 2) & 1u) << 20);
            st.cP = (st.cP & k3) | bits * (uint32_t)w;
        }
        const float* nA = st.at(st.pA, st.sA, st.cA());
        const float* nB = st.at(st.pB, st.sB, st.cB());
        const float* nC = st.at(st.pC, st.sC, st.cC());
        st.nA = nA;
        st.nB = nB;
        st.nC = nC;
        st.tNA = st.iA * (nA[0] - st.oA);
        st.tFA = st.iA * (*st.at(nA, st.sA, w) - st.oA);
        st.tNB = st.iB * (nB[0] - st.oB);
        st.tFB = st.iB * (*st.at(nB, st.sB, w) - st.oB);
        st.tNC = st.iC * (nC[0] - st.oC);
        st.tFC = st.iC * (*st.at(nC, st.sC, w) - st.oC);
    }
}

template <bool COUNT, class Masks, class Frames>
ORT_FN bool traverse_fast_t(const KScene& S, const float* planes, const uint8_t* rank_lut, const Ray& r, V3 inv,
                            float t_min, float t_max, int& hitEntry, float& hitT, Frames& fr, Counters& cnt,
                            Ray* walked = nullptr, int* steps = nullptr) {
    FastStateT<Masks> st;
    const bool in = fast_begin<(!COUNT && Masks::kLeafDedup)>(S, planes, rank_lut, r, inv, t_min, t_max, st);
    int n = 0;  // walk steps (steps: the cost order's record; folds away without it)
    // (a leaf hold as in the deep bounce walk, lanes at a leaf waiting for company, cost the deep
    // camera walk 10-14 % at 8-16 lanes: the coherent camera rays reach leaves together anyway)
    if (in)
        while (!fast_step<COUNT>(S, rank_lut, st, fr, cnt)) {
            ++n;
        }
    if (steps) *steps = in ? n + 1 : 0;
    // the ray back from the walk state (bit-identical to r; no extra registers across the walk)
    if (walked) *walked = st.ray();
    if (!in) return false;
    hitEntry = st.hitEntry;
    if constexpr (!COUNT && Masks::kLeafInline) {
        // a hit in an inline-form leaf left the leaf's node id (leaf16_tests): its entry -- what
        // shading reads leaf_idx[] by -- is its record's offset, one load per hit ray
        // (a leaf's record is the same in cam_node: the walk with repeat masks reads that array alone)
        if (hitEntry >= kLeafIdFlag)
            hitEntry = (int)(Masks::kLeafDedup ? fetch_cam(S, hitEntry ^ kLeafIdFlag) : fetch_node(S, hitEntry ^ kLeafIdFlag)).x;
    }
    hitT = st.closest;
    return st.hit();
}

// Split walk (the heavy camera rays of ort_trace_split): ONE ray's walk dealt over G lanes by
// its level-`level` subtrees.  The reference DFS (glsl:312-479) walks the subtree of a node
// completely before its next sibling, so the nodes of the walk's level-`level` subtrees are
// contiguous, in DFS order, and a hit ends the walk (glsl:336): the walk's result is the first
// hit of the lowest-ordered subtree holding one, unless a leaf above that level, visited before
// it, holds one.  Lane j walks the nodes above the level and the subtrees i with i % G == j,
// popping the others without visiting them, and stops at its first hit; `pos` orders the lanes'
// hits by their place in the DFS -- 2i + 1 for a hit inside subtree i, 2c for a hit in a leaf
// above the level visited after c subtrees -- and the lowest `pos` of the G lanes is the result
// of the whole walk (bit-identical: each lane's visits are the reference walk's own).
// Returns whether this lane found a hit; steps = the nodes it visited, own = those of them inside
// its own subtrees (the rest, above the level, every lane visits up to where it stops: a single
// walk's length is about the largest `steps - own` of the lanes plus the sum of their `own`).
template <class Masks, class Frames>
ORT_FN bool traverse_split(const KScene& S, const float* planes, const uint8_t* rank_lut, const Ray& r, V3 inv,
                           int level, int G, int j, int& pos, int& hitEntry, float& hitT, Frames& fr, int& steps,
                           int& own) {
    FastStateT<Masks> st;
    Counters cnt;  // (COUNT = false: untouched)
    steps = 0;
    own = 0;
    if (!fast_begin(S, planes, rank_lut, r, inv, kFastTMin, ORT_MAXFLOAT, st)) return false;
    int sub = -1, seen = 0;  // the level-`level` subtree the walk is in; how many were popped
    for (;;) {
        ++steps;
        own += st.depth >= level ? 1 : 0;
        if (fast_visit<false>(S, rank_lut, st, fr, cnt)) {
            pos = st.depth >= level ? 2 * sub + 1 : 2 * seen;
            hitEntry = st.hitEntry;
            hitT = st.closest;
            return true;
        }
        bool more = false;
        while (!st.masks.empty()) {  // the next node, passing over other lanes' subtrees
            fast_pop<false>(S, st, fr);
            if (st.depth != level) {
                more = true;
                break;
            }
            sub = seen++;
            if (sub % G == j) {
                more = true;
                break;
            }
        }
        if (!more) return false;
    }
}

template <bool COUNT, class Frames>
ORT_FN bool traverse_fast(const KScene& S, const float* planes, const uint8_t* rank_lut, const Ray& r, V3 inv,
                          float t_min, float t_max, int& hitEntry, float& hitT, Frames& fr, Counters& cnt) {
    if (S.depth <= 8) return traverse_fast_t<COUNT, Masks64>(S, planes, rank_lut, r, inv, t_min, t_max, hitEntry, hitT, fr, cnt);
    return traverse_fast_t<COUNT, Masks96>(S, planes, rank_lut, r, inv, t_min, t_max, hitEntry, hitT, fr, cnt);
}
}  // namespace ort
