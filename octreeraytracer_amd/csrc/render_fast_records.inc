// Piece of render_core.h, not to be included alone: the fast walk's record fetchers and the leaf16 / cam_node records.
namespace ort {
// Node record / leaf sphere loads of the fast walk.  On the device: buffer loads with a
// 32-bit byte offset (descriptor from the kernel arguments, so it stays in SGPRs) instead of
// 64-bit flat addresses -- fewer VALU ops and VGPRs per fetch (cdna_hip_programming.md T8).
ORT_FN uint2 fetch_node(const KScene& S, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.node, 0, (int)S.node_bytes, 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (uint32_t)i * 8u, 0, 0);
    return make_uint2(v[0], v[1]);
#else
    return S.node[i];
#endif
}
ORT_FN uint2 fetch_kid(const KScene& S, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.kid, 0, (int)S.node_bytes, 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (uint32_t)i * 8u, 0, 0);
    return make_uint2(v[0], v[1]);
#else
    return S.kid[i];
#endif
}
ORT_FN uint4 fetch_nk(const KScene& S, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.nk, 0, (int)S.nk_bytes, 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)i * 16u, 0, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
#else
    return S.nk[i];
#endif
}
ORT_FN float4 fetch_sphere(const KScene& S, int e) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.leaf_sph, 0, (int)S.leaf_bytes, 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)e * 16u, 0, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
#else
    return S.leaf_sph[e];
#endif
}

// The 16-byte leaf records (KScene::leaf16) of the depth <= 8 camera walk's inline leaf children
// (leaf_kids): one per node id, derived once per scene from node[] and leaf_sph[].
//   inline form: a leaf holding exactly one sphere whose r^2 is +0 .. +inf (sign bit clear, not
//                NaN) carries that sphere's leaf_sph entry {cx, cy, cz, r^2} itself, so the
//                record's load is the sphere's;
//   list form:   every other leaf carries {objectsOffset, objectCount, 0, 0x80000000 | count}:
//                its node record, tagged by the sign bit of .w (r * r is never negative).
// rec: the node's record; sp: leaf_sph[rec.x] of a one-sphere leaf (else unused).  Internal nodes
// get the list form of their record; the walk never reads it.
constexpr uint32_t kLeaf16ListTag = 0x80000000u;
// hitEntry of a hit in an inline-form leaf while the walk runs: the leaf's node id with this
// bit (16-byte records under the buffer loads' 4 GiB: ids and entries stay below 2^28);
// traverse_fast_t turns it into the leaf's entry, node[id].x, after the walk
constexpr int kLeafIdFlag = 0x40000000;
ORT_FN bool leaf16_is_inline(uint2 rec, uint4 sp) {
    return rec.y == 1u && (sp.w & 0x7fffffffu) <= 0x7f800000u && !(sp.w >> 31);
}
ORT_FN uint4 leaf16_record(uint2 rec, uint4 sp) {
    return leaf16_is_inline(rec, sp) ? sp : make_uint4(rec.x, rec.y, 0u, kLeaf16ListTag | rec.y);
}
ORT_FN uint4 fetch_leaf16(const KScene& S, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    // the array's true size in the descriptor: an index outside it reads zeros, not memory
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.leaf16, 0, (int)S.leaf16_bytes, 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)i * 16u, 0, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
#else
    return S.leaf16[i];
#endif
}

// The repeat masks of a leaf-children node (Masks64::kLeafDedup, leaf_kids): very often two or
// three sibling one-sphere leaves carry the very same sphere, and a ray that has rejected it in one
// of them need not test it in the others (the proof stands at leaf_kids).  k: the leaf16 records of
// the node's eight children; cm: its child mask.  Returns A | B << 8, octant masks: A the largest
// set of at least two existing children whose records are inline-form and equal in all four words,
// B the next largest; equal sizes go to the set holding the lowest octant; 0 where there is none.
ORT_FN uint32_t leaf_repeat_masks(const uint4* k, uint32_t cm) {
    uint32_t A = 0, B = 0, seen = 0;
    int nA = 0, nB = 0;
    for (int o = 0; o < 8; ++o) {
        if (!((cm >> o) & 1u) || ((seen >> o) & 1u) || (k[o].w >> 31)) continue;
        uint32_t g = 1u << o;
        int n = 1;
        for (int p = o + 1; p < 8; ++p) {
            const bool same = k[p].x == k[o].x && k[p].y == k[o].y && k[p].z == k[o].z && k[p].w == k[o].w;
            if (((cm >> p) & 1u) && same) {
                g |= 1u << p;
                n += 1;
            }
        }
        seen |= g;
        if (n < 2) continue;
        if (n > nA) {  // (sets come in the order of their lowest octant: a later one wins only if larger)
            B = A;
            nB = nA;
            A = g;
            nA = n;
        } else if (n > nB) {
            B = g;
            nB = n;
        }
    }
    return A | (B << 8);
}
// The camera walk's record of node i (KScene::cam_node): node[i], except that a leaf-children
// node whose eight children all lie inside the tree (co + 8 <= n_nodes) carries its repeat masks:
// A in bits 8-15 of .y -- which in node[] repeat the child mask (every existing child is a leaf) and
// which the inline-leaves walk never reads -- and B in bits 16-23; a leaf-children node whose
// children run past the tree carries none (both 0).  ab: leaf_repeat_masks of the node.
constexpr uint32_t kCamMaskBits = 0x00ffff00u;
ORT_FN bool cam_has_masks(uint2 rec, int64_t n_nodes) {
    return (rec.y & ORT_INTERNAL_FLAG) && (rec.y & ORT_LEAFKIDS_FLAG) && (int64_t)rec.x + 8 <= n_nodes;
}
ORT_FN uint2 cam_record(uint2 rec, uint32_t ab) {
    const bool lk = (rec.y & ORT_INTERNAL_FLAG) && (rec.y & ORT_LEAFKIDS_FLAG);
    return lk ? make_uint2(rec.x, (rec.y & ~kCamMaskBits) | (ab << 8)) : rec;
}
ORT_FN uint2 fetch_cam(const KScene& S, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    // the array's true size in the descriptor: an index outside it reads zeros, not memory
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.cam_node, 0, (int)S.cam_bytes, 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (uint32_t)i * 8u, 0, 0);
    return make_uint2(v[0], v[1]);
#else
    return S.cam_node[i];
#endif
}
}  // namespace ort
