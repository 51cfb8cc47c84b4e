// host_emulation.inc -- the TEST-ONLY host emulation (ort_internal.h: ort_debug_*), included by
// ort_kernel.hip in analysis builds (ORT_ANALYSIS) only: the kernels' per-ray and per-pixel code of
// render_core.h run on the CPU, the yardstick of the CPU suite.  Host code only.  Every emulation
// walks a HostScene; the queries' emulations (ray_query.inc, camera_query.inc, ray_modes.inc) too.

namespace {

// The scene a host emulation walks, built once from the raw arrays as the upload builds the
// device's: the compact layout with the fast walks' plane tables (fplanes; fplanes_b: the bounce
// walk's, reversed at depth 9-10) and the rank LUT, or the explicit layout's node arrays, or
// nothing more for brute force; with materials (ma, fr) or without (null).  The KScene points
// into this object: it is neither copied nor moved.
struct HostScene {
    enum Check {
        kValidate = 1,      // validateScene first, whatever the mode
        kNoOctree = 2,      // a tree walk of a scene without nodes: ORT_ERR_NO_SCENE "no octree"
        kValidateTree = 4,  // validateScene for a tree walk only, after kNoOctree
        kOrdered = 8,       // an unordered tree: ORT_ERR_UNSUPPORTED "unordered tree"
    };
    ort::KScene S;
    int mode = 2;  // 0 compact, 1 explicit, 2 brute force
    ort::CompactLayout cl;
    std::vector<float> fplanes, fplanes_b;
    std::vector<uint8_t> lut;           // the rank LUT
    std::vector<uint4> leaf16;          // depth <= 8: KScene::leaf16, as k_leaf16 derives it
    std::vector<uint2> cam_node;        // depth <= 8: KScene::cam_node, as k_cam_node derives it
    const uint8_t* rank_lut = nullptr;  // ... null for an unordered tree (and without the compact layout)
    std::string error;                  // of a failed build
    HostScene() { std::memset(&S, 0, sizeof(S)); }
    HostScene(const HostScene&) = delete;
    HostScene& operator=(const HostScene&) = delete;

    // use_octree != 1: brute force.  Returns ORT_OK or the code to fail with (text in `error`).
    int build(const float* cr, const float* ma, const float* fr, int32_t n_spheres, const float* node_min, const float* node_max,
              const int32_t* co, const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
              int32_t layout, int32_t use_octree, int checks) {
        if (!ma || !fr) zeros_.assign((size_t)n_spheres * 4, 0.0f);
        const ort::SceneInput in{cr, ma ? ma : zeros_.data(), fr ? fr : zeros_.data(), n_spheres, node_min, node_max, co, oo, cnt,
                                 n_nodes, idx, n_indices};
        const bool tree = use_octree == 1;
        if (checks & kValidate) error = ort::validateScene(in);
        if (!error.empty()) return ORT_ERR_INVALID_ARG;
        if (tree && (checks & kNoOctree) && n_nodes <= 0) return error = "no octree", ORT_ERR_NO_SCENE;
        if (tree && (checks & kValidateTree)) error = ort::validateScene(in);
        if (!error.empty()) return ORT_ERR_INVALID_ARG;
        S.sph_cr = (const float4*)cr;
        if (ma && fr) {
            fr2_.resize((size_t)n_spheres * 2);
            for (int32_t i = 0; i < n_spheres; ++i) {
                fr2_[2 * (size_t)i] = fr[4 * (size_t)i];
                fr2_[2 * (size_t)i + 1] = fr[4 * (size_t)i + 1];
            }
            S.sph_ma = (const float4*)ma;
            S.sph_fr = (const float2*)fr2_.data();
        }
        S.n_spheres = n_spheres;
        S.n_nodes = n_nodes;
        lut.resize(kRankLutBytes);
        for (size_t i = 0; i < lut.size(); ++i) lut[i] = ort::rank_lut_entry((uint32_t)i >> 8, (uint32_t)i & 255u);
        if (!tree) return ORT_OK;
        if (layout == ORT_LAYOUT_COMPACT) {
            if (!ort::buildCompactLayout(in, ORT_COMPACT_MAX_DEPTH, cl, error)) return ORT_ERR_UNSUPPORTED;
            if ((checks & kOrdered) && !cl.ordered) return error = "unordered tree", ORT_ERR_UNSUPPORTED;
            mode = 0;
            S.node = (const uint2*)cl.node.data();
            S.kid = (const uint2*)cl.kid.data();
            S.tail_base = (uint32_t)in.n_indices;
            S.leaf_sph = (const float4*)cl.leaf_sph.data();
            S.leaf_idx = cl.leaf_idx.data();
            S.planes = cl.planes.data();
            S.depth = cl.depth;
            if (ort::Masks64::kLeafInline && cl.depth <= 8) {
                fill_leaf16((const uint2*)cl.node.data(), (int64_t)(cl.node.size() / 2), (const uint4*)cl.leaf_sph.data(),
                            (int64_t)(cl.leaf_sph.size() / 4), leaf16);
                S.leaf16 = leaf16.data();
                S.leaf16_bytes = (uint32_t)(16 * leaf16.size());
                if (ort::Masks64::kLeafDedup) {
                    fill_cam_node((const uint2*)cl.node.data(), leaf16, cam_node);
                    S.cam_node = cam_node.data();
                    S.cam_bytes = (uint32_t)(8 * cam_node.size());
                }
            }
            fplanes.resize(ort::fast_plane_floats(cl.depth));
            ort::fill_fast_planes(cl.planes.data(), fplanes.data(), cl.depth);
            fplanes_b.resize(ort::fast_plane_floats(cl.depth, true));  // the bounce walks': reversed at every depth
            ort::fill_fast_planes(cl.planes.data(), fplanes_b.data(), cl.depth, true);
            if (cl.ordered) rank_lut = lut.data();
            return ORT_OK;
        }
        mode = 1;
        a_.resize(4 * (size_t)n_nodes);
        b_.resize(4 * (size_t)n_nodes);
        for (int32_t i = 0; i < n_nodes; ++i) {
            for (int k = 0; k < 3; ++k) {
                a_[4 * (size_t)i + k] = node_min[3 * (size_t)i + k];
                b_[4 * (size_t)i + k] = node_max[3 * (size_t)i + k];
            }
            std::memcpy(&a_[4 * (size_t)i + 3], &co[i], 4);
            std::memcpy(&b_[4 * (size_t)i + 3], &oo[i], 4);
        }
        S.nodeA = (const float4*)a_.data();
        S.nodeB = (const float4*)b_.data();
        S.count = cnt;
        S.indices = idx;
        return ORT_OK;
    }

    // k_leaf16 on the host: the same ort::leaf16_record per node
    static void fill_leaf16(const uint2* node, int64_t n, const uint4* leaf_sph, int64_t n_ent, std::vector<uint4>& out) {
        out.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const uint2 rec = node[i];
            uint4 sp = make_uint4(0u, 0u, 0u, ort::kLeaf16ListTag);
            if (rec.y == 1u && (int64_t)rec.x < n_ent) sp = leaf_sph[rec.x];
            out[(size_t)i] = ort::leaf16_record(rec, sp);
        }
    }

    // k_cam_node on the host: the same ort::leaf_repeat_masks / ort::cam_record per node
    static void fill_cam_node(const uint2* node, const std::vector<uint4>& leaf16, std::vector<uint2>& out) {
        const int64_t n = (int64_t)leaf16.size();
        out.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const uint2 rec = node[i];
            const uint32_t ab = ort::cam_has_masks(rec, n) ? ort::leaf_repeat_masks(&leaf16[rec.x], rec.y & 0xffu) : 0u;
            out[(size_t)i] = ort::cam_record(rec, ab);
        }
    }

private:
    std::vector<float> zeros_, fr2_, a_, b_;  // absent materials; the frame pairs; the explicit layout's node arrays
};

// ort_debug_child_order mode 4: the order tables as device code reads them, one byte a thread (this file
// is part of analysis builds only: ort_kernel.hip includes it under ORT_ANALYSIS)
__global__ void k_order_tables(uint8_t* out) {
    if (threadIdx.x < sizeof(ort::OrderTables)) out[threadIdx.x] = ort::g_order_tables.b[threadIdx.x];
}

}  // namespace

extern "C" {

// ---- TEST-ONLY host emulation (see ort_internal.h) ----------------------------------
int ort_debug_trace_rays(const float* cr, int32_t n_spheres, const float* node_min, const float* node_max,
                         const int32_t* co, const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx,
                         int64_t n_indices, const float* rays, int32_t n_rays, int32_t bounce, int32_t* out) {
    try {
        HostScene hs;
        if (int rc = hs.build(cr, nullptr, nullptr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices,
                              ORT_LAYOUT_COMPACT, 1, HostScene::kValidate | HostScene::kOrdered))
            return fail(nullptr, rc, hs.error);
        const ort::KScene& S = hs.S;
        const std::vector<float>&fplanes = hs.fplanes, &fplanes_b = hs.fplanes_b;
        const std::vector<uint8_t>& lut = hs.lut;
        ort::LocalFrames lf;
        for (int32_t i = 0; i < n_rays; ++i) {
            ort::Ray r;
            r.o = ort::mk(rays[6 * (size_t)i], rays[6 * (size_t)i + 1], rays[6 * (size_t)i + 2]);
            r.d = ort::mk(rays[6 * (size_t)i + 3], rays[6 * (size_t)i + 4], rays[6 * (size_t)i + 5]);
            ort::Counters cc;
            for (int k = 0; k < 6; ++k) cc.v[k] = 0;
            float tf = 0.0f, tx = 0.0f;
            int ef = -1, ex = -1;
            // the kernels' choice: the fast walk when fast_prepare takes the ray, else deferred
            ort::V3 inv = ort::mk(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
            const bool fast = ort::fast_prepare(S, r, inv);
            if (fast) {
                if (!bounce) ort::traverse_fast<false>(S, fplanes.data(), lut.data(), r, inv, 0.001f, ORT_MAXFLOAT, ef, tf, lf, cc);
                else if (S.depth <= 8)
                    ort::traverse_fast_t<false, ort::Masks64Plain>(S, fplanes.data(), lut.data(), r, inv, 0.001f, ORT_MAXFLOAT,
                                                                 ef, tf, lf, cc);
                else
                    ort::traverse_fast_t<false, ort::Masks96Lean>(S, fplanes_b.data(), lut.data(), r, inv, 0.001f,
                                                                ORT_MAXFLOAT, ef, tf, lf, cc);
            }
            ort::traverse_compact<false>(S, fplanes.data(), r, 0.001f, ORT_MAXFLOAT, ex, tx, lf, cc);
            int32_t* o = out + 5 * (size_t)i;
            o[0] = fast ? 1 : 0;
            o[1] = ef;
            o[2] = (int32_t)ort::f2u(tf);
            o[3] = ex;
            o[4] = (int32_t)ort::f2u(tx);
        }
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

int ort_debug_split_rays(const float* cr, int32_t n_spheres, const float* node_min, const float* node_max,
                         const int32_t* co, const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx,
                         int64_t n_indices, const float* rays, int32_t n_rays, int32_t level, int32_t lanes, int32_t* out) {
    try {
        if (lanes < 1 || level < 1) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_split_rays: lanes, level >= 1");
        HostScene hs;
        if (int rc = hs.build(cr, nullptr, nullptr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices,
                              ORT_LAYOUT_COMPACT, 1, HostScene::kValidate | HostScene::kOrdered))
            return fail(nullptr, rc, hs.error);
        const ort::KScene& S = hs.S;
        const std::vector<float>& fplanes = hs.fplanes;  // the default image's layout
        const std::vector<uint8_t>& lut = hs.lut;
        ort::LocalFrames lf;
        for (int32_t i = 0; i < n_rays; ++i) {
            ort::Ray r;
            r.o = ort::mk(rays[6 * (size_t)i], rays[6 * (size_t)i + 1], rays[6 * (size_t)i + 2]);
            r.d = ort::mk(rays[6 * (size_t)i + 3], rays[6 * (size_t)i + 4], rays[6 * (size_t)i + 5]);
            const ort::V3 inv = ort::mk(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
            int32_t* o = out + 4 * (size_t)i;
            o[0] = -1;
            o[1] = 0;
            o[2] = 0x7fffffff;
            o[3] = 0;
            if (!ort::fast_path_ok(r, inv, 0.001f, ORT_MAXFLOAT)) continue;
            // the lanes of one group one after another; the lowest DFS position wins
            int best = 0x7fffffff, be = -1, top = 0, owns = 0;  // steps as ort_trace_split records them
            float bt = 0.0f;
            for (int j = 0; j < lanes; ++j) {
                int pos = 0x7fffffff, e = -1, st = 0, own = 0;
                float t = 0.0f;
                if (S.depth > 8)
                    ort::traverse_split<ort::Masks96Split>(S, fplanes.data(), lut.data(), r, inv, level, lanes, j, pos, e, t, lf, st, own);
                else
                    ort::traverse_split<ort::Masks64Split>(S, fplanes.data(), lut.data(), r, inv, level, lanes, j, pos, e, t, lf, st, own);
                top = std::max(top, st - own);
                owns += own;
                if (pos < best) {
                    best = pos;
                    be = e;
                    bt = t;
                }
            }
            o[0] = be;
            o[1] = (int32_t)ort::f2u(bt);
            o[2] = best;
            o[3] = top + owns;
        }
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

int ort_debug_pack_rgba8(const float* rgb, int64_t n_pixels, uint32_t* out) {
    if (!rgb || !out || n_pixels < 0) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_pack_rgba8: null argument");
    for (int64_t i = 0; i < n_pixels; ++i) out[i] = ort::pack_rgba8(ort::mk(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]));
    return ORT_OK;
}

int ort_debug_fast_order(int32_t m, int32_t* order8, uint8_t* lut256) {
    if (m < 0 || m > 7 || !order8) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_fast_order: m in 0..7");
    for (uint32_t r = 0; r < 8; ++r) order8[r] = (int32_t)ort::rank_perm(r, (uint32_t)m);
    if (lut256)
        for (uint32_t c = 0; c < 256; ++c) lut256[c] = ort::rank_lut_entry((uint32_t)m, c);
    return ORT_OK;
}

int ort_debug_emulate_render(const float* cr, const float* ma, const float* fr, int32_t n_spheres,
                             const float* node_min, const float* node_max, const int32_t* co, const int32_t* oo,
                             const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
                             int32_t layout, const ort_params* p, const ort_tile* t, float* out, uint64_t* counts) {
    return ort_debug_emulate_render_prefix(cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices,
                                           layout, p, t, -1, out, counts);
}

int ort_debug_emulate_render_prefix(const float* cr, const float* ma, const float* fr, int32_t n_spheres,
                                    const float* node_min, const float* node_max, const int32_t* co, const int32_t* oo,
                                    const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
                                    int32_t layout, const ort_params* p, const ort_tile* t, int32_t samples_done,
                                    float* out, uint64_t* counts) {
    try {
        const std::string bad = check_frame_tile(p, t);
        if (!bad.empty()) return fail(nullptr, ORT_ERR_INVALID_ARG, bad);
        if (samples_done >= 0 && (samples_done < 1 || samples_done > p->num_samples))
            return fail(nullptr, ORT_ERR_INVALID_ARG, "samples_done must be 1 .. num_samples");
        const int done = samples_done < 0 ? -1 : samples_done;
        HostScene hs;  // (layout 2: the compact layout without the rank LUT)
        if (int rc = hs.build(cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices,
                              layout == 2 ? ORT_LAYOUT_COMPACT : layout, p->use_octree, HostScene::kValidate | HostScene::kNoOctree))
            return fail(nullptr, rc, hs.error);
        const ort::KScene& S = hs.S;
        const std::vector<float>&fplanes = hs.fplanes, &fplanes_b = hs.fplanes_b;
        const int mode = hs.mode;
        const ort::PixelParams pp = pixel_params(p);
        const TileMap tm = {t->x0, t->width, t->y0, t->rows, t->band_height, t->band_stride};
        ort::Counters total;
        for (int k = 0; k < 6; ++k) total.v[k] = 0;
        const uint8_t* rank_lut = layout == ORT_LAYOUT_COMPACT ? hs.rank_lut : nullptr;
        std::vector<int> snode(ORT_MAX_STACK);
        std::vector<float> stmin(ORT_MAX_STACK);
        ort::LocalFrames lf;
        for (int row = 0; row < t->rows; ++row) {
            const int y = tile_row_to_y(tm, row);
            for (int c = 0; c < t->width; ++c) {
                float* o = out + 3 * ((size_t)row * t->width + c);
                if (y >= p->height) { o[0] = o[1] = o[2] = 0.0f; continue; }
                ort::Counters cc;
                for (int k = 0; k < 6; ++k) cc.v[k] = 0;
                ort::V3 v, vc;
                // pixels from the production walk (COUNT=false: with the rejected-sphere skip),
                // counters from the counting walk (the reference's work, no skip) -- and the two
                // pixels must agree bit for bit
                if (mode == 0) {
                    v = ort::shade_pixel<0, false>(pp, S, fplanes.data(), fplanes_b.data(), rank_lut, lf, nullptr, nullptr,
                                                   t->x0 + c, y, cc, done);
                    vc = ort::shade_pixel<0, true>(pp, S, fplanes.data(), fplanes_b.data(), rank_lut, lf, nullptr, nullptr,
                                                   t->x0 + c, y, cc, done);
                } else if (mode == 1) {
                    v = ort::shade_pixel<1, false>(pp, S, nullptr, nullptr, nullptr, lf, snode.data(), stmin.data(), t->x0 + c, y, cc, done);
                    vc = ort::shade_pixel<1, true>(pp, S, nullptr, nullptr, nullptr, lf, snode.data(), stmin.data(), t->x0 + c, y, cc, done);
                } else {
                    v = ort::shade_pixel<2, false>(pp, S, nullptr, nullptr, nullptr, lf, nullptr, nullptr, t->x0 + c, y, cc, done);
                    vc = ort::shade_pixel<2, true>(pp, S, nullptr, nullptr, nullptr, lf, nullptr, nullptr, t->x0 + c, y, cc, done);
                }
                if (ort::f2u(v.x) != ort::f2u(vc.x) || ort::f2u(v.y) != ort::f2u(vc.y) || ort::f2u(v.z) != ort::f2u(vc.z))
                    return fail(nullptr, ORT_ERR_INTERNAL, "emulation: production and counting walks differ at pixel (" +
                                                               std::to_string(t->x0 + c) + ", " + std::to_string(y) + ")");
                o[0] = v.x; o[1] = v.y; o[2] = v.z;
                cc.v[4] = 1;
                for (int k = 0; k < 6; ++k) total.v[k] += cc.v[k];
            }
        }
        if (counts) for (int k = 0; k < 6; ++k) counts[k] = total.v[k];
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}


// Analysis builds only (ORT_PERSIST_CLOCK, tools/persist_clock.py): the persistent bounce
// kernel records a per-wave timeline {start, queue drained, end, XCC id | items << 8} into dev
// (n records of 4 x u64, one range per launch of a frame); null = off.
int ort_debug_wave_clock(ort_ctx* ctx, void* dev, int64_t n) {
    if (!ctx) return ORT_ERR_INVALID_ARG;
    ctx->wclock = dev;
    ctx->wclock_n = dev ? n : 0;
    return ORT_OK;
}

// ANALYSIS-ONLY (tools/wave_stats.py): walks sampled 8x8 pixel blocks (one wave each) of
// the primary-ray frame with the kernel's fast walk on the host and reports how the lanes'
// visited-node sets overlap, to price wave-level (packet) traversal against the per-lane
// loop.  stats: see tools/wave_stats.py for the field order.
int ort_debug_wave_stats(const float* cr, const float* ma, const float* fr, int32_t n_spheres,
                         const float* node_min, const float* node_max, const int32_t* co, const int32_t* oo,
                         const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
                         const ort_params* p, int32_t block_step, double* stats, int32_t n_stats) {
    try {
        if (n_stats < 16 || block_step < 1) return fail(nullptr, ORT_ERR_INVALID_ARG, "bad stats args");
        HostScene hs;
        if (int rc = hs.build(cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, ORT_LAYOUT_COMPACT, 1, 0))
            return fail(nullptr, rc, hs.error);
        const ort::KScene& S = hs.S;
        const ort::CompactLayout& cl = hs.cl;
        const std::vector<float>& fplanes = hs.fplanes;
        const std::vector<uint8_t>& lut = hs.lut;
        const ort::PixelParams pp = pixel_params(p);
        ort::LocalFrames lf;
        ort::Counters cc;
        for (int k = 0; k < 6; ++k) cc.v[k] = 0;
        for (int k = 0; k < n_stats; ++k) stats[k] = 0.0;
        const int bw = (p->width + 7) / 8, bh = (p->height + 7) / 8;
        std::vector<std::vector<int>> seq(64);
        std::vector<int> all;
        for (int b = 0; b < bw * bh; b += block_step) {
            const int bx = b % bw, by = b / bw;
            bool uniform = true;
            int m0 = -1, lanes = 0;
            size_t maxlen = 0;
            for (int l = 0; l < 64; ++l) {
                seq[l].clear();
                const int px = bx * 8 + (l & 7), py = by * 8 + (l >> 3);
                if (px >= p->width || py >= p->height) continue;
                ort_rng st;
                ort::pixel_rng_init(pp, px, py, st);
                const ort::Ray ray = ort::primary_ray(pp, px, py, 0, st);
                const ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
                if (!ort::fast_path_ok(ray, inv, 0.001f, ORT_MAXFLOAT)) { uniform = false; continue; }
                lanes++;
                const int m = ((ray.d.z < 0.0f) << 2) | ((ray.d.x < 0.0f) << 1) | (ray.d.y < 0.0f);
                if (m0 < 0) m0 = m;
                else if (m != m0) uniform = false;
                ort::FastStateT<ort::Masks96> fs;
                if (!ort::fast_begin(S, fplanes.data(), lut.data(), ray, inv, 0.001f, ORT_MAXFLOAT, fs)) continue;
                for (;;) {
                    seq[l].push_back(fs.node);
                    if (ort::fast_step<false>(S, lut.data(), fs, lf, cc)) break;
                }
                maxlen = std::max(maxlen, seq[l].size());
            }
            stats[0] += 1;                  // waves
            stats[1] += uniform ? 0 : 1;    // waves with mixed order / non-fast lanes
            stats[2] += lanes;
            all.clear();
            for (int l = 0; l < 64; ++l)
                for (int nd : seq[l]) {
                    const bool leaf = !(cl.node[2 * (size_t)nd + 1] & ORT_INTERNAL_FLAG);
                    stats[leaf ? 4 : 3] += 1;  // individual internal / leaf visits
                    if (leaf) stats[5] += cl.node[2 * (size_t)nd + 1];  // individual sphere tests
                    all.push_back(nd);
                }
            std::sort(all.begin(), all.end());
            all.erase(std::unique(all.begin(), all.end()), all.end());
            for (int nd : all) {
                const bool leaf = !(cl.node[2 * (size_t)nd + 1] & ORT_INTERNAL_FLAG);
                stats[leaf ? 7 : 6] += 1;  // union internal / leaf visits
                if (leaf) stats[8] += cl.node[2 * (size_t)nd + 1];
            }
            // lockstep per-lane loop (the current kernel): iteration k runs the internal
            // block if any lane's k-th node is internal, the leaf block (max spheres) if any
            // is a leaf, and the pop for every lane still walking
            for (size_t k = 0; k < maxlen; ++k) {
                bool anyI = false, anyL = false;
                uint32_t maxS = 0;
                int act = 0;
                for (int l = 0; l < 64; ++l) {
                    if (k >= seq[l].size()) continue;
                    act++;
                    const uint32_t y = cl.node[2 * (size_t)seq[l][k] + 1];
                    if (y & ORT_INTERNAL_FLAG) anyI = true;
                    else { anyL = true; maxS = std::max(maxS, y); }
                }
                stats[9] += 1;            // lockstep iterations
                stats[10] += anyI;        // iterations running the internal block
                stats[11] += anyL;        // iterations running the leaf block
                stats[12] += maxS;        // sphere-loop trips
                stats[13] += act;         // lane-iterations
            }
            stats[14] += (double)maxlen;
            if (n_stats >= 18) {
                // wave-uniform iterations: every lane still walking pops the same node -- the
                // leading run of them (the shared descent) and all of them
                bool lead = true;
                for (size_t k = 0; k < maxlen; ++k) {
                    int nd = -1;
                    bool uni = true;
                    for (int l = 0; l < 64 && uni; ++l) {
                        if (k >= seq[l].size()) continue;
                        if (nd < 0) nd = seq[l][k];
                        else if (seq[l][k] != nd) uni = false;
                    }
                    lead = lead && uni;
                    stats[15] += lead ? 1 : 0;
                    stats[16] += uni ? 1 : 0;
                }
                stats[17] += 1;
            }
        }
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}


// ANALYSIS-ONLY (tools/bounce_lines.py): the rays of bounce `bounce` (>= 1) of a tile's pixels,
// 1 sample (the host restatement of the path: trace_ray + shade_bounce per bounce, as
// shade_pixel), and per alive ray the loads of its bounce walk (the persistent kernel's walk,
// rejected-sphere skip on): per step {node popped, first object entry of a leaf or -1, objects}.
// rays: 8 floats per pixel {o.xyz, d.xyz, alive, steps}.  walks: 3 ints per step, ray after
// ray; n_out[0] = steps written (all steps if <= cap).
int ort_debug_bounce_walks(const float* cr, const float* ma, const float* fr, int32_t n_spheres,
                           const float* node_min, const float* node_max, const int32_t* co, const int32_t* oo,
                           const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
                           const ort_params* p, const ort_tile* t, int32_t bounce, float* rays, int32_t* walks,
                           int64_t cap, int64_t* n_out) {
    try {
        const std::string bad = check_params(p, t);
        if (!bad.empty() || bounce < 1 || p->num_samples != 1) return fail(nullptr, ORT_ERR_INVALID_ARG, "bad args");
        HostScene hs;
        if (int rc = hs.build(cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, ORT_LAYOUT_COMPACT, 1, 0))
            return fail(nullptr, rc, hs.error);
        const ort::KScene& S = hs.S;
        const ort::CompactLayout& cl = hs.cl;
        const std::vector<float>&fplanes = hs.fplanes, &fplanes_b = hs.fplanes_b;
        const std::vector<uint8_t>& lut = hs.lut;
        const ort::PixelParams pp = pixel_params(p);
        const TileMap tm = {t->x0, t->width, t->y0, t->rows, t->band_height, t->band_stride};
        ort::LocalFrames lf;
        ort::Counters cc;
        for (int k = 0; k < 6; ++k) cc.v[k] = 0;
        int64_t n = 0;
        auto walk = [&](auto tag, const ort::Ray& ray, ort::V3 inv) -> int {
            using Masks = decltype(tag);
            ort::FastStateT<Masks> fs;
            const float* pl = cl.depth > 8 ? fplanes_b.data() : fplanes.data();
            if (!ort::fast_begin(S, pl, lut.data(), ray, inv, 0.001f, ORT_MAXFLOAT, fs)) return 0;
            int steps = 0;
            for (bool done = false; !done;) {
                const uint2 rec = fs.rec;
                const bool leaf = !(rec.y & ORT_INTERNAL_FLAG);
                if (n < cap) {
                    walks[3 * n] = fs.node;
                    walks[3 * n + 1] = leaf ? (int)rec.x : -1;
                    walks[3 * n + 2] = leaf ? (int)rec.y : 0;
                }
                ++n;
                ++steps;
                done = ort::fast_step<false>(S, lut.data(), fs, lf, cc);
            }
            return steps;
        };
        for (int row = 0; row < t->rows; ++row) {
            const int y = tile_row_to_y(tm, row);
            for (int c = 0; c < t->width; ++c) {
                float* o = rays + 8 * ((size_t)row * t->width + c);
                for (int k = 0; k < 8; ++k) o[k] = 0.0f;
                if (y >= p->height) continue;
                const int px = t->x0 + c;
                ort_rng st;
                ort::pixel_rng_init(pp, px, y, st);
                ort::Ray ray = ort::primary_ray(pp, px, y, 0, st);
                ort::V3 col = ort::mk(1.0f, 1.0f, 1.0f);
                float importance = 1.0f;
                bool alive = true;
                for (int b = 0; b < bounce && alive; ++b) {
                    if (importance < 0.01f) { alive = false; break; }
                    float th;
                    int entry;
                    const int tr = ort::trace_ray<0, false>(S, fplanes.data(), lut.data(), ray, false, th, entry, lf, nullptr,
                                                            nullptr, cc, b > 0, fplanes_b.data());
                    ort::HitRec h;
                    if (tr == ORT_TRACE_HIT) h = ort::hit_record<0>(S, ray, th, entry);
                    if (ort::shade_bounce(tr == ORT_TRACE_HIT, h, ray, col, importance, st)) alive = false;
                }
                if (!alive || importance < 0.01f) continue;
                ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
                o[0] = ray.o.x; o[1] = ray.o.y; o[2] = ray.o.z;
                o[3] = ray.d.x; o[4] = ray.d.y; o[5] = ray.d.z;
                o[6] = 1.0f;
                if (!ort::fast_prepare(S, ray, inv)) { o[6] = 2.0f; continue; }  // deferred (exact walk)
                o[7] = (float)(cl.depth > 8 ? walk(ort::Masks96Lean{}, ray, inv) : walk(ort::Masks64Plain{}, ray, inv));
            }
        }
        *n_out = n;
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

int64_t ort_debug_walk_steps(const float* cr, const float* ma, const float* fr, int32_t n_spheres,
                             const float* node_min, const float* node_max, const int32_t* co, const int32_t* oo,
                             const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
                             const ort_params* p, int32_t block_step, int32_t* lens, int64_t n_lens, uint16_t* steps,
                             int64_t cap) {
    return ort_debug_walk_steps_ex(cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, p,
                                   block_step, 0, lens, n_lens, steps, cap);
}

// production != 0 (tools/leaf_dedup_sim.py): the non-counting walk's steps -- the leaf children it
// tested (after the repeat masks of this build's Masks64::kLeafDedup) and its sphere tests, from
// the walk's own hooks (g_leaf_dedup, g_leaf_forms), in the same step records.
int64_t ort_debug_walk_steps_ex(const float* cr, const float* ma, const float* fr, int32_t n_spheres,
                                const float* node_min, const float* node_max, const int32_t* co, const int32_t* oo,
                                const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
                                const ort_params* p, int32_t block_step, int32_t production, int32_t* lens, int64_t n_lens,
                                uint16_t* steps, int64_t cap) {
    try {
        if (block_step < 1) return fail(nullptr, ORT_ERR_INVALID_ARG, "bad block_step");
        HostScene hs;
        if (int rc = hs.build(cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices, ORT_LAYOUT_COMPACT, 1, 0))
            return fail(nullptr, rc, hs.error);
        if (hs.cl.depth > 8) return fail(nullptr, ORT_ERR_UNSUPPORTED, "walk_steps: depth <= 8 walk only");
        const ort::KScene& S = hs.S;
        const std::vector<float>& fplanes = hs.fplanes;
        const std::vector<uint8_t>& lut = hs.lut;
        const ort::PixelParams pp = pixel_params(p);
        ort::LocalFrames lf;
        const int bw = (p->width + 7) / 8, bh = (p->height + 7) / 8;
        int64_t w = 0, n = 0;
        for (int b = 0; b < bw * bh; b += block_step, ++w) {
            const int bx = b % bw, by = b / bw;
            for (int l = 0; l < 64; ++l) {
                int32_t len = 0;
                const int px = bx * 8 + (l & 7), py = by * 8 + (l >> 3);
                if (px < p->width && py < p->height) {
                    ort_rng st;
                    ort::pixel_rng_init(pp, px, py, st);
                    const ort::Ray ray = ort::primary_ray(pp, px, py, 0, st);
                    const ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
                    ort::FastStateT<ort::Masks64> fs;
                    if (production && ort::fast_path_ok(ray, inv, 0.001f, ORT_MAXFLOAT) &&
                        ort::fast_begin(S, fplanes.data(), lut.data(), ray, inv, 0.001f, ORT_MAXFLOAT, fs)) {
                        for (bool done = false; !done;) {
                            ort::Counters cc;
                            const unsigned long long k0 = ort::g_leaf_dedup[0], o0 = ort::g_leaf_forms[0] + ort::g_leaf_forms[2];
                            const uint32_t y = fs.rec.y;
                            done = ort::fast_step<false>(S, lut.data(), fs, lf, cc);
                            const uint64_t kids = ort::g_leaf_dedup[0] - k0;
                            const uint64_t objs = std::min<uint64_t>(ort::g_leaf_forms[0] + ort::g_leaf_forms[2] - o0, 255);
                            const bool lk = (y & ORT_INTERNAL_FLAG) && (y & ORT_LEAFKIDS_FLAG);
                            if (n < cap) steps[n] = (uint16_t)(objs | (kids < 15 ? kids : 15) << 8 | (lk ? 0x8000u : 0u));
                            ++n;
                            ++len;
                        }
                    } else if (!production && ort::fast_path_ok(ray, inv, 0.001f, ORT_MAXFLOAT) &&
                        ort::fast_begin<0>(S, fplanes.data(), lut.data(), ray, inv, 0.001f, ORT_MAXFLOAT, fs)) {
                        for (bool done = false; !done;) {  // (the counting walk: node[] throughout)
                            ort::Counters cc;
                            for (int k = 0; k < 6; ++k) cc.v[k] = 0;
                            const uint32_t y = fs.rec.y;
                            done = ort::fast_step<true>(S, lut.data(), fs, lf, cc);
                            const uint64_t objs = cc.v[2] < 255 ? cc.v[2] : 255, kids = cc.v[0] - 1;
                            const bool lk = (y & ORT_INTERNAL_FLAG) && (y & ORT_LEAFKIDS_FLAG);
                            if (n < cap) steps[n] = (uint16_t)(objs | (kids < 15 ? kids : 15) << 8 | (lk ? 0x8000u : 0u));
                            ++n;
                            ++len;
                        }
                    }
                }
                if (64 * w + l < n_lens) lens[64 * w + l] = len;
            }
        }
        return n <= cap ? n : -n;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

int ort_debug_lds_image(int32_t depth, const float* planes, uint32_t* image, int64_t cap_words, int32_t* layout) {
    return ort_debug_lds_image_rev(depth, planes, 0, image, cap_words, layout);
}

int ort_debug_lds_image_rev(int32_t depth, const float* planes, int32_t rev_tables, uint32_t* image, int64_t cap_words,
                            int32_t* layout) {
    if (depth < 0 || depth > ORT_COMPACT_MAX_DEPTH || !planes || !layout)
        return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_lds_image: bad argument");
    const bool rev = rev_tables != 0 || ort::fast_rev_planes(depth);  // as k_lds_image
    const ort::LdsLayout l = ort::lds_layout(depth, rev);
    layout[0] = l.frames;
    layout[1] = l.lut;
    layout[2] = 4 * ort::fast_plane_floats(depth, rev);
    layout[3] = l.pop;
    layout[4] = l.pop < 0 ? -1 : l.pop + ort::kPopTable2;
    layout[5] = l.pop < 0 ? 0 : ort::kPopEntries;
    layout[6] = ort::Masks64::kPopTable ? 1 : 0;
    if (!image) return ORT_OK;
    if (cap_words * 4 < (int64_t)l.frames) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_lds_image: image too small");
    // what k_lds_image writes: the tables (fill_fast_planes), then the rank LUT
    std::vector<float> img((size_t)l.frames / 4, 0.0f);
    ort::fill_fast_planes(planes, img.data(), depth, rev);
    uint8_t* lut = reinterpret_cast<uint8_t*>(img.data()) + l.lut;
    for (int i = 0; i < (int)kRankLutBytes; ++i) lut[i] = ort::rank_lut_entry((uint32_t)i >> 8, (uint32_t)i & 255u);
    std::memcpy(image, img.data(), (size_t)l.frames);
    return ORT_OK;
}

// tests/test_leaf_inline.py: the compact layout's node[] (2 words a node), leaf_sph[] (4 words an
// entry) and the leaf16 records derived from them (4 words a node; none when the build has no
// Masks64::kLeafInline or the tree is deeper than 8), each into its array when given; sizes[3] =
// {nodes, entries, leaf16 records}.
int ort_debug_leaf16(const float* cr, int32_t n_spheres, const float* node_min, const float* node_max, const int32_t* co,
                     const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
                     uint32_t* node, uint32_t* leaf_sph, uint32_t* leaf16, int64_t* sizes) {
    try {
        if (!sizes) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_leaf16: null sizes");
        HostScene hs;
        if (int rc = hs.build(cr, nullptr, nullptr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices,
                              ORT_LAYOUT_COMPACT, 1, HostScene::kValidate))
            return fail(nullptr, rc, hs.error);
        sizes[0] = (int64_t)(hs.cl.node.size() / 2);
        sizes[1] = (int64_t)(hs.cl.leaf_sph.size() / 4);
        sizes[2] = (int64_t)hs.leaf16.size();
        if (node) std::memcpy(node, hs.cl.node.data(), 4 * hs.cl.node.size());
        if (leaf_sph) std::memcpy(leaf_sph, hs.cl.leaf_sph.data(), 4 * hs.cl.leaf_sph.size());
        if (leaf16 && !hs.leaf16.empty()) std::memcpy(leaf16, hs.leaf16.data(), 16 * hs.leaf16.size());
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

// tests/test_gpu_leaf_inline.py: a context's device leaf16 records copied to out (cap records);
// returns their number through n.
int ort_debug_ctx_leaf16(ort_ctx* ctx, uint32_t* out, int64_t cap, int64_t* n) {
    if (!ctx || !n) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_debug_ctx_leaf16: null argument");
    *n = ctx->scene.leaf16.p ? (int64_t)(ctx->scene.leaf16.bytes / 16) : 0;
    if (!out || *n == 0) return ORT_OK;
    if (cap < *n) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_debug_ctx_leaf16: out too small");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, ctx->scene.leaf16.p, ctx->scene.leaf16.bytes, hipMemcpyDeviceToHost));
    return ORT_OK;
}

// tests/layout_cases.py: one array of the compact layout HostScene::build holds for a tree, by name.
int ort_debug_layout(const float* cr, int32_t n_spheres, const float* node_min, const float* node_max, const int32_t* co,
                     const int32_t* oo, const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices,
                     const char* name, void* out, int64_t cap_bytes, int64_t* bytes) {
    try {
        if (!name || !bytes) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_layout: null argument");
        HostScene hs;
        if (int rc = hs.build(cr, nullptr, nullptr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices,
                              ORT_LAYOUT_COMPACT, 1, HostScene::kValidate))
            return fail(nullptr, rc, hs.error);
        const std::string what = name;
        const int32_t depth = hs.cl.depth, ordered = hs.cl.ordered ? 1 : 0;
        const void* src = nullptr;
        size_t n = 0;
        if (what == "node") src = hs.cl.node.data(), n = 4 * hs.cl.node.size();
        else if (what == "kid") src = hs.cl.kid.data(), n = 4 * hs.cl.kid.size();
        else if (what == "leaf_sph") src = hs.cl.leaf_sph.data(), n = 4 * hs.cl.leaf_sph.size();
        else if (what == "leaf_idx") src = hs.cl.leaf_idx.data(), n = 4 * hs.cl.leaf_idx.size();
        else if (what == "planes") src = hs.cl.planes.data(), n = 4 * hs.cl.planes.size();
        else if (what == "leaf16") src = hs.leaf16.data(), n = 16 * hs.leaf16.size();
        else if (what == "cam_node") src = hs.cam_node.data(), n = 8 * hs.cam_node.size();
        else if (what == "depth") src = &depth, n = 4;
        else if (what == "ordered") src = &ordered, n = 4;
        else return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_layout: unknown array " + what);
        *bytes = (int64_t)n;
        if (!out || n == 0) return ORT_OK;
        if (cap_bytes < (int64_t)n) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_layout: out too small");
        std::memcpy(out, src, n);
        return ORT_OK;
    } catch (const std::exception& ex) {
        return fail(nullptr, ORT_ERR_INTERNAL, ex.what());
    }
}

// tests/layout_cases.py: one device array of a context's scene, by name, copied to out; *bytes = its
// size.  The scalars depth, ordered and layout come as one int32.
int ort_debug_ctx_array(ort_ctx* ctx, const char* name, void* out, int64_t cap_bytes, int64_t* bytes) {
    if (!ctx || !name || !bytes) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_debug_ctx_array: null argument");
    if (!ctx->scene.has_scene) return fail(ctx, ORT_ERR_NO_SCENE, "ort_debug_ctx_array: no scene");
    const std::string what = name;
    const Scene& sc = ctx->scene;
    const int32_t scalars[3] = {sc.depth, sc.ordered ? 1 : 0, sc.layout};
    const char* const scalar_names[3] = {"depth", "ordered", "layout"};
    for (int k = 0; k < 3; ++k)
        if (what == scalar_names[k]) {
            *bytes = 4;
            if (!out) return ORT_OK;
            if (cap_bytes < 4) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_debug_ctx_array: out too small");
            std::memcpy(out, &scalars[k], 4);
            return ORT_OK;
        }
    const DevBuf* b = nullptr;
    if (what == "node") b = &sc.node;
    else if (what == "kid") b = &sc.kid;
    else if (what == "leaf_sph") b = &sc.leaf_sph;
    else if (what == "leaf_idx") b = &sc.leaf_idx;
    else if (what == "planes") b = &sc.planes;
    else if (what == "nk") b = &sc.nk;
    else if (what == "leaf16") b = &sc.leaf16;
    else if (what == "cam_node") b = &sc.cam_node;
    else if (what == "lds_img") b = &sc.lds_img;
    else if (what == "lds_rev") b = &sc.lds_rev;
    else return fail(ctx, ORT_ERR_INVALID_ARG, "ort_debug_ctx_array: unknown array " + what);
    *bytes = b->p ? (int64_t)b->bytes : 0;
    if (!out || *bytes == 0) return ORT_OK;
    if (cap_bytes < *bytes) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_debug_ctx_array: out too small");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, b->p, b->bytes, hipMemcpyDeviceToHost));
    return ORT_OK;
}

// The kLeafInline host walk's sphere tests and accepted hits per record form (render_core.h
// g_leaf_forms): {inline tests, inline hits, list tests, list hits}.
int ort_debug_leaf_forms(uint64_t* out4, int32_t reset) {
    for (int i = 0; i < 4; ++i) {
        if (out4) out4[i] = ort::g_leaf_forms[i];
        if (reset) ort::g_leaf_forms[i] = 0;
    }
    return ORT_OK;
}

// The non-counting kLeafInline host walk's leaf children (render_core.h g_leaf_dedup): {tested,
// dropped untested by a repeat mask}; out3[2] = Masks64::kLeafDedup of this build.
int ort_debug_leaf_dedup(uint64_t* out3, int32_t reset) {
    for (int i = 0; i < 2; ++i) {
        if (out3) out3[i] = ort::g_leaf_dedup[i];
        if (reset) ort::g_leaf_dedup[i] = 0;
    }
    if (out3) out3[2] = (uint64_t)ort::Masks64::kLeafDedup;
    return ORT_OK;
}

// The camera walk's two child tests on the host (render_core.h child_drops / child_order_keep).
int ort_debug_child_order(int32_t mode, const float* in, int64_t n, const float* tmins, int32_t n_tmin,
                          const float* closests, int32_t n_closest, uint64_t* out) {
    if (!out) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_child_order: no output");
    if (mode == 2) {
        for (int i = 0; i < 5; ++i) {
            out[i] = ort::g_order_visits[i];
            if (n) ort::g_order_visits[i] = 0;
        }
        out[5] = (uint64_t)ort::Masks64::kOrderBits;
        return ORT_OK;
    }
    if (mode == 3) {  // the host's tables
        for (int i = 0; i < 128; ++i) out[i] = ort::kOrderTablesHost.b[i];
        return ORT_OK;
    }
    if (mode == 4) {  // the device's (g_order_tables), read by a kernel on the current device
        uint8_t* d = nullptr;
        uint8_t t[sizeof(ort::OrderTables)];
        if (hipMalloc((void**)&d, sizeof(t)) != hipSuccess) return fail(nullptr, ORT_ERR_INTERNAL, "ort_debug_child_order: hipMalloc failed");
        hipLaunchKernelGGL(k_order_tables, dim3(1), dim3(128), 0, 0, d);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(t, d, sizeof(t), hipMemcpyDeviceToHost);
        (void)hipFree(d);
        if (e != hipSuccess) return fail(nullptr, ORT_ERR_INTERNAL, "ort_debug_child_order: reading the tables failed");
        for (int i = 0; i < 128; ++i) out[i] = t[i];
        return ORT_OK;
    }
    if ((mode != 0 && mode != 1) || !in || n < 0) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_child_order: bad args");
    auto both = [&](const float* v, uint32_t& a, uint32_t& b) {
        a = ~ort::child_drops(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]) & 0xffu;
        b = ort::child_order_keep(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);
    };
    if (mode == 0) {
        for (int64_t i = 0; i < n; ++i) {
            uint32_t a, b;
            both(in + 10 * i, a, b);
            out[2 * i] = a;
            out[2 * i + 1] = b;
        }
        return ORT_OK;
    }
    // mode 1: every tN <= tM <= tF per axis from the grid (ascending; ties where the indices are
    // equal), the folds of every (t_min, closest) pair applied as fast_visit applies them
    if (!tmins || !closests || n_tmin < 1 || n_closest < 1) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_child_order: bad args");
    for (int64_t i = 1; i < n; ++i)
        if (!(in[i - 1] <= in[i])) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_debug_child_order: grid not ascending");
    struct Tri { float v[3]; float operator[](int i) const { return v[i]; } };
    std::vector<Tri> tri;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = i; j < n; ++j)
            for (int64_t k = j; k < n; ++k) tri.push_back(Tri{{in[i], in[j], in[k]}});
    for (int i = 0; i < 4; ++i) out[i] = 0;
    for (const auto& A : tri)
        for (const auto& B : tri)
            for (const auto& Cx : tri)
                for (int32_t ti = 0; ti < n_tmin; ++ti)
                    for (int32_t ci = 0; ci < n_closest; ++ci) {
                        const float v[10] = {A[0], B[0], A[1], B[1], A[2], B[2], fmaxf(Cx[0], tmins[ti]), fmaxf(Cx[1], tmins[ti]),
                                             fminf(Cx[1], closests[ci]), fminf(Cx[2], closests[ci])};
                        uint32_t a, b;
                        both(v, a, b);
                        const bool premise = ort::fmin3(v[4], v[5], v[9]) >= ort::fmax3(v[0], v[1], v[6]);
                        if (premise) {  // {cases with X >= E, of them the forms disagree,
                            out[0] += 1;
                            out[1] += a != b;
                        } else {  //  cases with X < E, of them child_drops keeps a child}
                            out[2] += 1;
                            out[3] += a != 0;
                        }
                    }
    return ORT_OK;
}

int ort_debug_pop_coverage(uint64_t* hb_pops, uint64_t* sign_masks, int32_t reset) {
    for (int i = 0; i < 64; ++i)
        if (hb_pops) hb_pops[i] = ort::g_pop_cover[i];
    for (int i = 0; i < 8; ++i)
        if (sign_masks) sign_masks[i] = ort::g_pop_cover[64 + i];
    if (reset)
        for (int i = 0; i < 72; ++i) ort::g_pop_cover[i] = 0;
    return ORT_OK;
}

}  // extern "C"
