// Included by ort_kernel.hip after host_context.inc.  Scene upload and build: the compact layout's
// derived arrays (LDS image, nk, leaf16, cam_node), ort_upload_scene / ort_build_scene and their kin, and
// device_scene, the scene as the kernels take it.
namespace {

// The compact layout's workgroup LDS image (plane tables | rank LUT) from ctx->scene.planes.
int build_lds_image(ort_ctx* ctx) {
    for (int rev = 0; rev < 2; ++rev) {
        if (rev && !(kRevBounce && ctx->scene.depth > 8)) break;
        DevBuf& img = rev ? ctx->scene.lds_rev : ctx->scene.lds_img;
        const size_t bytes = (size_t)ort::lds_layout(ctx->scene.depth, rev || ort::fast_rev_planes(ctx->scene.depth)).frames;
        int rc;
        if ((rc = upload(ctx, img, nullptr, bytes))) return rc;
        // k_lds_image writes the tables and the LUT; the words that pad the tables to 16 bytes are
        // copied into LDS with the rest (never read there): zero, as the host's image has them
        HIPCHK(ctx, hipMemsetAsync(img.p, 0, bytes, ctx->stream));
        hipLaunchKernelGGL(k_lds_image, dim3(1), dim3(kBlock), 0, ctx->stream, (const float*)ctx->scene.planes.p, ctx->scene.depth,
                           rev != 0, (unsigned char*)img.p);
        HIPCHK(ctx, hipGetLastError());
    }
    return ORT_OK;
}

// The walks that use the rejected-sphere skip load a node's record and kid entry together
// (fetch_rec): one 16-byte load, one cache line per record instead of one in each array.
// Built when both arrays are there and 16 bytes per node stay under the buffer loads' 4 GiB.
int build_nk(ort_ctx* ctx) {
    free_buf(ctx->scene.nk);
    const int64_t n = (int64_t)(ctx->scene.node.bytes / 8);
    if (!ctx->scene.kid.p || ctx->scene.kid.bytes < ctx->scene.node.bytes || n == 0 || 16 * n >= (int64_t)UINT32_MAX)
        return ORT_OK;
    int rc;
    if ((rc = upload(ctx, ctx->scene.nk, nullptr, 16 * (size_t)n))) return rc;
    hipLaunchKernelGGL(k_interleave_nk, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const uint2*)ctx->scene.node.p, (const uint2*)ctx->scene.kid.p, (uint4*)ctx->scene.nk.p, n);
    HIPCHK(ctx, hipGetLastError());
    return ORT_OK;
}

// The depth <= 8 camera walk pops its records from cam_node (Masks64::kLeafDedup): node[] with the
// leaf-children nodes' repeat masks, derived from the finished leaf16 records on the same stream
// (build_leaf16 ends with it); 8 bytes per node id.
int build_cam_node(ort_ctx* ctx) {
    free_buf(ctx->scene.cam_node);
    const int64_t n = (int64_t)(ctx->scene.node.bytes / 8);
    if (!ort::Masks64::kLeafDedup || !ctx->scene.leaf16.p || n == 0) return ORT_OK;
    int rc;
    if ((rc = upload(ctx, ctx->scene.cam_node, nullptr, 8 * (size_t)n))) return rc;
    hipLaunchKernelGGL(k_cam_node, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const uint2*)ctx->scene.node.p, (const uint4*)ctx->scene.leaf16.p, (uint2*)ctx->scene.cam_node.p, n);
    HIPCHK(ctx, hipGetLastError());
    return ORT_OK;
}

// The depth <= 8 camera walk reads its leaf children's records from leaf16 (Masks64::kLeafInline):
// one per node id, 16 bytes, so at most 307 MB (a full depth-8 tree).
int build_leaf16(ort_ctx* ctx) {
    free_buf(ctx->scene.leaf16);
    free_buf(ctx->scene.cam_node);
    const int64_t n = (int64_t)(ctx->scene.node.bytes / 8);
    if (!ort::Masks64::kLeafInline || ctx->scene.depth > 8 || n == 0) return ORT_OK;
    int rc;
    if ((rc = upload(ctx, ctx->scene.leaf16, nullptr, 16 * (size_t)n))) return rc;
    hipLaunchKernelGGL(k_leaf16, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const uint2*)ctx->scene.node.p, (const uint4*)ctx->scene.leaf_sph.p, (int64_t)(ctx->scene.leaf_sph.bytes / 16),
                       (uint4*)ctx->scene.leaf16.p, n);
    HIPCHK(ctx, hipGetLastError());
    return build_cam_node(ctx);
}

// Root box for the coherence-sort key: the tree's root node, or the spheres' bounds when
// there is no tree (brute force).  Only orders work; never affects pixels.
void set_root_box(ort_ctx* ctx, const float* nmin, const float* nmax, const float* cr, int32_t n) {
    for (int a = 0; a < 3; ++a) {
        ctx->scene.root_lo[a] = 0.0f;
        ctx->scene.root_hi[a] = 0.0f;
    }
    if (nmin && nmax) {
        for (int a = 0; a < 3; ++a) {
            ctx->scene.root_lo[a] = nmin[a];
            ctx->scene.root_hi[a] = nmax[a];
        }
        return;
    }
    for (int32_t i = 0; i < n && cr; ++i)
        for (int a = 0; a < 3; ++a) {
            const float lo = cr[4 * (size_t)i + a] - cr[4 * (size_t)i + 3], hi = cr[4 * (size_t)i + a] + cr[4 * (size_t)i + 3];
            if (i == 0 || lo < ctx->scene.root_lo[a]) ctx->scene.root_lo[a] = lo;
            if (i == 0 || hi > ctx->scene.root_hi[a]) ctx->scene.root_hi[a] = hi;
        }
}

// Spheres -> device (bindings 0, 1 and the .xy of binding 2).
int upload_spheres(ort_ctx* ctx, const float* cr, const float* ma, const float* fr, int32_t n) {
    std::vector<float> fr2((size_t)n * 2);
    for (int32_t i = 0; i < n; ++i) {
        fr2[2 * (size_t)i] = fr[4 * (size_t)i];
        fr2[2 * (size_t)i + 1] = fr[4 * (size_t)i + 1];
    }
    int rc;
    if ((rc = upload(ctx, ctx->scene.sph_cr, cr, 16 * (size_t)n))) return rc;
    if ((rc = upload(ctx, ctx->scene.sph_ma, ma, 16 * (size_t)n))) return rc;
    if ((rc = upload(ctx, ctx->scene.sph_fr, fr2.data(), 8 * (size_t)n))) return rc;
    ctx->scene.n_spheres = n;
    return ORT_OK;
}

// ort_build_scene: GPU octree build (gpu_build.hip) straight into the kernel layout.
int build_impl(ort_ctx* ctx, const float* cr, const float* ma, const float* fr, int32_t n, int32_t max_depth,
               int32_t max_per_node, int32_t keep_tree) {
    if (n <= 0) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_build_scene: Sphere list is empty");
    if (!cr || !ma || !fr) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_build_scene: null sphere array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    free_scene(ctx);
    int rc;
    if ((rc = upload_spheres(ctx, cr, ma, fr, n))) return rc;
    ort::GpuTree t;
    const std::string e = ort::gpuBuildOctree((const float4*)ctx->scene.sph_cr.p, n, max_depth, max_per_node, ctx->stream, t);
    if (!e.empty()) {
        ort::freeGpuTree(t);
        return fail(ctx, e.find("out of memory") != std::string::npos ? ORT_ERR_OUT_OF_MEMORY : ORT_ERR_INTERNAL,
                    "ort_build_scene: " + e);
    }
    ctx->scene.n_nodes = t.n_nodes;
    ctx->scene.n_indices = t.n_indices;
    ctx->scene.depth = t.depth;
    ctx->scene.ordered = t.ordered;
    {
        float lo[3], hi[3];
        if (hipMemcpy(lo, t.node_min, 12, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(hi, t.node_max, 12, hipMemcpyDeviceToHost) == hipSuccess)
            set_root_box(ctx, lo, hi, nullptr, 0);
    }
    ctx->scene.build_ms = (float)(t.seconds * 1e3);
    std::string why;
    ort::CompactDev cd;
    const bool compact_ok = ctx->opt.force_layout != ORT_LAYOUT_EXPLICIT &&
                            ort::gpuCompactLayout(t, (const float4*)ctx->scene.sph_cr.p, ORT_COMPACT_MAX_DEPTH, ctx->stream, cd, why);
    if (compact_ok) {
        ctx->scene.layout = ORT_LAYOUT_COMPACT;
        ctx->scene.node = {cd.node, cd.node_bytes};
        ctx->scene.kid = {cd.kid, cd.node_bytes};
        ctx->scene.leaf_sph = {cd.leaf_sph, cd.leaf_bytes};
        ctx->scene.leaf_idx = {cd.leaf_idx, cd.idx_bytes};
        ctx->scene.planes = {cd.planes, cd.plane_bytes};
        if ((rc = build_lds_image(ctx)) || (rc = build_nk(ctx)) || (rc = build_leaf16(ctx))) {
            ort::freeGpuTree(t);
            return rc;
        }
    } else {
        if (ctx->opt.force_layout == ORT_LAYOUT_COMPACT) {
            ort::freeGpuTree(t);
            return fail(ctx, ORT_ERR_UNSUPPORTED, "compact layout forced but not possible: " + why);
        }
        ort::ExplicitDev ed;
        const std::string ee = ort::gpuExplicitLayout(t, ctx->stream, ed);
        ctx->scene.nodeA = {ed.nodeA, 16 * (size_t)std::max(t.n_nodes, 1)};
        ctx->scene.nodeB = {ed.nodeB, 16 * (size_t)std::max(t.n_nodes, 1)};
        ctx->scene.cnt = {ed.cnt, 4 * (size_t)std::max(t.n_nodes, 1)};
        ctx->scene.indices = {ed.indices, 4 * (size_t)std::max<int64_t>(t.n_indices, 1)};
        if (!ee.empty()) {
            ort::freeGpuTree(t);
            free_scene(ctx);
            return fail(ctx, ORT_ERR_HIP, "ort_build_scene: " + ee);
        }
        ctx->scene.layout = ORT_LAYOUT_EXPLICIT;
    }
    if (keep_tree) ctx->scene.tree = t;
    else ort::freeGpuTree(t);
    ctx->scene.has_scene = true;
    return ORT_OK;
}

int upload_impl(ort_ctx* ctx, const ort::SceneInput& in) {
    const std::string bad = ort::validateScene(in);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_upload_scene: " + bad);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    free_scene(ctx);
    int rc;
    if ((rc = upload_spheres(ctx, in.sph_cr, in.sph_ma, in.sph_fr, in.n_spheres))) return rc;
    ctx->scene.n_nodes = in.n_nodes;
    ctx->scene.n_indices = in.n_indices;
    ctx->scene.layout = ORT_LAYOUT_EXPLICIT;
    ctx->scene.depth = 0;
    set_root_box(ctx, in.n_nodes > 0 ? in.node_min : nullptr, in.n_nodes > 0 ? in.node_max : nullptr, in.sph_cr,
                 in.n_spheres);
    if (in.n_nodes > 0) {
        ort::CompactLayout cl;
        std::string why;
        const bool want_compact = ctx->opt.force_layout != ORT_LAYOUT_EXPLICIT;
        const bool compact_ok = want_compact && ort::buildCompactLayout(in, ORT_COMPACT_MAX_DEPTH, cl, why);
        if (ctx->opt.force_layout == ORT_LAYOUT_COMPACT && !compact_ok)
            return fail(ctx, ORT_ERR_UNSUPPORTED, "compact layout forced but not possible: " + why);
        if (compact_ok) {
            ctx->scene.layout = ORT_LAYOUT_COMPACT;
            ctx->scene.depth = cl.depth;
            ctx->scene.ordered = cl.ordered;
            if ((rc = upload(ctx, ctx->scene.node, cl.node.data(), 4 * cl.node.size()))) return rc;
            if ((rc = upload(ctx, ctx->scene.kid, cl.kid.data(), 4 * cl.kid.size()))) return rc;
            if ((rc = upload(ctx, ctx->scene.leaf_sph, cl.leaf_sph.data(), 4 * cl.leaf_sph.size()))) return rc;
            if ((rc = upload(ctx, ctx->scene.leaf_idx, cl.leaf_idx.data(), 4 * cl.leaf_idx.size()))) return rc;
            if ((rc = upload(ctx, ctx->scene.planes, cl.planes.data(), 4 * cl.planes.size()))) return rc;
            if ((rc = build_lds_image(ctx))) return rc;
            if ((rc = build_nk(ctx))) return rc;
            if ((rc = build_leaf16(ctx))) return rc;
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        } else {
            const int d = ort::treeDepth(in);
            ctx->scene.depth = d < 0 ? 0 : d;
            std::vector<float> A(4 * (size_t)in.n_nodes), B(4 * (size_t)in.n_nodes);
            for (int32_t i = 0; i < in.n_nodes; ++i) {
                for (int k = 0; k < 3; ++k) {
                    A[4 * (size_t)i + k] = in.node_min[3 * (size_t)i + k];
                    B[4 * (size_t)i + k] = in.node_max[3 * (size_t)i + k];
                }
                std::memcpy(&A[4 * (size_t)i + 3], &in.co[i], 4);
                std::memcpy(&B[4 * (size_t)i + 3], &in.oo[i], 4);
            }
            if ((rc = upload(ctx, ctx->scene.nodeA, A.data(), 4 * A.size()))) return rc;
            if ((rc = upload(ctx, ctx->scene.nodeB, B.data(), 4 * B.size()))) return rc;
            if ((rc = upload(ctx, ctx->scene.cnt, in.cnt, 4 * (size_t)in.n_nodes))) return rc;
            if ((rc = upload(ctx, ctx->scene.indices, in.indices, 4 * (size_t)in.n_indices))) return rc;
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
    } else {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->scene.has_scene = true;
    return ORT_OK;
}

ort::KScene device_scene(const ort_ctx* c) {
    ort::KScene S;
    std::memset(&S, 0, sizeof(S));
    S.sph_cr = (const float4*)c->scene.sph_cr.p;
    S.sph_ma = (const float4*)c->scene.sph_ma.p;
    S.sph_fr = (const float2*)c->scene.sph_fr.p;
    S.n_spheres = c->scene.n_spheres;
    S.n_nodes = c->scene.n_nodes;
    S.node = (const uint2*)c->scene.node.p;
    S.kid = c->opt.kid_skip ? (const uint2*)c->scene.kid.p : nullptr;
    S.nk = c->opt.kid_skip == 1 ? (const uint4*)c->scene.nk.p : nullptr;  // 2: the separate arrays (testing)
    S.nk_bytes = (uint32_t)c->scene.nk.bytes;
    S.tail_base = (uint32_t)c->scene.n_indices;
    S.leaf16 = (const uint4*)c->scene.leaf16.p;
    S.leaf16_bytes = (uint32_t)c->scene.leaf16.bytes;
    S.cam_node = (const uint2*)c->scene.cam_node.p;
    S.cam_bytes = (uint32_t)c->scene.cam_node.bytes;
    S.leaf_sph = (const float4*)c->scene.leaf_sph.p;
    S.node_bytes = (uint32_t)c->scene.node.bytes;
    S.leaf_bytes = (uint32_t)c->scene.leaf_sph.bytes;
    S.leaf_idx = (const int*)c->scene.leaf_idx.p;
    S.planes = (const float*)c->scene.planes.p;
    S.lds_img = (const uint4*)c->scene.lds_img.p;
    S.lds_img_p16 = (int)(align16(sizeof(float) * (size_t)ort::fast_plane_floats(c->scene.depth)) / 16);
    S.lds_img_n16 = ort::lds_layout(c->scene.depth, ort::fast_rev_planes(c->scene.depth)).frames / 16;
    S.lds_rev = (const uint4*)c->scene.lds_rev.p;
    S.lds_rev_n16 = ort::lds_layout(c->scene.depth, true).frames / 16;
    S.depth = c->scene.depth;
    S.nodeA = (const float4*)c->scene.nodeA.p;
    S.nodeB = (const float4*)c->scene.nodeB.p;
    S.count = (const int*)c->scene.cnt.p;
    S.indices = (const int*)c->scene.indices.p;
    return S;
}

}  // namespace

extern "C" {

int ort_upload_scene(ort_ctx* ctx, const float* cr, const float* ma, const float* fr, int32_t n_spheres,
                     const float* node_min, const float* node_max, const int32_t* co, const int32_t* oo,
                     const int32_t* cnt, int32_t n_nodes, const int32_t* idx, int64_t n_indices) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_upload_scene: null ctx");
    try {
        ort::SceneInput in{cr, ma, fr, n_spheres, node_min, node_max, co, oo, cnt, n_nodes, idx, n_indices};
        return upload_impl(ctx, in);
    } catch (const std::bad_alloc&) {
        return fail(ctx, ORT_ERR_OUT_OF_MEMORY, "ort_upload_scene: out of host memory");
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_upload_scene: ") + ex.what());
    }
}

int ort_upload_octree_nodes(ort_ctx* ctx, const float* cr, const float* ma, const float* fr, int32_t n_spheres,
                            const void* nodes, int32_t n_nodes, const int32_t* idx, int64_t n_indices) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_upload_octree_nodes: null ctx");
    if (n_nodes < 0 || (n_nodes > 0 && !nodes)) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_upload_octree_nodes: bad nodes");
    try {
        struct Rec { float mn[3], mx[3]; int32_t co, oo, cnt; };
        static_assert(sizeof(Rec) == 36, "GPUOctreeNode layout");
        const Rec* r = (const Rec*)nodes;
        std::vector<float> mn(3 * (size_t)n_nodes), mx(3 * (size_t)n_nodes);
        std::vector<int32_t> co((size_t)n_nodes), oo((size_t)n_nodes), cn((size_t)n_nodes);
        for (int32_t i = 0; i < n_nodes; ++i) {
            std::memcpy(&mn[3 * (size_t)i], r[i].mn, 12);
            std::memcpy(&mx[3 * (size_t)i], r[i].mx, 12);
            co[i] = r[i].co;
            oo[i] = r[i].oo;
            cn[i] = r[i].cnt;
        }
        ort::SceneInput in{cr, ma, fr, n_spheres, mn.data(), mx.data(), co.data(), oo.data(), cn.data(), n_nodes, idx, n_indices};
        return upload_impl(ctx, in);
    } catch (const std::bad_alloc&) {
        return fail(ctx, ORT_ERR_OUT_OF_MEMORY, "ort_upload_octree_nodes: out of host memory");
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_upload_octree_nodes: ") + ex.what());
    }
}

int ort_scene_get_info(const ort_ctx* ctx, ort_scene_info* info) {
    if (!ctx || !info) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_scene_get_info: null argument");
    if (!ctx->scene.has_scene) return fail(const_cast<ort_ctx*>(ctx), ORT_ERR_NO_SCENE, "no scene uploaded");
    info->n_spheres = ctx->scene.n_spheres;
    info->n_nodes = ctx->scene.n_nodes;
    info->n_indices = ctx->scene.n_indices;
    info->layout = ctx->scene.layout;
    info->tree_depth = ctx->scene.depth;
    int64_t b = 0;
    each_scene_buffer(ctx->scene, [&](const DevBuf& d) { b += (int64_t)d.bytes; });
    info->device_bytes = b;
    return ORT_OK;
}

int ort_build_scene(ort_ctx* ctx, const float* sphere_center_radius, const float* sphere_mat_albedo,
                    const float* sphere_fuzz_ri, int32_t n_spheres, int32_t max_depth, int32_t max_spheres_per_node,
                    int32_t keep_tree) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_build_scene: null ctx");
    try {
        return build_impl(ctx, sphere_center_radius, sphere_mat_albedo, sphere_fuzz_ri, n_spheres, max_depth,
                          max_spheres_per_node, keep_tree);
    } catch (const std::exception& ex) {
        return fail(ctx, ORT_ERR_INTERNAL, std::string("ort_build_scene: ") + ex.what());
    }
}

int ort_scene_export_octree(ort_ctx* ctx, float* node_min, float* node_max, int32_t* children_offset,
                            int32_t* objects_offset, int32_t* object_count, int32_t* object_indices) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_scene_export_octree: null ctx");
    const ort::GpuTree& t = ctx->scene.tree;
    if (!ctx->scene.has_scene || !t.co)
        return fail(ctx, ORT_ERR_NO_SCENE, "ort_scene_export_octree: no GPU-built tree kept (ort_build_scene keep_tree)");
    if (!node_min || !node_max || !children_offset || !objects_offset || !object_count || (!object_indices && t.n_indices))
        return fail(ctx, ORT_ERR_INVALID_ARG, "ort_scene_export_octree: null output");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)t.n_nodes;
    HIPCHK(ctx, hipMemcpy(node_min, t.node_min, 12 * n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(node_max, t.node_max, 12 * n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(children_offset, t.co, 4 * n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(objects_offset, t.oo, 4 * n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(object_count, t.cnt, 4 * n, hipMemcpyDeviceToHost));
    if (t.n_indices) HIPCHK(ctx, hipMemcpy(object_indices, t.idx, 4 * (size_t)t.n_indices, hipMemcpyDeviceToHost));
    return ORT_OK;
}

int ort_last_build_ms(const ort_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_last_build_ms: null argument");
    *ms = ctx->scene.build_ms;
    return ORT_OK;
}

}  // extern "C"
