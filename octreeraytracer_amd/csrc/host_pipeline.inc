// Included by ort_kernel.hip after host_pixel_paths.inc.  The wavefront pipeline: render_impl as a
// sequence of stages, and the render, timing and ort_count_traffic calls of the C ABI.
namespace {

// What a frame's shape, the scene and the options decide about its launches, computed once
// (render_impl) and read by every stage below.
struct FrameFlags {
    int mode;  // 0 the compact layout's walks, 1 the explicit layout's, 2 brute force
    int ns, maxd;
    bool counting;  // ort_count_traffic's render
    size_t pix;
    int tilesX, tilesY, gridX;
    // tile pairs (ORT_OPT_TILE_PAIRS; the compact layout, trees of 4+ levels: cost_order_pair's
    // scratch): the slot blocks of a pair are consecutive, a last odd column's second tile a hole
    // (auto: on large tiles, and on any tile whose caller turned the split walks off -- frames in
    // flight fill the tail, and pairs then pay on small tiles too: 1/4 band at 3 in flight +4 %)
    bool pairs;
    long long blocks;
    size_t slots;
    bool direct;       // 1 sample, 1 bounce
    bool pers_bounce;  // persistent only for the bounce >= 1 lists
    bool compact;      // the alive paths are listed between bounces
    bool fuse;         // primary-ray mode (1 sample, 1 bounce) on the compact layout: the trace kernels shade
    bool sorted;       // radix sort of every slot's key
    bool listsort;     // sort of the appended list (its length read back)
    // bounce 0 of a multi-bounce frame: the trace kernels shade their camera rays into the path
    // state and append the paths that go on (no hit records, no shade launch: C5 -0.7 ms)
    bool fuse_first;
    bool no_times;      // no per-launch events
    bool start_is_tr0;  // the frame's start event is its first trace launch's (TimingRing::begin)
    unsigned long long sig;  // frame_sig
};

FrameFlags frame_flags(const ort_ctx* ctx, const ort_params* p, const ort_tile* t, int mode, bool counting) {
    FrameFlags F;
    const Options& o = ctx->opt;
    F.mode = mode;
    F.ns = p->num_samples;
    F.maxd = p->max_depth;
    F.counting = counting;
    F.pix = (size_t)t->width * (size_t)t->rows;
    F.tilesX = (t->width + 15) / 16;
    F.tilesY = (t->rows + 15) / 16;
    F.pairs = mode == 0 && ctx->scene.depth >= 4 &&
              (o.tile_pairs > 0 || (o.tile_pairs < 0 && ((long long)F.pix >= kPairsAutoPixels || o.split_steps == 0)));
    F.gridX = F.pairs ? (F.tilesX + 1) / 2 : F.tilesX;
    F.blocks = (long long)(F.pairs ? 2 * F.gridX : F.tilesX) * F.tilesY;
    F.slots = (size_t)F.blocks * kBlock;
    F.direct = (F.ns == 1 && F.maxd == 1);
    F.pers_bounce = o.persistent == 2;
    F.compact = !F.direct && p->max_depth > 1;
    F.fuse = F.direct && mode == 0;
    F.sorted = F.compact && o.sort_paths == 1;
    F.listsort = F.compact && o.sort_paths == 2;
    F.fuse_first = F.compact && !F.sorted && mode == 0 && !counting;
    F.no_times = (o.debug_flags & 1) || !o.launch_times;
    F.start_is_tr0 = F.maxd > 0 && !F.no_times;
    F.sig = frame_sig(ctx, p, t);
    return F;
}

// What the stages hand on: the argument block, and what the set-up stages found for the loop.
struct FrameRun {
    hipStream_t s;
    PipeArgs a;
    size_t qtemp_bytes = 0;
    bool cam_moved = false;
    int split_steps = 0;
    bool split = false;  // split walks of the heavy camera rays (1 sample; the production kernels, bounce 0)
    int nbc = 0;         // heavy first: recorded bounce indices
    uint16_t* bcost = nullptr;
    const uint16_t* bcost_rd = nullptr;
    int key_bits = 0;
    size_t lds = 0, lds_exact = 0;
    int pblocks = 0;
    int fslot = 0;  // this frame's timing slot
    // the alive paths of the current bounce in append order, and the buffer the next
    // bounce's are appended to: qbuf[cur] / qcnt[cur] and qbuf[cur ^ 1] / qcnt[cur ^ 1]
    int* qbuf[2] = {nullptr, nullptr};
    int* qcnt[2] = {nullptr, nullptr};
    int cur = 1;
    int smp = 0, b = 0, bounces = 1;
};

// Where the kernels write: the caller's device memory at the caller's pitch or a tight one (tile
// rows, or the frame's under frame placement), or a tight scratch frame on the device, copied out
// (finish_output) to host memory at `pitch`.
int resolve_output(ort_ctx* ctx, const ort_params* p, const ort_tile* t, const ort_output* o, size_t pix, DevOutput& dout,
                   long long& pitch) {
    const long long tight = (long long)(o->placement == ORT_PLACE_FRAME ? p->width : t->width) * format_bpp(o->format);
    pitch = o->row_pitch_bytes ? (long long)o->row_pitch_bytes : tight;
    dout = {o->data, pitch, o->format, o->placement};
    if (o->is_device) return ORT_OK;
    int rc;
    if ((rc = ensure(ctx, ctx->pipe.scratch_out, (size_t)format_bpp(o->format) * pix))) return rc;
    dout.data = ctx->pipe.scratch_out.p;
    dout.pitch = tight;
    return ORT_OK;
}

// The pipeline's buffers for a frame of F.slots path slots.
int size_pipeline(ort_ctx* ctx, const FrameFlags& F, FrameRun& R) {
    Pipeline& pl = ctx->pipe;
    const size_t slots = F.slots;
    int rc;
    if ((rc = ensure(ctx, pl.hit, 8 * slots)) || (rc = ensure(ctx, pl.defer_list, 4 * slots)) ||
        (rc = ensure(ctx, pl.defer_count, 128)))
        return rc;
    if (!F.direct || ctx->opt.persistent) {
        if ((rc = ensure(ctx, pl.po, 16 * slots)) || (rc = ensure(ctx, pl.pd, 16 * slots)) ||
            (rc = ensure(ctx, pl.prng, 8 * slots)) || (rc = ensure(ctx, pl.pc, 16 * slots)) ||
            (rc = ensure(ctx, pl.pcol, 16 * slots)))
            return rc;
    }
    if (!F.compact) return ORT_OK;
    const bool sort = F.sorted || F.listsort;
    R.qtemp_bytes = sort ? ort::sortAliveTempBytes((int)slots) : 0;
    if ((rc = ensure(ctx, pl.qlist, 4 * slots)) || (rc = ensure(ctx, pl.qlist2, 4 * slots)) ||
        (rc = ensure(ctx, pl.qcount, 64)) || (rc = ensure(ctx, pl.qtemp, std::max<size_t>(R.qtemp_bytes, 16))))
        return rc;
    if (sort && ((rc = ensure(ctx, pl.skeys, 4 * slots)) || (rc = ensure(ctx, pl.skeys2, 4 * slots)) ||
                 (rc = ensure(ctx, pl.svals, 4 * slots))))
        return rc;
    return ORT_OK;
}

// The list-length hints belong to one frame shape and scene: a new shape takes a bank that no copy
// is still headed for (Pipeline::alive_host).
int select_hint_bank(ort_ctx* ctx, const FrameFlags& F) {
    Pipeline& pl = ctx->pipe;
    if (!F.listsort || F.sig == pl.hint_sig) return ORT_OK;
    int bank = -1;
    for (int i = 1; i <= Pipeline::kHintBanks && bank < 0; ++i) {
        const int c = (pl.hint_bank + i) % Pipeline::kHintBanks;
        if (!pl.hint_ev_used[c] || hipEventQuery(pl.hint_ev[c]) == hipSuccess) bank = c;
    }
    if (bank < 0) {  // every bank still awaits copies (several shape changes in flight)
        bank = (pl.hint_bank + 1) % Pipeline::kHintBanks;
        HIPCHK(ctx, hipEventSynchronize(pl.hint_ev[bank]));
    }
    pl.hint_bank = bank;
    for (int i = 0; i < Pipeline::kHints; ++i) pl.alive_host[bank * Pipeline::kHints + i] = -1;
    pl.hint_sig = F.sig;
    return ORT_OK;
}

// The argument block beyond base_args: the grid's order, the pipeline's buffers, this frame's
// counter sets (re-zeroed after a failed render: begin_counter_sets).
int fill_args(ort_ctx* ctx, const FrameFlags& F, FrameRun& R, unsigned long long* dcounters) {
    const Pipeline& pl = ctx->pipe;
    PipeArgs& a = R.a;
    a.pair = F.pairs ? 1 : 0;
    a.swizzle = ctx->opt.xcd_swizzle >= 0 ? ctx->opt.xcd_swizzle
                                          : ((!F.pairs && (long long)F.pix <= kRasterAutoPixels) ? 0 : 2);
    a.xrun_log2 = xcd_run_log2(F.gridX);
    a.refill = ctx->opt.refill;
    a.hit = (int2*)pl.hit.p;
    a.defer_list = (int*)pl.defer_list.p;
    int rc;
    bool fresh;
    if ((rc = begin_counter_sets(ctx, R.s, fresh))) return rc;
    a.sync = (int*)pl.defer_count.p;
    a.po = (float4*)pl.po.p;
    a.pd = (float4*)pl.pd.p;
    a.pc = (float4*)pl.pc.p;
    a.prng = (float2*)pl.prng.p;
    a.pcol = (float4*)pl.pcol.p;
    a.counters = dcounters;
    a.mp = ort::mortonPlan(ctx->scene.root_lo, ctx->scene.root_hi);
    // with bounce 0 shaded in the trace kernels every pixel's path ends in a kernel that knows
    // its pixel, so the last sample writes the final pixels itself (no finalize pass)
    a.final_out = F.fuse_first ? 1 : 0;
    a.key_spread = (const uint32_t*)pl.key_spread.p;
    return ORT_OK;
}

// The cost order: the per-workgroup camera-ray kernels (ort_trace_compact[_deep]) only.  Whether
// the camera moved since this context's last rendered frame (counting renders leave the
// record alone): heavy priority here and heavy-first's bounce classes (heavy_first_setup) both gate
// on it, whether or not the cost order is on.
int cost_order_setup(ort_ctx* ctx, const FrameFlags& F, FrameRun& R) {
    CostOrder& co = ctx->cost;
    PipeArgs& a = R.a;
    R.cam_moved = F.mode == 0 && std::memcmp(&co.prio_cam, &a.pp.cam, sizeof(ort::KCamera)) != 0;
    if (F.mode == 0 && !F.counting) co.prio_cam = a.pp.cam;
    if (!(F.mode == 0 && ctx->opt.cost_order && ctx->scene.depth >= 2)) return ORT_OK;
    int rc;
    if ((rc = ensure(ctx, co.pcost, 2 * F.slots))) return rc;
    if (F.sig != co.cost_sig) {  // a new shape: tile order for the first frame
        HIPCHK(ctx, hipMemsetAsync(co.pcost.p, 0, 2 * F.slots, R.s));
        co.cost_sig = F.sig;
    }
    a.pcost = (uint16_t*)co.pcost.p;
    // heavy priority only for a camera that has not moved since this context's last frame:
    // after a move the per-slot steps are one frame stale (a pixel's walk cost follows its
    // pixel-seeded lens/jitter sample more than the scene: same-slot hints keep an in-block
    // correlation of 0.82 with the new walks, reprojected ones 0.05 -- profiles/r05_moving_*),
    // and raising the wrong waves costs: C3 moving frames 1.855 -> 1.798 ms without it
    // (profiles/r05_moving_shift_c3.log), static frames unchanged
    a.prio_steps = R.cam_moved ? 0 : ctx->opt.heavy_prio;
    return ORT_OK;
}

// Whether this frame splits the walks of its heavy camera rays, and what that needs: the second
// stream, the heavy list's buffers, the level of the subtrees dealt to the lanes.
int split_setup(ort_ctx* ctx, const FrameFlags& F, FrameRun& R) {
    SplitWalks& sw = ctx->split;
    PipeArgs& a = R.a;
    R.split_steps = ctx->opt.split_steps >= 0 ? ctx->opt.split_steps
                                              : ((long long)F.pix <= kSplitAutoPixels ? kSplitAutoSteps : 0);
    R.split = (F.fuse || F.fuse_first) && a.pcost && R.split_steps > 0 && !F.counting && F.ns == 1;
    if (!R.split) {
        sw.pre_ok = false;  // (a queued heavy list is only for the next split frame)
        return ORT_OK;
    }
    int rc;
    if (!sw.aux_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&sw.aux_stream, hipStreamNonBlocking));
    if ((rc = ensure(ctx, sw.hbits, 4 * (F.slots / 32 + 1))) || (rc = ensure(ctx, sw.hlist, 4 * (size_t)SplitWalks::kSplitCap)) ||
        (rc = ensure(ctx, sw.hcnt, 64)))
        return rc;
    a.hlist = (const int*)sw.hlist.p;
    a.hcap = SplitWalks::kSplitCap;
    // the subtrees dealt to the lanes: ~5 levels above the leaves (a depth-8 tree: level 3)
    a.split_level = ctx->opt.split_level > 0 ? ctx->opt.split_level : std::max(1, ctx->scene.depth - 5);
    return ORT_OK;
}

#ifndef ORT_GEO_T
#define ORT_GEO_T 1.2f, 2.7f, 6.8f  // the class thresholds, in units of the box's smallest extent
#endif
// Heavy first: the bounce >= 1 lists of the persistent trace (sorted, default path)
// ... whose classes are read only while the camera stands still (the steps are recorded
// always): after a move last frame's bounce walks are not this frame's, and sorting stale
// heavy paths first cost C5's moving frames 0.8 % (1568 -> 1556 Mrays/s, bench --opt HEAVY_FIRST=0);
// then the classes come from the rays themselves (geo_class_bits).
int heavy_first_setup(ort_ctx* ctx, const FrameFlags& F, FrameRun& R) {
    CostOrder& co = ctx->cost;
    PipeArgs& a = R.a;
    R.nbc = std::min(F.ns * (F.maxd > 0 ? F.maxd : 1), CostOrder::kCostBounces);
    if (F.listsort && F.mode == 0 && F.pers_bounce && ctx->opt.heavy_first > 0) {
        int rc;
        if ((rc = ensure(ctx, co.bcost, 2 * F.slots * (size_t)R.nbc))) return rc;
        if (F.sig != co.bcost_sig) {  // a new shape: no heavy walks known
            HIPCHK(ctx, hipMemsetAsync(co.bcost.p, 0, 2 * F.slots * (size_t)R.nbc, R.s));
            co.bcost_sig = F.sig;
        }
        R.bcost = (uint16_t*)co.bcost.p;
        a.heavy = ctx->opt.heavy_first;
    }
    R.bcost_rd = R.cam_moved ? nullptr : R.bcost;
    if (R.bcost && !R.bcost_rd) {  // moved: classes from the rays themselves (geo_class_bits)
        a.geo_heavy = 1;
        float m = 3.0e38f;
        for (int q = 0; q < 3; ++q) {
            a.gbox[q] = ctx->scene.root_lo[q];
            a.gbox[3 + q] = ctx->scene.root_hi[q];
            m = std::min(m, ctx->scene.root_hi[q] - ctx->scene.root_lo[q]);
        }
        const float gt[3] = {ORT_GEO_T};
        for (int q = 0; q < 3; ++q) a.gthr[q] = gt[q] * m;
    }
    R.key_bits = R.bcost ? ort::kPathKeyBits + kHeavyKeyBits : ort::kPathKeyBits;
    return ORT_OK;
}

// Open this trace launch: its counter set (mode 0 launches ort_trace_exact, which zeroes the other),
// its timing segment -- every trace launch of the frame, up to kSeg (analysis flag 1: none) -- and
// at, its copy of the arguments (analysis, ORT_PERSIST_CLOCK: with a record range per launch).
int open_trace_launch(ort_ctx* ctx, const FrameFlags& F, FrameRun& R, int pb, PipeArgs& at, int& seg, bool& timed) {
    Pipeline& pl = ctx->pipe;
    int* const set = (int*)pl.defer_count.p + 16 * pl.sync_set;
    R.a.sync = set;
    if (F.mode == 0) R.a.sync_next = (int*)pl.defer_count.p + 16 * (pl.sync_set ^ 1);
    else HIPCHK(ctx, hipMemsetAsync(set, 0, 64, R.s));
    seg = ctx->ring.tseg[R.fslot];
    timed = seg < TimingRing::kSeg && !F.no_times;
    if (timed) HIPCHK(ctx, ctx->ring.begin(R.fslot, seg, R.s, !(seg == 0 && F.start_is_tr0)));
    at = R.a;
#if ORT_ANALYSIS
    if (pb > 0 && R.a.wclock) {  // analysis (ORT_PERSIST_CLOCK): a record range per launch
        const long long nw = (long long)pb * (ctx->scene.depth > 8 ? kPersistDeepBlock : kBlock) / 64 *
                             (ORT_PERSIST_STATS ? 2 : 1);  // records per launch
        at.wclock = (seg + 1) * nw <= ctx->wclock_n ? R.a.wclock + seg * nw : nullptr;
        at.wclock_n = (int)nw;
    }
#endif
    return ORT_OK;
}

// Split walks, before the tile kernel: the heavy rays of this frame (last frame's steps) -- listed
// by the last split frame of this shape (its exact kernel), or by a scan here -- then their split
// walks on the second stream, beside the per-tile kernel (which passes over them).  With
// split_walks_join the only code that touches aux_stream.
int split_walks_start(ort_ctx* ctx, const FrameFlags& F, const FrameRun& R, int fmode, PipeArgs& at) {
    SplitWalks& sw = ctx->split;
    const hipStream_t s = R.s;
    const bool pre = sw.pre_ok && sw.pre_sig == F.sig && sw.pre_steps == R.split_steps && !(ctx->opt.debug_flags & 2);
    sw.pre_ok = false;
    int* hc = (int*)sw.hcnt.p;
    // the second stream follows this one up to here: with shading fused (1 bounce)
    // nothing of this frame precedes the split walks on it but ev0 (event packets
    // cost the frame ~1 % each); bounce 0 of a longer path needs the list memset too
    if (fmode == 1) {
        HIPCHK(ctx, hipStreamWaitEvent(sw.aux_stream, ctx->ring.ev0_last, 0));
    } else {
        HIPCHK(ctx, hipEventRecord(sw.ev_scan, s));
        HIPCHK(ctx, hipStreamWaitEvent(sw.aux_stream, sw.ev_scan, 0));
    }
    if (!pre) {  // (with pre, the last frame's exact kernel listed them, in this stream's order)
        HIPCHK(ctx, hipMemsetAsync(hc, 0, 64, sw.aux_stream));
        sw.hpar = 0;
        const HeavyScan H{(const uint16_t*)R.a.pcost, (int)F.slots, R.split_steps, SplitWalks::kSplitCap,
                          (uint32_t*)sw.hbits.p, (int*)sw.hlist.p, hc};
        hipLaunchKernelGGL(k_heavy_scan, dim3((unsigned)((F.slots + 4095) / 4096)), dim3(kBlock), 0, sw.aux_stream, H);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(sw.ev_pre, sw.aux_stream));
        HIPCHK(ctx, hipStreamWaitEvent(s, sw.ev_pre, 0));  // the tile kernel reads hbits
    }
    at.hsync = hc + 8 * sw.hpar;
    at.hsync_next = hc + 8 * (sw.hpar ^ 1);
    const hipError_t e = launch_trace_split(ctx->scene.depth > 8, fmode, at, R.lds, sw.aux_stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipGetLastError()");
    HIPCHK(ctx, hipEventRecord(sw.ev_split, sw.aux_stream));
    at.hbits = (const uint32_t*)sw.hbits.p;
    return ORT_OK;
}

// ... and after it: the split walks joined before the exact kernel (and before the launch's timing
// segment ends), which also lists the next frame's heavy rays, from this frame's steps (final now)
// -- no scan launch or cross-stream wait opens the next frame; ort_trace_split zeroed the other
// count pair.
int split_walks_join(ort_ctx* ctx, const FrameFlags& F, const FrameRun& R, PipeArgs& at) {
    SplitWalks& sw = ctx->split;
    HIPCHK(ctx, hipStreamWaitEvent(R.s, sw.ev_split, 0));
    sw.hpar ^= 1;
    at.scan_pcost = R.a.pcost;
    at.scan_T = R.split_steps;
    at.scan_bits = (uint32_t*)sw.hbits.p;
    at.scan_list = (int*)sw.hlist.p;
    at.scan_count = (int*)sw.hcnt.p + 8 * sw.hpar;
    sw.pre_sig = F.sig;
    sw.pre_steps = R.split_steps;
    return ORT_OK;
}

// The trace launch of bounce R.b: tile pairs, the persistent kernel over a list, the per-tile
// kernels or the explicit-layout / brute-force kernel, the heavy rays' split walks beside it, and
// the exact walk of the deferred rays (fmode 1: shading fused; 2: bounce 0 of a longer path, fused).
[[gnu::noinline]] int trace_bounce(ort_ctx* ctx, const FrameFlags& F, FrameRun& R, int fmode) {
    const hipStream_t s = R.s;
    const int smp = R.smp, b = R.b, bounces = R.bounces, cur = R.cur;
    const bool prim = b == 0;
    const int pb = (F.pers_bounce && b > 0) ? R.pblocks : 0;
    PipeArgs at;
    int seg, rc;
    bool timed;
    if ((rc = open_trace_launch(ctx, F, R, pb, at, seg, timed))) return rc;
    if (fmode == 2) {  // the trace kernels append bounce 1's list (as ort_shade_kernel would)
        HIPCHK(ctx, hipMemsetAsync(R.qcnt[cur ^ 1], 0, sizeof(int), s));
        at.qnext = R.qbuf[cur ^ 1];
        at.qnext_count = R.qcnt[cur ^ 1];
        at.qnext_keys = F.listsort ? (uint32_t*)ctx->pipe.skeys.p : nullptr;
    }
    {   // heavy first: record index smp * bounces + b (bounces >= 1 only)
        const int hi = smp * bounces + b;
        if (R.bcost && pb > 0 && b > 0 && hi < R.nbc) at.bcost_w = R.bcost + (size_t)hi * F.slots;
        if (R.bcost_rd && fmode == 2 && hi + 1 < R.nbc && b + 1 < bounces) at.bcost_r = R.bcost_rd + (size_t)(hi + 1) * F.slots;
    }
    const bool do_split = R.split && (fmode == 1 || fmode == 2);
    if (do_split && (rc = split_walks_start(ctx, F, R, fmode, at))) return rc;
    const int tblocks = (prim && F.pairs) ? (int)(F.blocks / 2) : (int)F.blocks;  // a workgroup per tile pair
    hipError_t e = launch_trace(F.counting, F.mode, prim, at, tblocks, pb, R.lds, s, fmode);
    if (e != hipSuccess) return hip_fail(ctx, e, "trace kernel launch");
    if (do_split && (rc = split_walks_join(ctx, F, R, at))) return rc;
    if (timed) {
        HIPCHK(ctx, ctx->ring.end(R.fslot, seg, s));
        ctx->ring.tseg[R.fslot] = seg + 1;
    }
    if (F.mode == 0) {
        e = launch_trace_exact(F.counting, prim, fmode, at, R.lds_exact, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "ort_trace_exact launch");
        ctx->pipe.sync_set ^= 1;  // it zeroes the other set for the next launch
        // it listed the next frame's heavy rays: only now may that frame skip its scan
        if (do_split) ctx->split.pre_ok = true;
    }
    return ORT_OK;
}

// Shade / append.  Bounce >= 1: the bounce's alive paths in APPEND order (about slot order: the
// path-state reads and writes coalesce; the sorted trace list scattered them, C5
// 65.4 -> 63.0 ms) -- or, with the every-slot sort (sort_paths 1), every slot
[[gnu::noinline]] int shade_bounce(ort_ctx* ctx, const FrameFlags& F, const FrameRun& R) {
    const int b = R.b, cur = R.cur;
    PipeArgs a2 = R.a;
    a2.qlist = nullptr;
    a2.qcount = nullptr;
    if (F.compact && !F.sorted && b > 0) {
        a2.qlist = R.qbuf[cur];
        a2.qcount = R.qcnt[cur];
    }
    if (F.compact && !F.sorted && !R.a.nobounce && b + 1 < R.bounces) {
        // the compaction: the shade kernel appends the paths that go on, one atomic
        // per workgroup (a separate rocprim::select pass over the slots cost 0.55 ms
        // per C5 bounce), into the other list buffer
        HIPCHK(ctx, hipMemsetAsync(R.qcnt[cur ^ 1], 0, sizeof(int), R.s));
        a2.qnext = R.qbuf[cur ^ 1];
        a2.qnext_count = R.qcnt[cur ^ 1];
        a2.qnext_keys = F.listsort ? (uint32_t*)ctx->pipe.skeys.p : nullptr;
        const int hn = R.smp * R.bounces + b + 1;  // the next bounce's record
        if (R.bcost_rd && hn < R.nbc) a2.bcost_r = R.bcost_rd + (size_t)hn * F.slots;
    }
    const hipError_t e = launch_shade(F.mode, b == 0, F.direct, a2, (int)F.blocks, R.s);
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_shade_kernel launch");
    return ORT_OK;
}

// Order the next bounce's list (it walks only the alive paths): the every-slot sort, or the list
// just appended, sorted up to a bound, and its length's copy into the next frame's hints.
[[gnu::noinline]] int order_next_list(ort_ctx* ctx, const FrameFlags& F, FrameRun& R) {
    Pipeline& pl = ctx->pipe;
    PipeArgs& a = R.a;
    const hipStream_t s = R.s;
    const int slots = (int)F.slots;
    if (F.sorted) {
        const ort::SortBuffers sb{(uint32_t*)pl.skeys.p, (uint32_t*)pl.skeys2.p, (int*)pl.svals.p, (int*)pl.qlist.p};
        const hipError_t e = ort::sortAlive(pl.qtemp.p, R.qtemp_bytes, (const float4*)pl.po.p, (const float4*)pl.pd.p, slots,
                                            ctx->scene.root_lo, ctx->scene.root_hi, (const uint32_t*)pl.key_spread.p, sb,
                                            (int*)pl.qcount.p, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "path compaction");
        a.qlist = (const int*)pl.qlist.p;
        a.qcount = (const int*)pl.qcount.p;
        return ORT_OK;
    }  // else the shade kernel appended them
    R.cur ^= 1;  // the list just appended is the next bounce's
    const int cur = R.cur;
    if (F.listsort) {
        // sort only about the alive paths, not every slot (C5: 36.6 M keys, not
        // 99.6 M), without reading the length back: the bound is this bounce's
        // length in an earlier frame of the same shape plus 1/64 + 1024 (the
        // same camera gives the same length), every slot when there is none
        const int hi = R.smp * R.bounces + R.b;
        long long bound = (long long)slots;
        if (ctx->opt.sort_bound > 0) bound = ctx->opt.sort_bound;
        else if (hi < Pipeline::kHints) {
            const int h = ((volatile int*)pl.alive_host)[pl.hint_bank * Pipeline::kHints + hi];
            if (h >= 0) bound = (long long)h + (h >> 6) + 1024;
        }
        bound = std::min<long long>(bound, (long long)slots);
        // (key, path) pairs as the shade / trace kernels appended them
        const ort::SortBuffers sb{(uint32_t*)pl.skeys.p, (uint32_t*)pl.skeys2.p, R.qbuf[cur], (int*)pl.svals.p};
        const hipError_t e = ort::sortListBounded(pl.qtemp.p, R.qtemp_bytes, (int)bound, R.qcnt[cur], sb, s, R.key_bits);
        if (e != hipSuccess) return hip_fail(ctx, e, "path list sort");
        if (hi < Pipeline::kHints)  // the next frame's bound (pinned: no host wait)
            HIPCHK(ctx, hipMemcpyAsync(pl.alive_host + pl.hint_bank * Pipeline::kHints + hi, R.qcnt[cur], sizeof(int),
                                       hipMemcpyDeviceToHost, s));
    }
    a.qlist = F.listsort ? (const int*)pl.svals.p : R.qbuf[cur];
    a.qcount = R.qcnt[cur];
    return ORT_OK;
}

// The frame's samples and bounces: trace, shade / append, order the next bounce's list.  (The three
// are kept out of line: inlined here, the loop was unswitched on the flags into 47 KB of host code.)
int run_bounces(ort_ctx* ctx, const FrameFlags& F, FrameRun& R) {
    Pipeline& pl = ctx->pipe;
    PipeArgs& a = R.a;
    int rc;
    for (R.smp = 0; R.smp < F.ns; ++R.smp) {
        a.sample = R.smp;
        a.qlist = nullptr;  // bounce 0: every slot
        a.qcount = nullptr;
        R.qbuf[0] = (int*)pl.qlist.p;
        R.qbuf[1] = (int*)pl.qlist2.p;
        R.qcnt[0] = (int*)pl.qcount.p;
        R.qcnt[1] = (int*)pl.qcount.p + 4;
        R.cur = 1;  // bounce 0 appends to qbuf[0]
        R.bounces = F.maxd > 0 ? F.maxd : 1;
        a.nobounce = F.maxd <= 0;
        for (R.b = 0; R.b < R.bounces; ++R.b) {
            a.last = (R.b == R.bounces - 1);
            const int fmode = F.fuse ? 1 : ((R.b == 0 && F.fuse_first) ? 2 : 0);
            if (!a.nobounce && (rc = trace_bounce(ctx, F, R, fmode))) return rc;
            if (!F.fuse && fmode != 2 && (rc = shade_bounce(ctx, F, R))) return rc;
            if (F.compact && !a.nobounce && R.b + 1 < R.bounces && (rc = order_next_list(ctx, F, R))) return rc;
        }
    }
    return ORT_OK;
}

int render_impl(ort_ctx* ctx, const ort_params* p, const ort_tile* t, const ort_output* o, void* stream,
                unsigned long long* dcounters) {
    const std::string bad = check_params(p, t);
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_render: " + bad);
    const std::string bad_out = check_output(p, t, o);
    if (!bad_out.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_render: " + bad_out);
    if (!ctx->scene.has_scene) return fail(ctx, ORT_ERR_NO_SCENE, "ort_render: no scene uploaded");
    const int mode = (p->use_octree == 1) ? (ctx->scene.layout == ORT_LAYOUT_COMPACT ? 0 : 1) : 2;
    if (mode != 2 && ctx->scene.n_nodes <= 0) return fail(ctx, ORT_ERR_NO_SCENE, "ort_render: scene has no octree");
    const FrameFlags F = frame_flags(ctx, p, t, mode, dcounters != nullptr);
    if (!o->data && F.pix > 0) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_render: null output");
    if (F.pix == 0) return ORT_OK;
    if (F.blocks * kBlock > 0x7fffffffLL) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_render: tile too large");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FrameRun R;
    const hipStream_t s = R.s = stream ? (hipStream_t)stream : ctx->stream;
    DevOutput dout;
    long long pitch;
    int rc;
    if ((rc = resolve_output(ctx, p, t, o, F.pix, dout, pitch))) return rc;
    if (!dcounters && use_pixel_paths(ctx, mode, F.ns, F.maxd)) {  // the frame in one launch
        if ((rc = ensure(ctx, ctx->pipe.defer_count, 128)) || (rc = render_pixel_paths(ctx, p, t, mode, dout, s))) return rc;
        return finish_output(ctx, o, dout, t, pitch, stream, s);
    }
    if ((rc = size_pipeline(ctx, F, R)) || (rc = select_hint_bank(ctx, F))) return rc;
    // the key tables of the current root box (built once per scene)
    if ((F.sorted || F.listsort) && (rc = ensure_key_spread(ctx))) return rc;
    R.a = base_args(ctx, p, t, dout, F.gridX, F.tilesY, F.blocks);
    if ((rc = fill_args(ctx, F, R, dcounters)) || (rc = cost_order_setup(ctx, F, R)) || (rc = split_setup(ctx, F, R)) ||
        (rc = heavy_first_setup(ctx, F, R)))
        return rc;
    const int depth = ctx->scene.depth;
    R.lds = lds_bytes(mode, depth, false);
    R.lds_exact = lds_bytes(mode, depth, true);
    R.pblocks = (mode == 0 && ctx->opt.persistent) ? persistent_blocks(ctx->device, F.counting, depth > 8, depth, R.lds, F.blocks) : 0;
    // the frame's start: also the start of its first trace launch when that is timed
    TimingRing& ring = ctx->ring;
    R.fslot = ring.slot();
    ring.tseg[R.fslot] = 0;
    ring.ev0_last = F.start_is_tr0 ? ring.tr0[R.fslot][0] : ctx->frame_ev.ev0;
    HIPCHK(ctx, hipEventRecord(ring.ev0_last, s));
    if ((rc = run_bounces(ctx, F, R))) return rc;
    if (ring.tseg[R.fslot] > 0) ring.frames += 1;
    if (F.listsort) {  // after this frame's hint copies: the bank is free once this completes
        HIPCHK(ctx, hipEventRecord(ctx->pipe.hint_ev[ctx->pipe.hint_bank], s));
        ctx->pipe.hint_ev_used[ctx->pipe.hint_bank] = true;
    }
    if (!F.direct && !R.a.final_out) {
        hipLaunchKernelGGL(ort_finalize_kernel, dim3((unsigned)F.blocks), dim3(kBlock), 0, s, R.a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(ctx, e, "ort_finalize_kernel launch");
    }
    HIPCHK(ctx, ctx->frame_ev.end(s));
    ctx->pipe.sync_ok = true;  // every launch enqueued: the counter sets are in step again
    return finish_output(ctx, o, dout, t, pitch, stream, s);
}

}  // namespace

extern "C" {

int ort_render(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, float* rgb_out, int out_is_device,
               void* stream) {
    const ort_output o = {rgb_out, out_is_device, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
    return ort_render_ex(ctx, params, tile, &o, stream);
}

int ort_render_ex(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, const ort_output* output,
                  void* stream) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_render: null ctx");
    return render_impl(ctx, params, tile, output, stream, nullptr);
}

int ort_last_kernel_ms(ort_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_last_kernel_ms: null argument");
    if (!ctx->frame_ev.timed) return fail(ctx, ORT_ERR_NO_SCENE, "no kernel launched yet");
    HIPCHK(ctx, ctx->frame_ev.elapsed(ms, ctx->ring.ev0_last));
    return ORT_OK;
}

int ort_last_trace_ms(ort_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_last_trace_ms: null argument");
    return ort_trace_times_ms(ctx, 1, ms) == 1 ? ORT_OK : fail(ctx, ORT_ERR_NO_SCENE, "no trace kernel timed yet");
}

int ort_trace_times_ms(ort_ctx* ctx, int n, float* ms) {
    if (!ctx || !ms || n < 0) return -ORT_ERR_INVALID_ARG;
    const TimingRing& ring = ctx->ring;
    const int k = ring.held(n);
    for (int i = 0; i < k; ++i)
        if (ring.elapsed(ring.slot_of(k, i), 0, &ms[i]) != hipSuccess) return -ORT_ERR_HIP;
    return k;
}

int ort_frame_trace_times_ms(ort_ctx* ctx, int n, float* ms, int32_t* launches) {
    if (!ctx || !ms || n < 0) return -ORT_ERR_INVALID_ARG;
    const TimingRing& ring = ctx->ring;
    const int k = ring.held(n);
    for (int i = 0; i < k; ++i) {
        const int slot = ring.slot_of(k, i);
        float sum = 0.0f;
        for (int j = 0; j < ring.tseg[slot]; ++j) {
            float t = 0.0f;
            if (ring.elapsed(slot, j, &t) != hipSuccess) return -ORT_ERR_HIP;
            sum += t;
        }
        ms[i] = sum;
        if (launches) launches[i] = ring.tseg[slot];
    }
    return k;
}

int ort_count_traffic(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, uint64_t* counts) {
    if (!ctx || !counts) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_count_traffic: null argument");
    const std::string bad = check_params(params, tile);  // before the counters and the frame are allocated
    if (!bad.empty()) return fail(ctx, ORT_ERR_INVALID_ARG, "ort_count_traffic: " + bad);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->pipe.counters.p) {
        HIPCHK(ctx, hipMalloc(&ctx->pipe.counters.p, 64));
        ctx->pipe.counters.bytes = 64;
    }
    HIPCHK(ctx, hipMemsetAsync(ctx->pipe.counters.p, 0, 64, ctx->stream));
    const size_t pix = tile ? (size_t)tile->width * (size_t)tile->rows : 0;
    DevBuf tmp;
    if (pix) HIPCHK(ctx, hipMalloc(&tmp.p, 12 * pix));
    const ort_output o = {tmp.p, 1, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0};
    const int rc = render_impl(ctx, params, tile, &o, nullptr, (unsigned long long*)ctx->pipe.counters.p);
    if (rc == ORT_OK && !pix) {
        // a tile of no pixels: render_impl launched nothing and waited for nothing, so the memset
        // above may still be queued on the context's (non-blocking) stream, which the copy below
        // does not wait for -- it would return the counters of the count before this one
        for (int k = 0; k < ORT_COUNT_N; ++k) counts[k] = 0;
        return ORT_OK;
    }
    if (rc == ORT_OK) {
        unsigned long long h[8] = {0};
        hipError_t e = hipMemcpy(h, ctx->pipe.counters.p, 64, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free_buf(tmp); return hip_fail(ctx, e, "ort_count_traffic: copy counters"); }
        for (int k = 0; k < ORT_COUNT_N; ++k) counts[k] = h[k];
        // pixels inside the frame (main() runs once per fragment)
        const TileMap tm = {tile->x0, tile->width, tile->y0, tile->rows, tile->band_height, tile->band_stride};
        uint64_t px = 0;
        for (int j = 0; j < tile->rows; ++j)
            if (tile_row_to_y(tm, j) < params->height) px += (uint64_t)tile->width;
        counts[ORT_COUNT_PIXELS] = px;
    }
    free_buf(tmp);
    return rc;
}

}  // extern "C"
