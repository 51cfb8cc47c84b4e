// Included by ort_kernel.hip after host_frame.inc.  Whole-pixel paths: when a frame takes them
// (use_pixel_paths), the speculation auto-tune's state machine, and render_pixel_paths.
namespace {

// Whole-pixel paths (ort_pixel_paths): the frame in one launch.  Auto (ORT_OPT_PIXEL_PATHS -1):
// frames of more than one traversal per pixel on brute force, and on trees of at most
// kPixelPathsAutoNodes nodes, kPixelPathsAutoNodes5 with 5+ bounces, kPixelPathsAutoNodes8 with
// 8+ -- where the pipeline's per-bounce launches and sorts cost more than its coherence gains.
// The crossover follows the bounces: the pipeline pays a launch, a sort and a copy per bounce
// even when few paths are left, whole-pixel paths only the paths' own work (1080p grid over
// 1.5-11 M nodes x 1-4 samples x 4-16 bounces, profiles/r06/grid/, DESIGN.md 4.4).
constexpr long long kPixelPathsAutoNodes = 1ll << 19;   // any bounce depth
constexpr long long kPixelPathsAutoNodes5 = 1ll << 23;  // maxDepth 5-7
constexpr long long kPixelPathsAutoNodes8 = 1ll << 24;  // maxDepth 8+ (measured to 11 M nodes)
#ifndef ORT_PIXEL_LDS_SCENE_BYTES
#define ORT_PIXEL_LDS_SCENE_BYTES 32768
#endif
constexpr int kPixelLdsSceneBytes = ORT_PIXEL_LDS_SCENE_BYTES;  // LDS-resident scene budget (ort_pixel_paths)
// samples in parallel: device bytes of the per-sample buffers (two end states, the radiance) and
// the per-slot ones (flags, fixup list); frames above the budget run the pixels' chains whole
constexpr size_t kSpecBudget = size_t(8) << 30;
#ifndef ORT_PIXEL_SPEC_CHUNKS
#define ORT_PIXEL_SPEC_CHUNKS 4
#endif
// a pixel's samples in (about) this many chunks of at least kSpecMinChunk samples: a SPEC item
// is one chunk of a block's pixels -- shorter chains with more chunks, but each item starts with
// a load of its state and a refill (one-sample chunks: 4 x 4 on 10 spheres at 1080p 0.55 ->
// 1.69 ms; config.h's 16 x 8 in 2 / 4 / 8 chunks: 1.46 / 1.77 / 1.60x, profiles/r06/ab_spec_*)
constexpr int kSpecChunks = ORT_PIXEL_SPEC_CHUNKS;
constexpr int kSpecMinChunk = 4;
inline int spec_chunk(int ns) { return std::max(kSpecMinChunk, (ns + kSpecChunks - 1) / kSpecChunks); }
inline int spec_nch(int ns) { return (ns + spec_chunk(ns) - 1) / spec_chunk(ns); }
#ifndef ORT_PIXEL_SPEC_MOVED_MAX
#define ORT_PIXEL_SPEC_MOVED_MAX 1000
#endif
constexpr long long kSpecMovedMax = ORT_PIXEL_SPEC_MOVED_MAX;
constexpr float kSpecAutoGain = 1.0f;           // auto keeps speculating when it ran at most this x the whole-chain frame
constexpr long long kSpecAutoPixels = 1 << 20;  // ... and without timing events, on frames of at most this many pixels
inline size_t spec_bytes(size_t slots, int ns) { return slots * ((size_t)spec_nch(ns) * 16 + (size_t)ns * 12 + 28); }

bool use_pixel_paths(const ort_ctx* ctx, int mode, int ns, int maxd) {
    if (mode == 1 || maxd < 1 || (ns == 1 && maxd == 1) || ctx->opt.pixel_paths == 0) return false;
    if (ctx->opt.pixel_paths > 0) return true;
    // 1080p, whole-pixel paths over the pipeline: 8 bounces 1.02-1.50x from 1.5 to 11 M nodes
    // (1 to 4 samples), 5 bounces 1.09-1.10x to 5 M, 1.00x at 8.3 M, 0.95x at 11 M; 4 bounces
    // 0.74-1.02x from 1.5 M nodes on, 1.09x at 209 k (profiles/r06/grid/)
    const long long limit = maxd >= 8 ? kPixelPathsAutoNodes8 : (maxd >= 5 ? kPixelPathsAutoNodes5 : kPixelPathsAutoNodes);
    return mode == 2 || ctx->scene.n_nodes <= limit;
}

// The dynamic LDS of an ort_pixel_paths launch on ctx's scene, and whether the scene itself lives
// there (lds_scene; then a's lds_* fields say where).
size_t pixel_paths_lds(const ort_ctx* ctx, int mode, PipeArgs& a, bool& lds_scene) {
    size_t lds = mode == 0 ? lds_bytes(0, ctx->scene.depth, true) : 0;
    // an LDS-resident scene: node records + kid entries (16 B per node) and the leaf spheres
    // (16 B per entry: objectIndices, then the per-sphere tail), when they fit the budget
    const size_t nk_b = 16 * (size_t)ctx->scene.n_nodes, sph_b = 16 * ((size_t)ctx->scene.n_indices + (size_t)ctx->scene.n_spheres);
    lds_scene = mode == 0 && ctx->scene.depth <= 8 && a.S.nk && ctx->opt.pixel_lds_scene && nk_b + sph_b <= (size_t)kPixelLdsSceneBytes;
    if (lds_scene) {
        a.lds_nk_off = (int)align16(lds);
        a.lds_sph_off = (int)(a.lds_nk_off + nk_b);
        a.lds_nk_n16 = (int)(nk_b / 16);
        a.lds_sph_n16 = (int)(sph_b / 16);
        lds = (size_t)a.lds_sph_off + sph_b;
    }
    return lds;
}

// What a whole-pixel frame does with its pixels' chains: runs them whole; runs them whole and records
// the samples' end states for a later speculating frame; or runs the samples' chunks in parallel
// from the last frame's states (three launches: the samples, the resolve, the fixup list).
enum class SpecFrame { Whole, Recording, Speculating };

// The speculation auto-tune, first half: what kind of frame is this one?  (The state buffers are
// there.)  A new shape starts over with an empty fixup list; measured frames whose timing slots the
// ring is about to reuse are measured again; auto mode decides from the two measured frames once
// both have completed; and auto mode's frame after the warm-up runs whole, to be measured.
int spec_classify(ort_ctx* ctx, unsigned long long sig, bool timed, long long pixels, hipStream_t s, SpecFrame& kind) {
    Speculation& sp = ctx->spec;
    const TimingRing& ring = ctx->ring;
    const int opt = ctx->opt.pixel_spec;
    if (sp.sig != sig) {  // a fresh start: an empty fixup list, nothing moved
        HIPCHK(ctx, hipMemsetAsync(sp.fixn.p, 0, 64, s));
        sp.tune = SpecTune::Fresh;
        // untimed contexts cannot compare: speculate on frames of at most kSpecAutoPixels
        sp.use = opt > 0 || timed || pixels <= kSpecAutoPixels;
    }
    if ((sp.tune == SpecTune::WholeMeasured || sp.tune == SpecTune::SpecMeasured) && ring.frames - sp.tframe >= TimingRing::kRing - 2)
        sp.tune = SpecTune::WarmedUp;  // the measured frames' timing slots are being reused: measure again
    if (opt < 0 && sp.tune == SpecTune::SpecMeasured) {  // auto: a measured whole-chain frame against a measured SPEC frame
        float tw = 0.0f, tsp = 0.0f, x = 0.0f;
        bool ok = hipEventQuery(ring.tr1[sp.tslot[1]][2]) == hipSuccess;
        for (int j = 0; ok && j < 3; ++j) {
            ok = ring.elapsed(sp.tslot[1], j, &x, false) == hipSuccess;
            tsp += x;
        }
        if (ok) ok = ring.elapsed(sp.tslot[0], 0, &tw, false) == hipSuccess;
        if (ok) {
            sp.use = tsp < kSpecAutoGain * tw;
            sp.tune = SpecTune::Decided;
        }
    }
    const bool spec_frame = sp.sig == sig && sp.use &&
                            !(opt < 0 && timed && sp.tune == SpecTune::WarmedUp);  // auto: the measured whole-chain frame
    // (Whole: auto found speculation slower on this shape: no recording)
    kind = spec_frame ? SpecFrame::Speculating : (sp.use ? SpecFrame::Recording : SpecFrame::Whole);
    return ORT_OK;
}

// ... second half: a frame of this kind was just enqueued, timed, in ring slot fslot.  The first
// frame of each kind warms up; the next of each kind is that side's measurement.
void spec_note(Speculation& sp, const TimingRing& ring, SpecFrame kind, int fslot) {
    if (kind == SpecFrame::Recording && sp.tune == SpecTune::Fresh) {
        sp.tune = SpecTune::FirstDone;  // auto: a shape's first frame (not measured)
    } else if (kind == SpecFrame::Recording && sp.tune == SpecTune::WarmedUp) {  // auto: this frame's time is the whole-chain side
        sp.tslot[0] = fslot;
        sp.tframe = ring.frames;
        sp.tune = SpecTune::WholeMeasured;
    } else if (kind == SpecFrame::Speculating && sp.tune == SpecTune::FirstDone) {
        sp.tune = SpecTune::WarmedUp;  // auto: the first speculating frame (not measured)
    } else if (kind == SpecFrame::Speculating && sp.tune == SpecTune::WholeMeasured) {  // auto: ... and this one's the speculating side
        sp.tslot[1] = fslot;
        sp.tune = SpecTune::SpecMeasured;
    }
}

// What render_pixel_paths' steps share about the frame.
struct PixelFrame {
    long long blocks;
    size_t slots;  // a.total
    int ns, nch;   // samples, and the chunks they run in when speculating
    unsigned long long sig;
    bool timed;    // per-launch events
    SpecFrame kind = SpecFrame::Whole;
    float2 *sp_prev = nullptr, *sp_cur = nullptr;  // last frame's end states and this frame's
    bool deep = false, lds_scene = false;
    size_t lds = 0;
    int fslot = 0;  // the frame's timing slot
};

// Samples in parallel (ORT_OPT_PIXEL_SPECULATE, ort_pixel_paths<..., SPEC>): from the second
// frame of a shape on, when the per-sample state buffers fit kSpecBudget; the first frame
// runs the pixels' chains whole and records their samples' end states.  spec_on: the buffers fit;
// f.kind: what this frame does (spec_classify).
int spec_setup(ort_ctx* ctx, const ort_tile* t, PipeArgs& a, PixelFrame& f, hipStream_t s, bool& spec_on) {
    Speculation& sp = ctx->spec;
    spec_on = ctx->opt.pixel_spec != 0 && f.nch > 1 && spec_bytes(f.slots, f.ns) <= kSpecBudget;
    if (!spec_on) {
        sp.sig = 0;
        return ORT_OK;
    }
    int rc;
    const void* had = sp.st.p;
    if ((rc = ensure(ctx, sp.st, 2 * sizeof(float2) * (size_t)f.nch * f.slots)) ||
        (rc = ensure(ctx, sp.col, 3 * sizeof(float) * (size_t)f.ns * f.slots)) ||
        (rc = ensure(ctx, sp.fix, (2 * sizeof(int) + sizeof(float2) + 3 * sizeof(float)) * f.slots)) ||
        (rc = ensure(ctx, sp.fixn, 64)))
        return rc;
    if (sp.st.p != had) sp.sig = 0;  // reallocated: no recorded states
    if ((rc = spec_classify(ctx, f.sig, f.timed, (long long)t->width * t->rows, s, f.kind))) return rc;
    a.sp_ctl = (int*)sp.fixn.p;
    float2* st0 = (float2*)sp.st.p;
    f.sp_prev = sp.par ? st0 + (size_t)f.nch * f.slots : st0;
    f.sp_cur = sp.par ? st0 : st0 + (size_t)f.nch * f.slots;
    a.sp_chunk = spec_chunk(f.ns);
    a.sp_nch = f.nch;
    return ORT_OK;
}

// Heavy blocks first (ORT_OPT_PIXEL_HEAVY_FIRST; auto: several samples -- a pixel's chain is
// then long enough for the frame's tail to matter, while one-sample frames keep tile order's
// locality: 1080p 1 x 4 on 10k spheres 0.89x in heavy-first order, profiles/r06/ab_blk_*);
// not in a frame of parallel samples (nothing there is as long as a pixel's chain)
int pixel_lists_setup(ort_ctx* ctx, const ort_params* p, PipeArgs& a, const PixelFrame& f, hipStream_t s) {
    PixelLists& pp = ctx->pp;
    const bool spec_frame = f.kind == SpecFrame::Speculating;
    const bool heavy_first = !spec_frame &&
                             (ctx->opt.pixel_heavy_first > 0 || (ctx->opt.pixel_heavy_first < 0 && p->num_samples > 1));
    if (!heavy_first && !spec_frame) pp.sig = 0;
    if (!heavy_first) return ORT_OK;
    // last frame's class lists (same shape) and this frame's
    const size_t nb = (size_t)f.blocks * (kBlock / 64), cnt_b = 2 * kPixelClasses * sizeof(int);
    int rc;
    if ((rc = ensure(ctx, pp.list, 2 * kPixelClasses * 4 * nb)) || (rc = ensure(ctx, pp.cnt, cnt_b)) ||
        (rc = ensure(ctx, pp.cost, 8 * nb)))
        return rc;
    if (pp.sig == 0 || pp.sig != f.sig) {  // no lists of this shape: zero counts and accumulators
        HIPCHK(ctx, hipMemsetAsync(pp.cnt.p, 0, cnt_b, s));
        HIPCHK(ctx, hipMemsetAsync(pp.cost.p, 0, 8 * nb, s));
    }
    const int w = pp.par, r = w ^ 1;
    int* lists = (int*)pp.list.p;
    int* cnt = (int*)pp.cnt.p;
    a.pl_stride = (int)nb;
    a.pl_w = lists + (size_t)w * kPixelClasses * nb;
    a.pl_wcnt = cnt + kPixelClasses * w;
    a.pl_rcnt = cnt + kPixelClasses * r;
    a.pl_cost = (unsigned long long*)pp.cost.p;
    a.pl_r = (pp.sig == f.sig) ? lists + (size_t)r * kPixelClasses * nb : nullptr;
    pp.par = r;
    pp.sig = f.sig;
    return ORT_OK;
}

// Every pixel's whole chain in one launch (recording its samples' end states in a Recording frame),
// then how many pixels moved since the last frame.
int launch_whole_frame(ort_ctx* ctx, int mode, PipeArgs& a, const PixelFrame& f, hipStream_t s) {
    Speculation& sp = ctx->spec;
    a.sp_cur = f.sp_cur;
    const bool rec = f.kind == SpecFrame::Recording;
    const hipError_t e = launch_pixel_paths(rec ? 2 : 0, ctx->device, mode, f.deep, f.lds_scene, f.lds, f.blocks, a, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_pixel_paths launch");
    if (f.timed) HIPCHK(ctx, ctx->ring.end(f.fslot, 0, s));
    if (rec && f.timed) spec_note(sp, ctx->ring, f.kind, f.fslot);
    if (rec && sp.sig == f.sig) {  // how many pixels moved since last frame (mode word 0: count)
        int* cnt = (int*)sp.fixn.p + 1;
        a.sp_prev = f.sp_prev;
        HIPCHK(ctx, hipMemsetAsync(cnt, 0, 2 * sizeof(int), s));
        hipLaunchKernelGGL(ort_sample_moved, dim3((unsigned)((f.slots + 255) / 256)), dim3(256), 0, s, a, cnt);
        hipError_t e2;
        if ((e2 = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e2, "ort_sample_moved launch");
    }
    return ORT_OK;
}

// The samples' chunks in parallel, the resolve, the fixup list, the count of the pixels that moved.
int launch_spec_frame(ort_ctx* ctx, const ort_tile* t, int mode, PipeArgs& a, const PixelFrame& f, hipStream_t s) {
    Speculation& sp = ctx->spec;
    TimingRing& ring = ctx->ring;
    const size_t slots = f.slots;
    int* fx = (int*)sp.fix.p;
    a.sp_prev = f.sp_prev;
    a.sp_cur = f.sp_cur;
    a.sp_col = (float*)sp.col.p;
    a.fx_n = (int*)sp.fixn.p;
    a.fx_slot = fx;
    a.fx_s0 = fx + slots;
    a.fx_st = (float2*)(fx + 2 * slots);
    a.fx_col = (float*)(fx + 4 * slots);
    PipeArgs as = a;  // the samples: no fixup list; heavy blocks first by the lists the last
    as.fx_slot = nullptr;  // whole-chain frame of this shape wrote (read only: SPEC frames keep them)
    if (ctx->pp.sig == f.sig && ctx->pp.list.p) {
        const size_t nbk = (size_t)f.blocks * (kBlock / 64);
        const int r = ctx->pp.par ^ 1;
        as.pl_stride = (int)nbk;
        as.pl_r = (int*)ctx->pp.list.p + (size_t)r * kPixelClasses * nbk;
        as.pl_rcnt = (int*)ctx->pp.cnt.p + kPixelClasses * r;
    }
    hipLaunchKernelGGL(ort_sample_decide, dim3(1), dim3(64), 0, s, a.sp_ctl, (long long)t->width * t->rows, kSpecMovedMax);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_sample_decide launch");
    e = launch_pixel_paths(1, ctx->device, mode, f.deep, f.lds_scene, f.lds, f.blocks * f.nch, as, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_pixel_paths (samples) launch");
    if (f.timed) HIPCHK(ctx, ring.end(f.fslot, 0, s));
    if (f.timed) HIPCHK(ctx, ring.begin(f.fslot, 1, s));
    hipLaunchKernelGGL(ort_sample_resolve, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_sample_resolve launch");
    if (f.timed) HIPCHK(ctx, ring.end(f.fslot, 1, s));
    if (f.timed) HIPCHK(ctx, ring.begin(f.fslot, 2, s));
    // the fixup list (the workgroups beyond what it needs leave at once); in a fall-back frame
    // every pixel's chain, then the count of the pixels that moved
    e = launch_pixel_paths(2, ctx->device, mode, f.deep, f.lds_scene, f.lds, f.blocks, a, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "ort_pixel_paths (fixup) launch");
    if (f.timed) HIPCHK(ctx, ring.end(f.fslot, 2, s));
    hipLaunchKernelGGL(ort_sample_moved, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, a, a.sp_ctl + 1);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "ort_sample_moved launch");
    if (f.timed) spec_note(sp, ring, f.kind, f.fslot);
    return ORT_OK;
}

// The frame as one ort_pixel_paths launch (use_pixel_paths); dout: the frame on the device.
// Classify the frame, set up its buffers and lists, launch one of the two shapes of frame, note it.
int render_pixel_paths(ort_ctx* ctx, const ort_params* p, const ort_tile* t, int mode, const DevOutput& dout,
                       hipStream_t s) {
    const int tilesX = (t->width + 15) / 16, tilesY = (t->rows + 15) / 16;
    PixelFrame f;
    f.blocks = (long long)tilesX * tilesY;
    PipeArgs a = base_args(ctx, p, t, dout, tilesX, tilesY, f.blocks);
    // the cursor and done count: this frame's counter set (zero; the kernel's last workgroup
    // zeroes them again, so the set stays the pipeline's next one)
    int rc;
    bool fresh;
    if ((rc = begin_counter_sets(ctx, s, fresh))) return rc;
    if (fresh) ctx->pp.sig = 0;  // (the class lists' counts re-zeroed below)
    a.sync = (int*)ctx->pipe.defer_count.p + 16 * ctx->pipe.sync_set;
    f.sig = frame_sig(ctx, p, t);
    f.ns = p->num_samples;
    f.slots = (size_t)a.total;
    f.nch = spec_nch(f.ns);
    f.timed = !((ctx->opt.debug_flags & 1) || !ctx->opt.launch_times);
    bool spec_on;
    if ((rc = spec_setup(ctx, t, a, f, s, spec_on)) || (rc = pixel_lists_setup(ctx, p, a, f, s))) return rc;
    const bool spec_frame = f.kind == SpecFrame::Speculating;
    f.deep = ctx->scene.depth > 8;
    f.lds = pixel_paths_lds(ctx, mode, a, f.lds_scene);
    TimingRing& ring = ctx->ring;
    f.fslot = ring.slot();
    ring.tseg[f.fslot] = 0;
    const int nseg = spec_frame ? 3 : 1;  // SPEC: the samples, the resolve, the fixup list
    for (int j = 0; f.timed && j < nseg; ++j) HIPCHK(ctx, ring.create(f.fslot, j));
    ring.ev0_last = f.timed ? ring.tr0[f.fslot][0] : ctx->frame_ev.ev0;  // the frame's start is its trace launch's
    HIPCHK(ctx, hipEventRecord(ring.ev0_last, s));
    if ((rc = spec_frame ? launch_spec_frame(ctx, t, mode, a, f, s) : launch_whole_frame(ctx, mode, a, f, s))) return rc;
    if (spec_on) {  // this frame's end states are the next frame's
        ctx->spec.par ^= 1;
        ctx->spec.sig = f.sig;
    }
    if (f.timed) {
        ring.tseg[f.fslot] = nseg;
        ring.frames += 1;
    }
    HIPCHK(ctx, ctx->frame_ev.end(s));
    ctx->pipe.sync_ok = true;
    return ORT_OK;
}

}  // namespace
