// Included by ort_kernel.hip after its kernels.  The context: ort_ctx's state grouped by owner, each
// group declared and documented here with the one list of its device buffers; the error and buffer
// helpers; ort_create, ort_destroy, ort_set_option.
namespace {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

void free_buf(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

// A group keeps its device buffers in a base struct of DevBuf members only and lists them once,
// next to that struct, in an each_*buffer visitor built on this: the assertion fails when a buffer
// is declared and not listed (what frees a group frees exactly the list).
template <class Buffers, class F, class... B>
void visit_buffers(F f, B&... b) {
    static_assert(sizeof(Buffers) == sizeof...(B) * sizeof(DevBuf), "the group's list names every DevBuf it declares");
    (f(b), ...);
}

// Two timing events around one piece of enqueued work and whether they have been recorded: the
// frame's (ort_ctx::frame_ev), a query's, a denoise's, an accumulation pass's.
struct EventPair {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    hipError_t create() {  // on first use (ort_create and ort_accum_begin: up front)
        hipError_t e = ev0 ? hipSuccess : hipEventCreate(&ev0);
        if (e == hipSuccess && !ev1) e = hipEventCreate(&ev1);
        return e;
    }
    hipError_t begin(hipStream_t s) { return hipEventRecord(ev0, s); }
    hipError_t end(hipStream_t s) {
        const hipError_t e = hipEventRecord(ev1, s);
        if (e == hipSuccess) timed = true;
        return e;
    }
    // waits for the end; from: the start when it is another event than ev0 (TimingRing::ev0_last)
    hipError_t elapsed(float* ms, hipEvent_t from = nullptr) {
        const hipError_t e = hipEventSynchronize(ev1);
        return e != hipSuccess ? e : hipEventElapsedTime(ms, from ? from : ev0, ev1);
    }
    void destroy() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        *this = EventPair{};
    }
};

// The frame timing ring: the trace launches of the last kRing timed frames, kSeg segments (launches)
// a frame at most.  A frame takes slot(); its segments are begun and ended in order, and the frame
// counts (frames) once it has timed one.
struct TimingRing {
    static constexpr int kRing = 64;  // trace-kernel timing of the last 64 frames
    static constexpr int kSeg = 16;   // ... of their first 16 trace launches each
    hipEvent_t tr0[kRing][kSeg] = {}, tr1[kRing][kSeg] = {};  // segment 0 created up front, others lazily
    int tseg[kRing] = {};             // trace launches timed in each frame slot
    long long frames = 0;             // frames whose first trace kernel was timed
    hipEvent_t ev0_last = nullptr;    // the last frame's start: the frame's ev0, or its first trace-timing event
    int slot() const { return (int)(frames % kRing); }
    hipError_t create(int slot, int j) {  // segment j's events, on first use
        if (tr0[slot][j]) return hipSuccess;
        const hipError_t e = hipEventCreate(&tr0[slot][j]);
        return e != hipSuccess ? e : hipEventCreate(&tr1[slot][j]);
    }
    // begin segment j of the slot's frame.  record false: the frame's start event already is this
    // segment's start (ev0_last == tr0[slot][0], nothing enqueued between them), which saves an
    // event packet per frame (~1 % of a 1/8 band frame)
    hipError_t begin(int slot, int j, hipStream_t s, bool record = true) {
        const hipError_t e = create(slot, j);
        return e != hipSuccess || !record ? e : hipEventRecord(tr0[slot][j], s);
    }
    hipError_t end(int slot, int j, hipStream_t s) { return hipEventRecord(tr1[slot][j], s); }
    // how many of the last n timed frames the ring still holds, and the slot of the i-th of those k
    int held(int n) const { return (int)std::min<long long>(n, std::min<long long>(frames, kRing)); }
    int slot_of(int k, int i) const { return (int)((frames - k + i) % kRing); }
    hipError_t elapsed(int slot, int j, float* ms, bool wait = true) const {  // segment j's time
        const hipError_t e = wait ? hipEventSynchronize(tr1[slot][j]) : hipSuccess;
        return e != hipSuccess ? e : hipEventElapsedTime(ms, tr0[slot][j], tr1[slot][j]);
    }
    void destroy() {
        for (int i = 0; i < kRing; ++i)
            for (int j = 0; j < kSeg; ++j) {
                if (tr0[i][j]) (void)hipEventDestroy(tr0[i][j]);
                if (tr1[i][j]) (void)hipEventDestroy(tr1[i][j]);
            }
    }
};

// The queries' own state (ort_trace_rays, ort_trace_rays_ex, ort_trace_camera: ray_query.inc), none of
// the per-frame pipeline's: the staging of host arrays (grow-only; trange: ort_trace_rays_ex's
// intervals; states, radiance: ort_trace_radiance's), the defer list and the {deferred count, cursor} counters, ORT_QUERY_SORT's keys and
// lists, the timing events of the last query.
struct QueryBuffers {
    DevBuf rays, hits, normals, trange, states, radiance;
    DevBuf defer, sync;
    DevBuf keys, keys2, vals, list, temp;
};
struct QueryState : QueryBuffers {
    EventPair ev;
};
template <class F>
void each_buffer(QueryBuffers& q, F f) {
    visit_buffers<QueryBuffers>(f, q.rays, q.hits, q.normals, q.trange, q.states, q.radiance, q.defer, q.sync, q.keys, q.keys2,
                                q.vals, q.list, q.temp);
}

// The denoiser's own state (ort_denoise: denoise.inc), none of the queries' or the pipeline's: the
// staging of host arrays and of a host output (grow-only), the packed guide records, the two
// colour buffers the iterations ping-pong between, the timing events of the last denoise.
struct DenoiseBuffers {
    DevBuf in_color, in_hits, in_normals, out;
    DevBuf guide, col_a, col_b;
    DevBuf in_var, var_a, var_b;  // ort_denoise_ex: the staged variance plane and the two the iterations ping-pong between
};
struct DenoiseState : DenoiseBuffers {
    EventPair ev;
};
template <class F>
void each_buffer(DenoiseBuffers& d, F f) {
    visit_buffers<DenoiseBuffers>(f, d.in_color, d.in_hits, d.in_normals, d.out, d.guide, d.col_a, d.col_b, d.in_var,
                                  d.var_a, d.var_b);
}

#ifndef ORT_HEAVY_STEPS
#define ORT_HEAVY_STEPS 64  // ORT_OPT_HEAVY_FIRST default: classes >= 256, >= 128, >= 64 steps
#endif
// Camera-ray defaults, measured with tools/ab_stream.py (DESIGN.md 4): a raised issue priority
// for waves holding a >= 150-step walk (C3 1/8 band +15 %, full frame +-0); split walks of the
// >= 200-step rays on tiles of at most 2^21 pixels (C3 1/8 band +26 %, 1/4 band +21 %, 1/2 band
// -2 %, full frame -2 %) and tile pairs on the larger ones (full frame +1.2 %, 1/2 band +0.8 %;
// 1/4 band: split +21 % > pairs +16 %; 1/8 band: pairs with split -22 %).
constexpr int kHeavyPrioSteps = 150;
constexpr int kSplitAutoSteps = 200;
constexpr long long kSplitAutoPixels = 1ll << 21;
constexpr long long kPairsAutoPixels = kSplitAutoPixels + 1;
// ORT_OPT_XCD_SWIZZLE -1 (auto): raster order (0) for the per-tile kernel on tiles of at most
// this many pixels, runs (2) otherwise.  A C3 1/8 band (1 M pixels, ~2 generations of
// workgroups) at one frame in flight: 0.307 -> 0.298 ms with raster order (its heavy region
// spread over all 8 XCDs instead of runs of 16 tiles on one); a 1/4 band 0.492 vs 0.505 and
// tile pairs (frames in flight) 0.224 vs 0.242 ms the other way (profiles/r05_band_swizzle.log)
constexpr long long kRasterAutoPixels = 3ll << 19;

// What ort_set_option sets (kOptions: one row per ranged option).
struct Options {
    int force_layout = -1;
    int exact_only = 0;
    int pixel_paths = -1;  // ORT_OPT_PIXEL_PATHS: -1 auto (use_pixel_paths), 0 off, 1 on where it applies
    int pixel_lds_scene = 1;  // ORT_OPT_PIXEL_LDS_SCENE: small scenes in LDS for whole-pixel paths
    int pixel_heavy_first = -1;  // ORT_OPT_PIXEL_HEAVY_FIRST: -1 auto (2+ samples), 0 off, 1 on
    int pixel_spec = -1;  // ORT_OPT_PIXEL_SPECULATE: -1 auto, 0 off, 1 on
    int refill = 16;  // ORT_OPT_REFILL: C5 (64-item chunks) 16 > 12 (-0.6 %) > 8 (-1.2 %); tools/ab_stream.py
    int persistent = 2;  // ORT_OPT_PERSISTENT: 0 off, 2 bounce >= 1 traces (default)
    int xcd_swizzle = -1;  // ORT_OPT_XCD_SWIZZLE: workgroup -> tile order (block_tile); -1 auto
    int kid_skip = 1;     // ORT_OPT_KID_SKIP: rejected-sphere skip of one-sphere leaf children (2: without nk)
    // ORT_OPT_SORT_PATHS: order of the alive paths between bounces.  2 (default): the list the
    // shade kernel appended, radix-sorted by the coherence key after reading its length back --
    // C5 bounce traces 33.8 -> 31.2 ms, frame 55.5 -> 54.9 ms (A/B).  1 (every slot's key sorted,
    // dead ones last) costs as much as it saves; coarser orders lose: octant only or 12-18 key
    // bits ~ slot order, octant + direction bits and 16-bit atomic buckets slower than slot
    // order, a block-local sort of 4096-entry runs (rocprim block_radix_sort) 55.4 ms.
    int sort_paths = 2;
    int sort_bound = 0;  // ORT_OPT_SORT_BOUND (testing): > 0 forces this bound
    // ORT_OPT_COST_ORDER (cost_order_slot): per slot the walk steps of its last camera ray
    // (CostOrder::pcost)
    int cost_order = 1;
    // ORT_OPT_HEAVY_FIRST: threshold in walk steps (0 off; CostOrder::bcost)
    int heavy_first = ORT_HEAVY_STEPS;
    int heavy_prio = kHeavyPrioSteps;  // ORT_OPT_HEAVY_PRIO (steps; 0 off)
    // ORT_OPT_TILE_PAIRS: camera-ray workgroups of two tiles (cost_order_pair); -1 = auto (tiles
    // of at least kPairsAutoPixels)
    int tile_pairs = -1;
    // ORT_OPT_SPLIT_HEAVY (steps; 0 off; -1 = auto: kSplitAutoSteps on tiles of at most
    // kSplitAutoPixels) / ORT_OPT_SPLIT_LEVEL (0: auto): the heavy camera rays of a 1-sample
    // frame walked by ort_trace_split on SplitWalks::aux_stream (k_heavy_scan lists them)
    int split_steps = -1;
    int split_level = 0;
    int debug_flags = 0;   // ORT_OPT_DEBUG_FLAGS (A/B of the per-frame stream structure only)
    int launch_times = 1;  // ORT_OPT_LAUNCH_TIMES: per-launch trace-timing events
};

// The scene on the device: the spheres, the tree in one of the two layouts, and what describes it.
struct SceneBuffers {
    DevBuf sph_cr, sph_ma, sph_fr;
    DevBuf node, leaf_sph, leaf_idx, planes, kid;  // compact
    DevBuf nk;                                   // ... node records and kid entries interleaved (build_nk)
    DevBuf leaf16;                               // ... depth <= 8: the 16-byte leaf records (build_leaf16)
    DevBuf cam_node;                             // ... depth <= 8: node[] with the repeat masks (build_cam_node)
    DevBuf lds_img;                              // compact: the workgroup LDS image (k_lds_image)
    DevBuf lds_rev;                              // ... depth 9-10: the reversed-table image (persistent kernel)
    DevBuf nodeA, nodeB, cnt, indices;           // explicit
};
struct Scene : SceneBuffers {
    float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};  // root box (coherence-sort key)
    ort::GpuTree tree;  // reference-layout tree of the last ort_build_scene(keep_tree)
    float build_ms = 0.0f;
    bool has_scene = false;
    int layout = ORT_LAYOUT_EXPLICIT;
    int depth = 0;
    bool ordered = true;  // compact layout: fast walk allowed (CompactLayout::ordered)
    int32_t n_spheres = 0, n_nodes = 0;
    int64_t n_indices = 0;
    // the scene's generation: free_scene advances it, and an accumulation begun or restarted under
    // another one is stale
    unsigned long long scene_gen = 0;
};
// The scene's device buffers (C: SceneBuffers or const SceneBuffers): the one list free_scene frees
// and ort_scene_get_info sums.
template <class C, class F>
void each_scene_buffer(C& c, F f) {
    visit_buffers<SceneBuffers>(f, c.sph_cr, c.sph_ma, c.sph_fr, c.node, c.kid, c.nk, c.leaf16, c.cam_node, c.leaf_sph, c.leaf_idx, c.planes,
                                c.lds_img, c.lds_rev, c.nodeA, c.nodeB, c.cnt, c.indices);
}

// The wavefront pipeline (render_impl): a host output's scratch frame and ort_count_traffic's
// counters; the path state, sized for the largest tile rendered so far; the counter sets; the
// compaction lists; the coherence sort and its list-length hints.
struct PipelineBuffers {
    DevBuf scratch_out, counters;
    DevBuf hit, defer_list, defer_count, po, pd, pc, prng, pcol;
    DevBuf qlist, qlist2, qcount, qtemp;  // bounce >= 1 path compaction (two lists: read one, append the other)
    DevBuf skeys, skeys2, svals;  // coherence sort
    DevBuf key_spread;            // its origin-code tables for the scene's root box (path_key.h)
};
struct Pipeline : PipelineBuffers {
    int sync_set = 0;      // defer_count's counter set of the next trace launch (render_impl)
    bool sync_ok = false;  // both sets zero except the one the last exact kernel left to zero
    float spread_box[6] = {0, 0, 0, 0, 0, 0};  // the root box key_spread was built for
    // The list sort without a host wait (sortListBounded): its size is a host-side bound, the
    // list's length from the same bounce of an earlier frame (read back asynchronously into
    // pinned memory: alive_host[sample * bounces + bounce]) plus a margin; a longer list goes
    // on unsorted (same pixels).  hint_sig: the frame shape the hints belong to.  The hints live
    // in one of kHintBanks banks: a new shape takes a bank that no copy is still headed for (the
    // event after the bank's last copy has completed), so a copy of the old shape's frames
    // still in flight cannot land in the new shape's hints.
    static constexpr int kHints = 64;
    static constexpr int kHintBanks = 4;
    int* alive_host = nullptr;         // kHintBanks x kHints
    int hint_bank = 0;
    hipEvent_t hint_ev[kHintBanks] = {};
    bool hint_ev_used[kHintBanks] = {};
    unsigned long long hint_sig = 0;
};
template <class F>
void each_buffer(PipelineBuffers& b, F f) {
    visit_buffers<PipelineBuffers>(f, b.scratch_out, b.counters, b.hit, b.defer_list, b.defer_count, b.po, b.pd, b.pc, b.prng,
                                   b.pcol, b.qlist, b.qlist2, b.qcount, b.qtemp, b.skeys, b.skeys2, b.svals, b.key_spread);
}

// Cost order and heavy first: pcost, per slot the walk steps of its last camera ray, cleared when
// the frame shape or scene changes (cost_sig); bcost, per bounce >= 1 of the first kCostBounces of a
// frame, every slot's last walk steps (cleared with bcost_sig).
struct CostBuffers {
    DevBuf pcost, bcost;
};
struct CostOrder : CostBuffers {
    static constexpr int kCostBounces = 8;
    unsigned long long cost_sig = 0, bcost_sig = 0;
    ort::KCamera prio_cam{};  // the camera of this context's last frame (heavy priority: static only)
};
template <class F>
void each_buffer(CostBuffers& b, F f) {
    visit_buffers<CostBuffers>(f, b.pcost, b.bcost);
}

// Split walks: the heavy camera rays of a 1-sample frame on a second stream.
struct SplitBuffers {
    DevBuf hcnt;  // two {heavy count, split cursor} pairs (16 ints): ort_trace_split zeroes the other
    DevBuf hbits, hlist;
};
struct SplitWalks : SplitBuffers {
    static constexpr int kSplitCap = 4096;  // heavy rays listed per frame at most
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_scan = nullptr, ev_split = nullptr, ev_pre = nullptr;
    // the next frame's heavy list is listed by a split frame's exact kernel (pcost final by then)
    // instead of by a scan opening the next frame: pre_ok when the list in hbits/hlist/hcnt[hpar]
    // is that of a frame of shape pre_sig and threshold pre_steps
    bool pre_ok = false;
    unsigned long long pre_sig = 0;
    int pre_steps = 0, hpar = 0;
};
template <class F>
void each_buffer(SplitBuffers& b, F f) {
    visit_buffers<SplitBuffers>(f, b.hbits, b.hlist, b.hcnt);
}

// Whole-pixel paths, heavy blocks first: two {kPixelClasses segments of block lists} buffers
// and their counts, the blocks' cost accumulators, the parity of the next frame's write
// buffer, and the shape the read buffer's lists belong to (0: none)
struct PixelListBuffers {
    DevBuf list, cnt, cost;
};
struct PixelLists : PixelListBuffers {
    int par = 0;
    unsigned long long sig = 0;
};
template <class F>
void each_buffer(PixelListBuffers& b, F f) {
    visit_buffers<PixelListBuffers>(f, b.list, b.cnt, b.cost);
}

// ORT_OPT_PIXEL_SPECULATE auto (-1): per shape, a whole-chain frame's time against a speculating
// frame's decides Speculation::use (spec_classify, spec_note: host_pixel_paths.inc).
enum class SpecTune {
    Fresh,          // nothing of this shape rendered
    FirstDone,      // first frame done
    WarmedUp,       // first speculating frame done (warm-up of both)
    WholeMeasured,  // whole-chain frame measured
    SpecMeasured,   // speculating frame measured
    Decided,
};

// Samples in parallel (ORT_OPT_PIXEL_SPECULATE): the two per-chunk end-state buffers (st,
// which one is last frame's: par), the samples' radiance, the fixup list and its length,
// and the shape the recorded states belong to (0: none)
// (the pixels a frame found moved, and whether the next one speculates: fixn, PipeArgs::sp_ctl)
struct SpecBuffers {
    DevBuf st, col, fix, fixn;
};
struct Speculation : SpecBuffers {
    int par = 0;
    unsigned long long sig = 0;
    SpecTune tune = SpecTune::Fresh;
    int tslot[2] = {0, 0};  // the frame slots (TimingRing) of the measured whole-chain and speculating frames
    long long tframe = 0;   // TimingRing::frames when the whole-chain side was measured
    bool use = true;
};
template <class F>
void each_buffer(SpecBuffers& b, F f) {
    visit_buffers<SpecBuffers>(f, b.st, b.col, b.fix, b.fixn);
}

}  // namespace

struct ort_accum;
struct ort_history;
struct ort_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    Options opt;
#if ORT_ANALYSIS
    void* wclock = nullptr;  // ort_debug_wave_clock (ORT_PERSIST_CLOCK analysis builds)
    long long wclock_n = 0;
#endif
    Scene scene;
    EventPair frame_ev;  // the last frame's start (unless ring.ev0_last is another event) and end
    TimingRing ring;
    Pipeline pipe;
    CostOrder cost;
    SplitWalks split;
    PixelLists pp;
    Speculation spec;
    QueryState query;  // ray, camera and mode queries (ray_query.inc)
    DenoiseState denoise;  // ort_denoise (denoise.inc)
    // accumulations (ort_accum_*, accum.inc): the live ones, each with its own state, counters and
    // events (ort_destroy frees what is left)
    std::vector<ort_accum*> accums;
    // histories (ort_history_*, reproject.inc): the live ones, each with its own records, staging and
    // events (ort_destroy frees what is left)
    std::vector<ort_history*> histories;
};

// A frame's samples accumulated over several passes (include/ort.h): the frame and tile it was
// begun with, the samples done, and per path slot (tile-block order, as PipeArgs::total) the RNG
// state (float2) followed by the colour sum's three planes -- 20 bytes a slot, each array read and
// written by consecutive lanes for consecutive slots.  With ORT_ACCUM_MOMENTS a fourth float plane
// follows them: m2, the sum of the samples' squared luminances (24 bytes a slot).
struct ort_accum {
    ort_ctx* ctx = nullptr;
    ort_params p{};
    ort_tile t{};
    int mode = 0;          // 0 the compact layout's walk, 2 brute force
    int done = 0;
    bool moments = false;  // ORT_ACCUM_MOMENTS: the state carries the m2 plane
    bool adaptive = false; // ORT_ACCUM_ADAPTIVE (implies moments): ... and an int plane, each pixel's count; done is the largest one possible
    long long blocks = 0;  // 16x16 tiles
    unsigned long long scene_gen = 0;
    DevBuf state;          // float2[slots] | float[3][slots] (| float[slots]: m2 (| int[slots]: counts))
    DevBuf sync;           // the launch's cursor and done count (16 ints, zeroed before every pass)
    DevBuf stage;          // host output: the tight picture on the device (allocated by the first such pass)
    DevBuf mstage;         // ort_accum_read_moments into host memory: the mean and the variance, tight
    DevBuf alist;          // adaptive: the slots a pass traces, listed by its pre-pass (allocated by the first pass that may hold pixels)
    DevBuf astage;         // adaptive: ort_accum_read_counts into host memory, and the stats reduction's records
    EventPair ev;
};

// What decides whether an update has a previous frame, and its four transitions (pure host code,
// shared with the test-only ort_debug_history_state).  ort_history_update_ex's ORT_HISTORY_MOTION lets
// a history survive a scene replacement: the replacement leaves it stale, with the updates value it
// had, and a MOTION update revives it if it holds a snapshot of as many spheres as the new scene has.
struct HistoryState {
    long long updates = 0;        // since begin, ort_history_reset or a scene upload (a revival goes on counting)
    bool has_prev = false;
    bool stale = false;           // a scene replacement took a previous frame away ...
    long long stale_updates = 0;  // ... and `updates` was this
    bool has_snap = false;        // the last update was a MOTION update: its scene's spheres are kept ...
    int snap_n = 0;               // ... this many

    void scene_replaced() {
        if (has_prev) {
            stale = true;
            stale_updates = updates;
        }
        has_prev = false;
        updates = 0;
    }
    void forget_motion() { stale = has_snap = false; }  // a plain update, ort_history_reset
    void reset() {
        forget_motion();
        has_prev = false;
        updates = 0;
    }
    // A MOTION update on a scene of n spheres begins: the history revived if it may be.  Returns
    // whether the update reads the snapshot (false: every sphere counts as unmoved).
    bool motion_begin(int n) {
        if (stale && has_snap && snap_n == n) {
            has_prev = true;
            updates = stale_updates;
        }
        stale = false;
        return has_prev && has_snap && snap_n == n;
    }
    void updated() {
        has_prev = true;
        updates += 1;
    }
};

// A preview's history across camera moves (include/ort.h): two ping-pong sets of two 16-byte records
// per pixel -- {r, g, b, n} and {m1, m2, t, sphere} -- the previous update's frame and tile origin,
// and whether there is one.  Host pointers are staged through the history's own buffers.
struct ort_history : HistoryState {
    ort_ctx* ctx = nullptr;
    int width = 0, rows = 0;
    int cur = 0;            // the set the last update wrote
    ort_params prev_p{};
    int prev_x0 = 0, prev_y0 = 0;
    DevBuf rec[2][2];       // [set][0: {r, g, b, n}, 1: {m1, m2, t, sphere}]
    DevBuf in_color, in_rays, in_hits, out_color, out_var, out_len;  // host pointers' staging (grow-only)
    DevBuf snap;            // the snapshot: 16 bytes per sphere, upload order (grow-only; the first MOTION update's)
    EventPair ev;
};

namespace {

int fail(ort_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    ort::set_thread_error(msg);
    return code;
}

int hip_fail(ort_ctx* ctx, hipError_t e, const char* what) {
    return fail(ctx, e == hipErrorOutOfMemory ? ORT_ERR_OUT_OF_MEMORY : ORT_ERR_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(ctx, expr)                                  \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_fail(ctx, _e, #expr); \
    } while (0)

// A group's buffers and events, and the group back to its initial state.
template <class S>
void free_state(S& s) {
    each_buffer(s, [](DevBuf& b) { free_buf(b); });
    s.ev.destroy();
    s = S{};
}

void free_scene(ort_ctx* c) {
    each_scene_buffer(c->scene, [](DevBuf& b) { free_buf(b); });
    ort::freeGpuTree(c->scene.tree);
    c->scene.has_scene = false;
    c->scene.scene_gen += 1;  // the accumulations begun on this scene are stale (accum.inc)
    // ... and sphere ids mean something else: no previous frame, unless a MOTION update vouches for them
    for (ort_history* h : c->histories) h->scene_replaced();
}

template <class F>
void each_history_buffer(ort_history* h, F f) {
    for (auto& set : h->rec)
        for (DevBuf& b : set) f(b);
    f(h->in_color);
    f(h->in_rays);
    f(h->in_hits);
    f(h->out_color);
    f(h->out_var);
    f(h->out_len);
    f(h->snap);
}

// A history's device memory and events, and the object (its context's list is the caller's).
void free_history(ort_history* h) {
    each_history_buffer(h, [](DevBuf& b) { free_buf(b); });
    h->ev.destroy();
    delete h;
}

// An accumulation's device memory and events, and the object (its context's list is the caller's).
void free_accum(ort_accum* a) {
    free_buf(a->state);
    free_buf(a->sync);
    free_buf(a->stage);
    free_buf(a->mstage);
    free_buf(a->astage);
    free_buf(a->alist);
    a->ev.destroy();
    delete a;
}

int upload(ort_ctx* ctx, DevBuf& b, const void* src, size_t bytes) {
    free_buf(b);
    if (bytes == 0) bytes = 16;  // keep a valid pointer for empty arrays
    HIPCHK(ctx, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    if (src) HIPCHK(ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ORT_OK;
}

int ensure(ort_ctx* ctx, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return ORT_OK;
    free_buf(b);
    HIPCHK(ctx, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return ORT_OK;
}

// One row per ranged option: the field it writes, its inclusive range, and what a value outside it
// is answered with.  The options that are not a plain range are ort_set_option's own cases.
struct OptionRow {
    int id;
    int Options::*field;
    int lo, hi;
    const char* bad;
};
const OptionRow kOptions[] = {
    {ORT_OPT_FORCE_LAYOUT, &Options::force_layout, -1, ORT_LAYOUT_EXPLICIT, "bad layout"},
    {ORT_OPT_KID_SKIP, &Options::kid_skip, 0, 2, "ORT_OPT_KID_SKIP: 0, 1 or 2"},
    {ORT_OPT_XCD_SWIZZLE, &Options::xcd_swizzle, -1, 2, "xcd swizzle must be -1 (auto), 0, 1 or 2"},
    {ORT_OPT_SORT_PATHS, &Options::sort_paths, 0, 2, "sort_paths must be 0, 1 or 2"},
    {ORT_OPT_HEAVY_FIRST, &Options::heavy_first, 0, 65535, "ORT_OPT_HEAVY_FIRST: 0 (off) .. 65535 steps"},
    {ORT_OPT_TILE_PAIRS, &Options::tile_pairs, -1, 1, "ORT_OPT_TILE_PAIRS: -1 (auto), 0 or 1"},
    {ORT_OPT_SPLIT_HEAVY, &Options::split_steps, -1, 65535, "ORT_OPT_SPLIT_HEAVY: -1 (auto), 0 (off) .. 65535 steps"},
    {ORT_OPT_SPLIT_LEVEL, &Options::split_level, 0, ORT_COMPACT_MAX_DEPTH, "ORT_OPT_SPLIT_LEVEL: 0 (auto) .. 10"},
    {ORT_OPT_PIXEL_PATHS, &Options::pixel_paths, -1, 1, "ORT_OPT_PIXEL_PATHS: -1 (auto), 0 or 1"},
    {ORT_OPT_PIXEL_SPECULATE, &Options::pixel_spec, -1, 1, "ORT_OPT_PIXEL_SPECULATE: -1 (auto), 0 or 1"},
    {ORT_OPT_PIXEL_HEAVY_FIRST, &Options::pixel_heavy_first, -1, 1, "ORT_OPT_PIXEL_HEAVY_FIRST: -1 (auto), 0 or 1"},
    {ORT_OPT_PIXEL_LDS_SCENE, &Options::pixel_lds_scene, 0, 1, "ORT_OPT_PIXEL_LDS_SCENE: 0 or 1"},
    {ORT_OPT_LAUNCH_TIMES, &Options::launch_times, 0, 1, "ORT_OPT_LAUNCH_TIMES: 0 or 1"},
#if ORT_ANALYSIS  // analysis: 1 no trace-timing events, 2 no queued heavy scan
    {ORT_OPT_DEBUG_FLAGS, &Options::debug_flags, 0, 3, "ORT_OPT_DEBUG_FLAGS: 0 .. 3"},
#endif
    {ORT_OPT_HEAVY_PRIO, &Options::heavy_prio, 0, 65535, "ORT_OPT_HEAVY_PRIO: 0 (off) .. 65535 steps"},
    {ORT_OPT_COST_ORDER, &Options::cost_order, 0, 1, "ORT_OPT_COST_ORDER: 0 or 1"},
    {ORT_OPT_SORT_BOUND, &Options::sort_bound, 0, INT_MAX, "ORT_OPT_SORT_BOUND must be >= 0"},  // no upper bound
    {ORT_OPT_REFILL, &Options::refill, 1, 64, "refill must be 1..64"},
};

}  // namespace

extern "C" {

int ort_create(int device, ort_ctx** out) {
    if (!out) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_create: null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceCount");
    if (device < 0 || device >= n) {
        std::string have;
        [[clang::noinline]] have = std::to_string(n);  // (called, not inlined: the library keeps exporting its copy)
        return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_create: device " + std::to_string(device) + " not present (" + have +
                                                      " visible)");
    }
    ort_ctx* c = new (std::nothrow) ort_ctx();
    if (!c) return fail(nullptr, ORT_ERR_OUT_OF_MEMORY, "ort_create: out of host memory");
    c->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = c->frame_ev.create()) != hipSuccess) {
        const int rc = hip_fail(nullptr, e, "ort_create");
        delete c;
        return rc;
    }
    for (int i = 0; i < TimingRing::kRing; ++i) {
        if ((e = c->ring.create(i, 0)) != hipSuccess) {
            const int rc = hip_fail(nullptr, e, "ort_create: events");
            ort_destroy(c);
            return rc;
        }
    }
    Pipeline& pl = c->pipe;
    if ((e = hipHostMalloc((void**)&pl.alive_host, sizeof(int) * Pipeline::kHints * Pipeline::kHintBanks,
                           hipHostMallocDefault)) != hipSuccess) {
        pl.alive_host = nullptr;
        const int rc = hip_fail(nullptr, e, "ort_create: pinned hint buffer");
        ort_destroy(c);
        return rc;
    }
    for (int i = 0; i < Pipeline::kHints * Pipeline::kHintBanks; ++i) pl.alive_host[i] = -1;
    for (int i = 0; i < Pipeline::kHintBanks; ++i)
        if ((e = hipEventCreateWithFlags(&pl.hint_ev[i], hipEventDisableTiming)) != hipSuccess) {
            const int rc = hip_fail(nullptr, e, "ort_create: hint events");
            ort_destroy(c);
            return rc;
        }
    // (the second stream itself is created with the first split frame: a stream takes one of the
    // process's few hardware queues, and contexts that never split -- group ranks sharing a
    // device -- should not crowd the others' queues)
    if ((e = hipEventCreateWithFlags(&c->split.ev_scan, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->split.ev_split, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->split.ev_pre, hipEventDisableTiming)) != hipSuccess) {
        const int rc = hip_fail(nullptr, e, "ort_create: second stream");
        ort_destroy(c);
        return rc;
    }
    *out = c;
    return ORT_OK;
}

int ort_destroy(ort_ctx* ctx) {
    if (!ctx) return ORT_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (ort_accum* a : ctx->accums) free_accum(a);
    ctx->accums.clear();
    for (ort_history* h : ctx->histories) free_history(h);
    ctx->histories.clear();
    free_scene(ctx);
    const auto drop = [](DevBuf& b) { free_buf(b); };
    each_buffer(ctx->pipe, drop);
    each_buffer(ctx->cost, drop);
    each_buffer(ctx->split, drop);
    each_buffer(ctx->pp, drop);
    each_buffer(ctx->spec, drop);
    free_state(ctx->query);
    free_state(ctx->denoise);
    ctx->frame_ev.destroy();
    ctx->ring.destroy();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->pipe.alive_host) (void)hipHostFree(ctx->pipe.alive_host);
    for (hipEvent_t ev : ctx->pipe.hint_ev)
        if (ev) (void)hipEventDestroy(ev);
    SplitWalks& sw = ctx->split;
    if (sw.aux_stream) {
        (void)hipStreamSynchronize(sw.aux_stream);
        (void)hipStreamDestroy(sw.aux_stream);
    }
    if (sw.ev_scan) (void)hipEventDestroy(sw.ev_scan);
    if (sw.ev_split) (void)hipEventDestroy(sw.ev_split);
    if (sw.ev_pre) (void)hipEventDestroy(sw.ev_pre);
    delete ctx;
    return ORT_OK;
}

const char* ort_last_error(const ort_ctx* ctx) { return ctx ? ctx->err.c_str() : ort::thread_error(); }

int ort_set_option(ort_ctx* ctx, int option, int value) {
    if (!ctx) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_set_option: null ctx");
    if (option == ORT_OPT_PERSISTENT) {
        if (value == 1)  // removed in round 4 (DESIGN.md 4)
            return fail(ctx, ORT_ERR_UNSUPPORTED, "ORT_OPT_PERSISTENT 1 (every trace persistent) was removed (C5 -19 %)");
        if (value != 0 && value != 2) return fail(ctx, ORT_ERR_INVALID_ARG, "persistent must be 0 or 2");
        ctx->opt.persistent = value;
        return ORT_OK;
    }
    if (option == ORT_OPT_EXACT_TRAVERSAL) {
        ctx->opt.exact_only = value ? 1 : 0;
        return ORT_OK;
    }
    for (const OptionRow& r : kOptions)
        if (r.id == option) {
            if (value < r.lo || value > r.hi) return fail(ctx, ORT_ERR_INVALID_ARG, r.bad);
            ctx->opt.*r.field = value;
            return ORT_OK;
        }
#if !ORT_ANALYSIS
    if (option == ORT_OPT_DEBUG_FLAGS)
        return fail(ctx, ORT_ERR_UNSUPPORTED, "ORT_OPT_DEBUG_FLAGS: analysis library only (libort_analysis.so)");
#endif
    if (ORT_OPT_IS_RETIRED(option))  // removed options (DESIGN.md 4)
        return fail(ctx, ORT_ERR_UNSUPPORTED, "option " + std::to_string(option) + " is retired (" +
                                                  (option == 5 ? "packet walk" : option == 7 ? "wave queue"
                                                                                             : "longest-first workgroups") +
                                                  ": measured slower, DESIGN.md 4)");
    return fail(ctx, ORT_ERR_INVALID_ARG, "unknown option");
}

int ort_get_stream(const ort_ctx* ctx, void** stream) {
    if (!ctx || !stream) return fail(nullptr, ORT_ERR_INVALID_ARG, "ort_get_stream: null argument");
    *stream = (void*)ctx->stream;
    return ORT_OK;
}

}  // extern "C"
