// ort_kernel.hip -- gfx950 primary/secondary-ray kernel and the device half of the C ABI.
//
// Replaces the reference's GL dispatch: setupBuffers' SSBO uploads
// (src/raytracer.cpp:74-152) become ort_upload_*; the per-frame uniform update +
// glDrawArrays (src/raytracer.cpp:491-499) becomes ort_render, which runs the fragment
// shader (glsl:636-664) as a wavefront pipeline, per sample and bounce:
//   ort_trace_kernel    camera ray (bounce 0) or stored ray + octree walk -> 8-byte hit
//                       record; one path per lane, a wave = 8x8 pixels, a workgroup = 16x16.
//                       Only the sign-specialised fast walk is compiled in, so it runs at
//                       8 waves/SIMD; rays it cannot take are appended to a defer list.
//   ort_trace_persistent  bounces >= 1: the sorted alive-path list, lanes refilled from a queue.
//   ort_trace_exact     the exact walk for the (rare) deferred rays, persistent grid.
//   ort_shade_kernel    BSDF / sky, path state or (1 spp, 1 bounce) the final pixel.
//   ort_finalize_kernel average + gamma for the multi-sample / multi-bounce case.
// The walk keeps one frame per tree level in LDS (columns indexed by lane: conflict-free),
// per-level child masks in registers, and the tree's split-plane table in LDS
// (3 x (2^D+1) floats, loaded once per workgroup).
// This file holds the kernels; the host half of the translation unit is the host_*.inc files
// included after them, followed by the queries', accumulation's and denoiser's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <type_traits>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "camera.h"
#include "gpu_build.h"
#include "layout.h"
#include "path_key.h"
#include "ort_internal.h"
#include "render_core.h"

#pragma clang fp contract(off)

// ORT_ANALYSIS (Makefile `analysis`: octreeraytracer_amd/lib/libort_analysis.so) adds the
// test/analysis surface: the ort_debug_* entry points (host emulation of the kernel's per-pixel
// code for the CPU suite, walk statistics for tools/), ORT_OPT_DEBUG_FLAGS, and the per-wave
// timeline builds (ORT_TILE_CLOCK, ORT_PERSIST_CLOCK, ORT_PERSIST_STATS, ORT_PIXEL_CLOCK).  The product library
// libort.so is built without it and exports only include/ort.h.
#ifndef ORT_ANALYSIS
#define ORT_ANALYSIS 0
#endif
#if !ORT_ANALYSIS && ((defined(ORT_TILE_CLOCK) && ORT_TILE_CLOCK) || (defined(ORT_PERSIST_CLOCK) && ORT_PERSIST_CLOCK) || \
                      (defined(ORT_PERSIST_STATS) && ORT_PERSIST_STATS) || (defined(ORT_PIXEL_CLOCK) && ORT_PIXEL_CLOCK))
#error "per-wave timeline builds are analysis builds: add -DORT_ANALYSIS=1"
#endif

namespace {

constexpr int kBlock = 256;  // 4 waves, 16x16 pixels

struct TileMap {
    int x0, tw, y0, th, bh, bs;
};

struct PipeArgs {
    ort::PixelParams pp;
    ort::KScene S;
    TileMap tm;
    int tilesX, tilesY;  // the dispatch grid: tiles, or (pair) tile pairs across x tiles
    int pair;         // ORT_OPT_TILE_PAIRS: a camera-ray workgroup renders two tiles side by side (trace_pair_body)
    int swizzle;      // ORT_OPT_XCD_SWIZZLE (block_tile)
    int xrun_log2;    // swizzle 2: log2 of the tiles per XCD run (xcd_run_log2)
    int total;        // path slots = workgroups x 256 (tile-block order, some are holes)
    int sample;       // s of main()'s sample loop
    int last;         // this bounce is the last one (b == maxDepth - 1)
    int nobounce;     // maxDepth <= 0: radiance() returns (1,1,1) without tracing
    int exact_only;   // ORT_OPT_EXACT_TRAVERSAL: every compact ray takes the exact walk
    int refill;       // persistent trace: refill a wave when at least this many lanes idle
    int final_out;    // a path that ends in the last sample writes its final pixel (no finalize pass)
    const int* qlist;    // bounce >= 1: the alive path slots (compacted, increasing), or null = all
    const int* qcount;   // their number (device)
    int* qnext;          // shade kernels: append the paths that go on here (next bounce's list), or null
    int* qnext_count;
    uint32_t* qnext_keys;  // ... and their coherence keys beside them (ORT_OPT_SORT_PATHS 2), or null
    ort::MortonPlan mp;    // the keys' origin code (path_key.h)
    const uint32_t* key_spread;  // ... as table lookups (mortonSpread)
    int2* hit;        // per path: {entry (-1 miss), t bits}
    int* defer_list;
    int* sync;        // [0] deferred count, [1] work cursor of the persistent trace
    int* sync_next;   // ort_trace_exact zeroes these 16 ints: the next trace launch's sync (the other set)
    const uint16_t* scan_pcost;  // ort_trace_exact also lists the next frame's heavy rays (split frames)
    int scan_T;
    uint32_t* scan_bits;
    int* scan_list;
    int* scan_count;
    float4* po;       // o.xyz, importance
    float4* pd;       // d.xyz, alive (1/0)
    float4* pc;       // path throughput c.xyz
    float2* prng;     // randState
    float4* pcol;     // running sum of samples
    void* out;        // the output (ort_output; out_pitch, out_format, out_place below)
    unsigned long long* counters;
    uint16_t* pcost;  // ORT_OPT_COST_ORDER: per slot, the walk steps of its last camera ray, or null
    uint16_t* bcost_w;        // ORT_OPT_HEAVY_FIRST: the persistent bounce trace records each walk's steps here
    const uint16_t* bcost_r;  // ... the kernels appending the next bounce's list read that bounce's last-frame steps
    int heavy;                // ... walks of at least this many steps are heavy: they sort first
    // ... and after a camera move (no fresh steps), the class of a path from its ray alone: the
    // root box (lo xyz, hi xyz) and the exit-distance thresholds of classes 0-2 (geo_heavy)
    int geo_heavy;
    float gbox[6];
    float gthr[3];
    int prio_steps;   // ORT_OPT_HEAVY_PRIO: a camera-ray wave holding a ray whose last walk took >= this many
                      // steps runs at raised issue priority (0: off)
    // ORT_OPT_SPLIT_HEAVY (1 sample, 1 bounce): the camera rays whose walk took >= split steps in the
    // previous frame, listed by k_heavy_scan, are walked by ort_trace_split (their walk dealt over 8
    // lanes by level-split_level subtrees) on the context's second stream; the per-tile kernel
    // passes over the slots hbits marks
    const uint32_t* hbits;
    const int* hlist;
    int* hsync;       // [0] heavy rays found (the list holds the first hcap), [1] ort_trace_split's cursor
    int* hsync_next;  // the other pair: ort_trace_split zeroes it for the next frame's scan
    int hcap;
    int split_level;
    // ort_pixel_paths with an LDS-resident scene: byte offset of nk[] in the dynamic LDS (leaf
    // spheres at lds_sph_off), their sizes in 16-byte chunks
    int lds_nk_off, lds_sph_off, lds_nk_n16, lds_sph_n16;
    // ort_pixel_paths, heavy blocks first: the 8x8 blocks in kPixelClasses cost classes (last
    // frame of this shape, read: pl_r / pl_rcnt, or null = tile order) and this frame's classes
    // for the next (pl_w / pl_wcnt; pl_cost: per block {bounces, slots done}); pl_stride blocks
    // per class segment
    const int* pl_r;
    int* pl_rcnt;
    int* pl_w;
    int* pl_wcnt;
    unsigned long long* pl_cost;
    int pl_stride;
    // whole-pixel paths, samples in parallel (ORT_OPT_PIXEL_SPECULATE): a pixel's samples in
    // sp_nch chunks of sp_chunk; per chunk c and slot k (index c * total + k) the RNG state the
    // chunk ends with -- sp_prev last frame's (chunk c+1 of this frame starts from sp_prev[c]),
    // sp_cur this frame's -- and per sample s the radiance (sp_col: three planes of ns * total
    // floats, index s * total + k).  A whole-pixel launch with sp_cur records its chunks' end
    // states; one with fx_slot runs the fixup list: pixel fx_slot[i] from sample fx_s0[i] with
    // state fx_st[i] and the colour sum of its earlier samples fx_col (three planes of total
    // floats), *fx_n entries
    // (An adaptive pass, PM 5, and its pre-pass and stats kernels also borrow sp_nch, hcap and gthr[0..1]
    // from further up -- adaptive.inc says for what: a whole-pixel kernel that starts to read those must
    // look there first.)
    // An accumulation pass (ort_accum_render, PM 3: accum.inc) borrows four of these fields, indexed
    // by path slot: samples `sample` .. sp_chunk - 1 of every pixel, from the RNG state fx_st[k] and
    // the colour sum fx_col (three planes of total floats) when sample > 0, both stored back
    const float2* sp_prev;
    float2* sp_cur;
    float* sp_col;
    int sp_chunk, sp_nch;  // samples per SPEC item (a chunk of a pixel's samples), chunks per pixel
    // sp_ctl[0] the fixup list's length, [1] the pixels the last frame found moved, [2] this
    // frame's mode (1 speculate, 0 fall back: every pixel's whole chain through the fixup list)
    // -- decided on the device by ort_sample_decide, so frames queued ahead of the host follow it
    int* sp_ctl;
    int* fx_n;
    int* fx_slot;
    int* fx_s0;
    float2* fx_st;
    float* fx_col;
    // the output description (store_pixel / store_padding): the pixel of output row R, column C at
    // out + R * out_pitch + C * bytes per pixel.  (Last, so that the fields above keep their places
    // in the kernel argument segment: the tuned kernels load them in the same groups as before.)
    unsigned out_pitch;   // bytes per output row (32 bits: a row's address is one 32 x 32 -> 64 bit multiply-add)
    int out_format;       // ORT_FORMAT_*
    int out_place;        // ORT_PLACE_*
#if ORT_ANALYSIS
    ulonglong4* wclock;  // analysis builds only (ORT_PERSIST_CLOCK, ort_debug_wave_clock): per wave a timeline record
    int wclock_n;
#endif
};

__host__ __device__ inline int tile_row_to_y(const TileMap& t, int j) {
    return t.bh > 0 ? t.y0 + (j / t.bh) * t.bs + (j % t.bh) : t.y0 + j;
}

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

constexpr size_t kRankLutBytes = 8 * 256;  // ort::rank_lut_entry table

// The persistent bounce kernel at depth 9-10 (Masks96Lean): 512-thread
// workgroups over the reversed-table image (fast_rev_planes: 32.8 KB at depth 10, the rank
// LUT in its gap), 53.3 KB of LDS with 512 lanes' frames -- 3 workgroups = 6 waves/SIMD.
constexpr bool kRevBounce = ort::Masks96Lean::kRevPlanes;  // (true)
#ifndef ORT_PERSIST_DEEP_BLOCK
#define ORT_PERSIST_DEEP_BLOCK 512
#endif
constexpr int kPersistDeepBlock = ORT_PERSIST_DEEP_BLOCK;

// with_tm: the exact walk also keeps a per-level tmin column; the fast walk needs none.
// rev / nb: the image layout and workgroup size (the deep persistent kernel's: true, 512).
size_t lds_bytes(int mode, int depth, bool with_tm, bool rev = false, int nb = kBlock) {
    if (mode != 0) return 0;
    const ort::LdsLayout l = ort::lds_layout(depth, rev || ort::fast_rev_planes(depth));
    const size_t levels = (size_t)std::max(depth, 1);
    return (size_t)l.frames + (with_tm ? 2 : 1) * levels * (size_t)nb * sizeof(int);
}

// LDS image of one workgroup: split planes | rank LUT | frame columns (co[, tmin]).
struct LdsView {
    const float* planes;
    const uint8_t* lut;
    ort::LdsFrames fr;
};
template <bool WITH_LUT, int NB = kBlock>
__device__ inline LdsView lds_view(unsigned char* smem, int D, bool rev = false) {
    const ort::LdsLayout l = ort::lds_layout(D, rev || ort::fast_rev_planes(D));
    LdsView v;
    v.planes = reinterpret_cast<float*>(smem);
    v.lut = WITH_LUT ? smem + l.lut : nullptr;
    v.fr.co = reinterpret_cast<int*>(smem + l.frames);
    v.fr.tm = reinterpret_cast<float*>(smem + l.frames + (size_t)(D > 0 ? D : 1) * NB * sizeof(int));
    v.fr.stride = NB;
    v.fr.lane = threadIdx.x;
    return v;
}
// The plane tables and rank LUT are the same for every workgroup of a scene: k_lds_image
// builds them once per scene (ort_ctx::lds_img; at depth 9-10 also the reversed-table image
// ort_ctx::lds_rev) and each workgroup copies the image in 16-byte pieces -- building them
// per workgroup (an integer division per plane entry, ~80 VALU per LUT byte) cost as much
// VALU as several walk steps of every wave.
__global__ void __launch_bounds__(kBlock) k_lds_image(const float* planes, int D, bool rev, unsigned char* img) {
    const int tid = threadIdx.x;
    rev = rev || ort::fast_rev_planes(D);
    ort::fill_fast_planes(planes, reinterpret_cast<float*>(img), D, rev, tid, kBlock);  // forward, then reversed
    __syncthreads();  // the LUT may sit in a gap of the tables (lds_layout)
    uint8_t* lut = img + ort::lds_layout(D, rev).lut;
    for (int i = tid; i < (int)kRankLutBytes; i += kBlock) lut[i] = ort::rank_lut_entry((uint32_t)i >> 8, (uint32_t)i & 255u);
}
// REV: the reversed-table image of a depth 9-10 tree (S.lds_rev), for NB-thread workgroups.
template <bool WITH_LUT, int NB = kBlock, bool REV = false>
__device__ inline LdsView setup_lds(unsigned char* smem, const ort::KScene& S) {
#if defined(__HIP_DEVICE_COMPILE__)
    // The reversed plane tables rely on absolute LDS addresses aligned to their 4T-byte
    // blocks (1 KiB at depth <= 8, up to 4 KiB in the depth 9-10 reversed image); dynamic
    // LDS follows any static LDS (append_slots' counters), so check it.  The address is a
    // link-time constant: the check folds away when it holds and traps loudly when not.
    if (reinterpret_cast<uintptr_t>(smem) & (REV ? 4095u : 1023u)) __builtin_trap();
#endif
    const int n16 = REV ? S.lds_rev_n16 : (WITH_LUT ? S.lds_img_n16 : S.lds_img_p16);
    const uint4* src = REV ? S.lds_rev : S.lds_img;
    uint4* dst = reinterpret_cast<uint4*>(smem);
    for (int i = threadIdx.x; i < n16; i += NB) dst[i] = src[i];
    __syncthreads();
    return lds_view<WITH_LUT, NB>(smem, S.depth, REV);
}

// Tile (bx, by) of 16x16 pixels rendered by workgroup blk.  The dispatcher deals workgroup b
// to XCD b % 8, each XCD with its own L2.  ORT_OPT_XCD_SWIZZLE picks the order:
//   0  raster: XCD x renders every 8th tile of a tile row -- neighbouring tiles, whose rays
//      walk the same octree nodes, are spread over all 8 L2s;
//   2  (default above kRasterAutoPixels) within every 8*run consecutive workgroups the `run` that land on one XCD
//      get `run` consecutive raster tiles (run = xcd_run_log2: 16 tiles, a 256x16-pixel run,
//      at 3840 px): c3 +2% (8-tile runs) and another +1.7% (16), c5 +2% in interleaved A/B
//      (tools/ab_stream.py);
//   1  within every 512 the 64 of one XCD get an 8x8-tile super-tile (128x128 pixels): more
//      compact but slower at c3 (-1.5% vs raster) -- the run order keeps consecutive
//      workgroups of one XCD on neighbouring tiles while they are resident together.
// Each is a bijection on any tile grid (a last partial group keeps raster order; super-tiles at
// the frame's right/bottom edge are narrower), so the pixels are the same whichever order runs.
// Swizzle 2's run length: the largest power of two <= tilesX / 15 (1..64), i.e. each XCD's
// run covers about a fifteenth of a tile row.  Measured (interleaved A/B): 8-tile runs are
// best at 1920 px (120 tiles per row; 16 is 1.9 % slower), 16-tile runs at 3840 px (+1.2 %
// over 8).
inline int xcd_run_log2(int tilesX) {
    int lr = 0;
    while (lr < 6 && (2 << lr) * 15 <= tilesX) ++lr;
    return lr;
}
__host__ __device__ inline void block_tile_grid(const PipeArgs& A, int blk, int& bx, int& by) {
    if (!A.swizzle) {
        bx = blk % A.tilesX;
        by = blk / A.tilesX;
        return;
    }
    int l = blk;
    if (A.swizzle == 2) {  // raster order in chunks of 8 tiles per XCD
        const int lr = A.xrun_log2, run = 1 << lr, group = 8 << lr;
        if ((blk | (group - 1)) < A.tilesX * A.tilesY)
            l = (blk & ~(group - 1)) | ((blk & 7) << lr) | ((blk >> 3) & (run - 1));
        bx = l % A.tilesX;
        by = l / A.tilesX;
        return;
    }
    if ((blk | 511) < A.tilesX * A.tilesY) l = (blk & ~511) | ((blk & 7) << 6) | ((blk >> 3) & 63);
    // logical order: super-rows of 8 tile rows; in one, super-tiles of 8 tile columns left to
    // right; in one, tiles in raster order
    const int srow = l / (A.tilesX * 8);
    const int rem = l - srow * A.tilesX * 8;
    const int rows = A.tilesY - srow * 8 < 8 ? A.tilesY - srow * 8 : 8;
    const int sc = rem / (8 * rows);
    const int r2 = rem - sc * 8 * rows;
    const int cols = A.tilesX - sc * 8 < 8 ? A.tilesX - sc * 8 : 8;
    bx = sc * 8 + r2 % cols;
    by = srow * 8 + r2 / cols;
}
// Tile pairs (ORT_OPT_TILE_PAIRS): slot blocks 2b and 2b+1 are the two tiles of pair b, which the
// swizzle places on the pair grid (x-adjacent tiles; a last odd column's second tile is a hole).
__host__ __device__ inline void block_tile(const PipeArgs& A, int blk, int& bx, int& by) {
    if (!A.pair) {
        block_tile_grid(A, blk, bx, by);
        return;
    }
    block_tile_grid(A, blk >> 1, bx, by);
    bx = 2 * bx + (blk & 1);
}

// Path slot k (tile-block order: 256 slots = one 16x16 tile, 64 = one 8x8 wave block)
// -> tile column/row.  Returns false for slots outside the tile.  UNI: every lane of the wave
// holds a slot of the same 256-slot block (the per-tile kernels), so the tile lookup -- two
// integer divisions by the tile-grid width -- runs once per wave on the scalar unit.  UNI 2:
// every lane holds a slot of the same tile PAIR (tile pairs, cost_order_pair), so the pair's
// place is looked up once per wave and each lane picks its tile of the two.
template <int UNI = 0>
__host__ __device__ inline bool slot_coords(const PipeArgs& A, int k, int& col, int& row) {
    const int tid = k & 255, wave = tid >> 6, lane = tid & 63;
    int bx, by;
#if defined(__HIP_DEVICE_COMPILE__)
    if (UNI == 2) {
        block_tile_grid(A, __builtin_amdgcn_readfirstlane(k >> 9), bx, by);
        bx = 2 * bx + ((k >> 8) & 1);
    } else {
        block_tile(A, UNI ? __builtin_amdgcn_readfirstlane(k >> 8) : k >> 8, bx, by);
    }
#else
    block_tile(A, k >> 8, bx, by);
#endif
    col = bx * 16 + (wave & 1) * 8 + (lane & 7);  // an 8x8 block per wave (16x4 and 4x16: no faster, §8)
    row = by * 16 + (wave >> 1) * 8 + (lane >> 3);
    return col < A.tm.tw && row < A.tm.th;
}

template <bool COUNT>
__device__ inline void flush_counts(const ort::Counters& c, unsigned long long* dst) {
    if (COUNT)
        for (int k = 0; k < 6; ++k)
            if (c.v[k]) atomicAdd(dst + k, c.v[k]);
}

__device__ inline ort::Ray load_ray(const PipeArgs& A, int k, bool& alive) {
    const float4 o = A.po[k], d = A.pd[k];
    ort::Ray r;
    r.o = ort::mk(o.x, o.y, o.z);
    r.d = ort::mk(d.x, d.y, d.z);
    alive = d.w != 0.0f;
    return r;
}

// Persistent trace over the compact layout: every lane keeps one ray's FastState; the
// wave owns a chunk of kChunk consecutive path slots (one atomic on the global cursor per
// chunk, MI355X_MICROARCH.md 'dequeue') and hands the next slots of its chunk to lanes
// that finished, so the wave stays full until the queue drains.  Rays the fast walk
// cannot take are appended to the defer list for ort_trace_exact.
// Waves per SIMD (minimum, amdgpu_waves_per_eu): the per-lane trace kernels run at 8 (59-64
// VGPRs, spill-free; tools/kernel_resources.py).  The persistent bounce kernel is asked for 6:
// its depth 9-10 walk over the reversed plane tables fits 79 VGPRs there without spills (the
// forward-table walk needed 87 unconstrained and spilled 5 at 6 waves), and its LDS (53.3 KB
// per 512-thread workgroup at depth 10) caps it at 6 anyway; the depth <= 8 instance 78.
#ifndef ORT_PERSISTENT_WAVES
#define ORT_PERSISTENT_WAVES 6
#endif
#ifndef ORT_TRACE_WAVES
#define ORT_TRACE_WAVES 8
#endif
// Deep (depth > 8) per-lane kernel: its LDS image (24.6 KB per 256-thread workgroup at depth 10)
// caps a CU at 6 workgroups = 6 waves/SIMD, so it may use the registers of 6 waves: 60-64
// VGPRs without spills.  (512-thread workgroups, whose LDS would allow 8 waves/SIMD at these
// 64 VGPRs, measured no faster: C5 -0.1 % at 6, -0.4 % at 8 in A/B.)
#ifndef ORT_TRACE_WAVES_DEEP
#define ORT_TRACE_WAVES_DEEP 6
#endif
// Items a wave takes from the global cursor at a time.  The resident waves then work on a
// window of about (waves x kChunk) consecutive list items -- neighbouring paths, overlapping
// node sets, one L2 working set: C5 frame 58.2 (256) -> 56.7 (128) -> 55.8 ms (64; 32: 56.0)
// in A/B.  (One queue per XCD over 8 contiguous list ranges measured no better: -0.4 %.)
#ifndef ORT_PERSIST_CLOCK
#define ORT_PERSIST_CLOCK 0
#endif
// Analysis builds only (-DORT_PERSIST_STATS=1, tools/persist_stats.py): per wave of the persistent
// kernel, how its loop iterations went -- refills, steps, and how many lanes stepped an internal
// node or a leaf (the two blocks of a step run one after the other, each with its own lanes).
#ifndef ORT_PERSIST_STATS
#define ORT_PERSIST_STATS 0
#endif
// Leaf hold in the depth 9-10 bounce walk: a lane whose next node is a leaf waits until this many
// lanes of its wave are at leaves (or none is at an internal node), so the leaf block -- run in 92 %
// of the steps for 6.5 lanes on average (tools/persist_stats.py) -- runs less often for more lanes.
// C5 +2.4 / +2.7 / +2.3 / -2.4 % at 8 / 12 / 16 / 24 (tools/ab_stream.py); the depth <= 8 bounce
// walk loses (C3 at 4 bounces: -1.7 % at 8), so it is off there.
#ifndef ORT_LEAF_HOLD
#define ORT_LEAF_HOLD 12
#endif
// ... and only while at least this many lanes are at internal nodes: in a launch's drain (few lanes
// left) a held leaf lane would wait for a lone internal walk -- C5 1/8 band at one frame in
// flight 7.2 -> 8.2 ms with 1 (full frame: 16 and 1 alike)
#ifndef ORT_LEAF_HOLD_MIN_INTERNAL
#define ORT_LEAF_HOLD_MIN_INTERNAL 16
#endif
#ifndef ORT_CHUNK
#define ORT_CHUNK 64
#endif
constexpr int kChunk = ORT_CHUNK;
// Lists of at least ORT_CHUNK_ADAPT items per resident wave take chunks of 2 x kChunk: C5
// +0.7 % (bounces 1-2 of the full frame), band tiles unchanged (tools/ab_stream.py); fixed
// 128-item chunks lost 20 % on a 1/8 band (too few chunks per wave to balance).  0: kChunk.
#ifndef ORT_CHUNK_ADAPT
#define ORT_CHUNK_ADAPT 1024
#endif

// DEEP: trees deeper than 8 levels (96-bit masks, lean state); depth <= 8 takes the
// primary-ray walk's 64-bit masks and reversed plane tables (71 VGPRs, 7 waves/SIMD).
template <bool COUNT, bool DEEP>
__global__ void __launch_bounds__(DEEP ? kPersistDeepBlock : kBlock) __attribute__((amdgpu_waves_per_eu(ORT_PERSISTENT_WAVES)))
ort_trace_persistent(PipeArgs A) {
    // plane tables at 4T-byte-aligned absolute LDS addresses (fast_rev_planes; no static LDS here)
    extern __shared__ __attribute__((aligned(4096))) unsigned char smem[];
    constexpr bool REV = DEEP && kRevBounce;
    LdsView L = setup_lds<true, DEEP ? kPersistDeepBlock : kBlock, REV>(smem, A.S);
    const uint8_t* lut = L.lut;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    ort::Counters cnt;
    for (int q = 0; q < 6; ++q) cnt.v[q] = 0;
    // depth <= 8 without the inline leaf children: on incoherent bounce rays they cost 9 %
    // (C3 scene, 8 bounces); the plain 64-bit walk is 5 % faster than the 96-bit one there
    using Masks = typename std::conditional<DEEP, ort::Masks96Lean, ort::Masks64Plain>::type;
    ort::FastStateT<Masks> st;
    int k = -1;
    int nst = 0;             // steps of the lane's walk (ORT_OPT_HEAVY_FIRST's record)
    int next = 0, end = 0;   // wave-uniform: remaining work items [next, end) of the wave's chunk
    bool drained = false;    // wave-uniform: the global cursor passed the item count
    // items: the compacted (sorted) alive-path list of a bounce >= 1, or every slot
    const int total = A.qlist ? *A.qcount : A.total;
#if ORT_CHUNK_ADAPT
    // long lists (>= ORT_CHUNK_ADAPT items per resident wave): twice the chunk
    const int chunk = total >= (int)(gridDim.x * (blockDim.x >> 6)) * ORT_CHUNK_ADAPT ? 2 * kChunk : kChunk;
#else
    constexpr int chunk = kChunk;
#endif
#if ORT_PERSIST_CLOCK  // analysis builds only (tools/build_variant.sh): per-wave timeline
    const unsigned long long clk0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long clk_drain = 0;
    int n_items = 0;
#endif
#if ORT_PERSIST_STATS
    unsigned long long ps[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // iterations, refills, steps, internal lanes,
                                                            // leaf lanes, steps with internal / leaf / both
#endif
    for (;;) {
        const unsigned long long idle = __ballot(k < 0);
        const int n_idle = __popcll(idle);
        if (n_idle == 64 && drained) break;
#if ORT_PERSIST_STATS
        ps[0] += 1;
#endif
        if (!drained && n_idle >= A.refill) {
#if ORT_PERSIST_STATS
            ps[1] += 1;
#endif
            if (next == end) {
                int base = 0;
                if (lane == 0) base = atomicAdd(A.sync + 1, chunk);
                base = __shfl(base, 0);
                if (base >= total) {
                    drained = true;
#if ORT_PERSIST_CLOCK
                    clk_drain = __builtin_amdgcn_s_memrealtime();
#endif
                    continue;
                }
#if ORT_PERSIST_CLOCK
                n_items += min(base + chunk, total) - base;
#endif
                next = base;
                end = min(base + chunk, total);
            }
            const int take = min(n_idle, end - next);
            if (k < 0) {
                const int rank = __popcll(idle & below);
                if (rank < take) {
                    const int cand = A.qlist ? A.qlist[next + rank] : next + rank;
                    bool alive;
                    const ort::Ray ray = load_ray(A, cand, alive);
                    if (alive) {
                        ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
                        if (A.exact_only || !ort::fast_prepare(A.S, ray, inv)) {
                            A.defer_list[atomicAdd(A.sync, 1)] = cand;
                        } else {
                            if (COUNT) cnt.v[5] += 1;
                            nst = 0;
                            if (ort::fast_begin(A.S, L.planes, lut, ray, inv, 0.001f, ORT_MAXFLOAT, st)) k = cand;
                            else A.hit[cand] = make_int2(-1, 0);
                        }
                    }
                }
            }
            next += take;
            continue;
        }
#if ORT_PERSIST_STATS
        {
            const bool in = k >= 0 && (st.rec.y & ORT_INTERNAL_FLAG);
            const bool lf = k >= 0 && !(st.rec.y & ORT_INTERNAL_FLAG);
            const int ni = __popcll(__ballot(in)), nl = __popcll(__ballot(lf));
            ps[2] += 1;
            ps[3] += ni;
            ps[4] += nl;
            ps[5] += ni > 0;
            ps[6] += nl > 0;
            ps[7] += (ni > 0 && nl > 0);
        }
#endif
#if ORT_LEAF_HOLD
        // leaf hold (DEEP): each lane's own walk is unchanged, only when it steps (same pixels)
        bool hold = false;
        if (DEEP) {
            const bool at_leaf = k >= 0 && !(st.rec.y & ORT_INTERNAL_FLAG);
            const unsigned long long lm = __ballot(at_leaf), im = __ballot(k >= 0 && !at_leaf);
            hold = at_leaf && __popcll(im) >= ORT_LEAF_HOLD_MIN_INTERNAL && __popcll(lm) < ORT_LEAF_HOLD;
        }
        if (k >= 0 && !hold) {
#else
        if (k >= 0) {
#endif
            ++nst;
            if (ort::fast_step<COUNT>(A.S, lut, st, L.fr, cnt)) {
                A.hit[k] = make_int2(st.hitEntry, __float_as_int(st.closest));
                if (!COUNT && A.bcost_w) A.bcost_w[k] = (uint16_t)min(nst, 65535);
                k = -1;
            }
        }
    }
#if ORT_PERSIST_CLOCK
    const int gw = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (A.wclock && lane == 0 && gw < A.wclock_n) {
        const unsigned xcc = __builtin_amdgcn_s_getreg((15 << 11) | 20);  // XCC_ID
        A.wclock[gw] = make_ulonglong4(clk0, clk_drain, __builtin_amdgcn_s_memrealtime(),
                                       (unsigned long long)(xcc & 15u) | ((unsigned long long)n_items << 8));
    }
#endif
#if ORT_PERSIST_STATS
    {
        const int gw = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
        if (A.wclock && lane == 0 && 2 * gw + 1 < A.wclock_n) {
            A.wclock[2 * gw] = make_ulonglong4(ps[0], ps[1], ps[2], ps[3]);
            A.wclock[2 * gw + 1] = make_ulonglong4(ps[4], ps[5], ps[6], ps[7]);
        }
    }
#endif
    flush_counts<COUNT>(cnt, A.counters);
}

// Bounce >= 1 with a compacted list: thread index -> alive path slot (false past the list).
__device__ inline bool list_slot(const PipeArgs& A, int& k) {
    if (!A.qlist) return true;
    if (k >= *A.qcount) return false;
    k = A.qlist[k];
    return true;
}

// Path-slot ray for the trace kernels: bounce 0 generates the sample's camera ray here
// (main() up to radiance()'s first line; the shade kernel regenerates it identically),
// later bounces read the ray the previous shade kernel stored.
template <bool PRIMARY, int UNI = 0>
__device__ inline ort::Ray slot_ray(const PipeArgs& A, int k, bool& alive, ort_rng* st_out = nullptr) {
    if constexpr (PRIMARY) {
        int col, row;
        alive = slot_coords<UNI>(A, k, col, row);
        const int y = alive ? tile_row_to_y(A.tm, row) : 0;
        alive = alive && y < A.pp.H;
        ort::Ray ray;
        ray.o = ort::mk(0.0f, 0.0f, 0.0f);
        ray.d = ray.o;
        if (!alive) return ray;
        ort_rng st;
        if (A.sample == 0) {
            ort::pixel_rng_init(A.pp, A.tm.x0 + col, y, st);
        } else {
            const float2 v = A.prng[k];
            st.x = v.x;
            st.y = v.y;
        }
        const ort::Ray r = ort::primary_ray(A.pp, A.tm.x0 + col, y, A.sample, st);
        if (st_out) *st_out = st;
        return r;
    } else {
        return load_ray(A, k, alive);
    }
}

// Every pixel leaves the kernels through store_pixel / store_padding.  The format and the
// placement are wave-uniform kernel arguments: scalar branches.
// out_coords: the output row and column of tile row `row`, tile column `col` -- themselves under
// tile placement, the pixel's (y, x) under frame placement (y < 0 where the site does not hold the
// pixel row: derived).  PLAIN: compiled for ort_render's own output (RGB32F, tile placement, tight
// rows) alone -- ort_shade_kernel's bounce-0 instance, whose scalar registers the output
// description would overflow (8 -> 7 waves per SIMD).
template <bool PLAIN = false>
__device__ __forceinline__ void out_coords(const PipeArgs& A, int row, int col, int y, int& orow, int& ocol) {
    orow = row;
    ocol = col;
    if (!PLAIN && A.out_place == ORT_PLACE_FRAME) {  // the pixel (x, y) at row y, column x of a whole frame
        orow = y < 0 ? tile_row_to_y(A.tm, row) : y;
        ocol = A.tm.x0 + col;
    }
}
// The finished pixel v at output row orow, column ocol (out_coords).
template <bool PLAIN = false>
__device__ __forceinline__ void store_at(const PipeArgs& A, int orow, int ocol, ort::V3 v) {
    if (PLAIN) {
        float* o = (float*)A.out + 3 * ((size_t)orow * A.tm.tw + ocol);
        o[0] = v.x;
        o[1] = v.y;
        o[2] = v.z;
        return;
    }
    char* o8 = (char*)A.out + (size_t)(unsigned)orow * A.out_pitch;
    if (A.out_format == ORT_FORMAT_RGBA8) {
        *(uint32_t*)(o8 + 4u * (unsigned)ocol) = ort::pack_rgba8(v);
    } else {
        float* o = (float*)(o8 + 12u * (unsigned)ocol);
        // plain stores (one global_store_dwordx3): non-temporal ones ran no faster and, their
        // partial 64-byte lines written out unmerged, moved 1.38x the frame's bytes (PMC WRITE_SIZE)
        o[0] = v.x;
        o[1] = v.y;
        o[2] = v.z;
    }
}
// store_pixel: the finished pixel v of tile row `row`, tile column `col` (a pixel of the frame:
// its row y < H at every site; y < 0 where the site does not hold it).
__device__ __forceinline__ void store_pixel(const PipeArgs& A, int row, int col, int y, ort::V3 v) {
    int orow, ocol;
    out_coords(A, row, col, y, orow, ocol);
    if (A.out_place == ORT_PLACE_FRAME && orow >= A.pp.H) return;  // (the frame's bound, kept here too)
    store_at(A, orow, ocol, v);
}
// The kernel's arguments read again from the kernel argument segment through a laundered pointer
// (as trace_slot does for its shading): for a store at the end of a long loop, so that the output
// description is not held in scalar registers across it.  Kernels whose first argument is PipeArgs.
__device__ __forceinline__ PipeArgs reread_args(const PipeArgs& A) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const PipeArgs KernArgs;
    KernArgs* kp = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return *kp;
#else
    return A;
#endif
}

// A tile row past the frame (band padding, y >= H): zeros under tile placement (an RGBA8 pixel's
// four bytes, alpha included: the row stays recognisable); under frame placement it lies outside
// the frame and nothing is written.
__device__ __forceinline__ void store_padding(const PipeArgs& A, int row, int col) {
    if (A.out_place == ORT_PLACE_FRAME) return;
    if (A.out_format == ORT_FORMAT_RGBA8) {
        *(uint32_t*)((char*)A.out + ((size_t)(unsigned)row * A.out_pitch + 4u * (unsigned)col)) = 0u;
    } else {
        float* o = (float*)((char*)A.out + ((size_t)(unsigned)row * A.out_pitch + 12u * (unsigned)col));
        o[0] = 0.0f;
        o[1] = 0.0f;
        o[2] = 0.0f;
    }
}

// 1 sample, 1 bounce (the primary-ray benchmark mode): the trace kernels shade their own
// rays -- exactly ort_shade_kernel<0, true, true> -- instead of writing hit records for it.
template <int UNI = 0>
__device__ inline void shade_direct(const PipeArgs& A, int k, ort::Ray ray, ort_rng st, bool hit, int entry, float t) {
    int col, row;
    (void)slot_coords<UNI>(A, k, col, row);
    ort::V3 c = ort::mk(1.0f, 1.0f, 1.0f);
    float importance = 1.0f;
    ort::HitRec rec;
    if (hit) rec = ort::hit_record<0>(A.S, ray, t, entry);
    (void)ort::shade_bounce<true>(hit, rec, ray, c, importance, st);  // 1 sample, 1 bounce: final
    const ort::V3 v = ort::finish_pixel(ort::add(ort::mk(0.0f, 0.0f, 0.0f), c), 1);
    store_pixel(A, row, col, -1, v);
}
// Tile rows past the frame (band padding) are written as zeros, as the shade kernel does.
template <int UNI = 1>
__device__ inline void shade_direct_padding(const PipeArgs& A, int k) {
    int col, row;
    if (!slot_coords<UNI>(A, k, col, row) || tile_row_to_y(A.tm, row) < A.pp.H) return;
    store_padding(A, row, col);
}

// The shading proper of path slot k, given its ray and RNG state and the walk's result
// (entry < 0: no hit); shared by ort_shade_kernel and the trace kernels that shade bounce 0
// themselves.  Returns true when the path goes on to the next bounce.
template <int MODE, bool FIRST, bool DIRECT, bool PLAIN = false>
__device__ __forceinline__ bool shade_state(const PipeArgs& A, int k, int orow, int ocol, ort::Ray ray, ort_rng st,
                                            int entry, float t) {
    ort::V3 c = ort::mk(1.0f, 1.0f, 1.0f);
    float importance = 1.0f;
    if (!FIRST) {
        const float4 cc = A.pc[k];
        c = ort::mk(cc.x, cc.y, cc.z);
        importance = A.po[k].w;
    }
    bool done = true;
    if (!A.nobounce) {
        ort::HitRec rec;
        if (entry >= 0) rec = ort::hit_record<MODE>(A.S, ray, t, entry);
        if (A.last && A.sample == A.pp.ns - 1)  // nothing reads the ray or RNG state after this bounce
            done = ort::shade_bounce<true>(entry >= 0, rec, ray, c, importance, st);
        else
            done = ort::shade_bounce(entry >= 0, rec, ray, c, importance, st);
        if (!done && (A.last || importance < 0.01f)) done = true;  // loop bound / glsl:605
    }
    if constexpr (DIRECT) {
        const ort::V3 v = ort::finish_pixel(ort::add(ort::mk(0.0f, 0.0f, 0.0f), c), 1);
        store_at(A, orow, ocol, v);
    } else {
        // the last sample of a final_out frame: a path that ends here writes its pixel and
        // nothing else -- the later kernels walk the lists of alive paths only, and no sample
        // follows to read its RNG state
        const bool fin = A.final_out && A.sample == A.pp.ns - 1;
        if (done) {
            ort::V3 acc = ort::mk(0.0f, 0.0f, 0.0f);
            if (A.sample > 0) {
                const float4 a = A.pcol[k];
                acc = ort::mk(a.x, a.y, a.z);
            }
            acc = ort::add(acc, c);
            if (fin) {  // ort_finalize_kernel's work for this pixel
                const ort::V3 v = ort::finish_pixel(acc, A.pp.ns);
                store_at<PLAIN>(A, orow, ocol, v);
            } else {
                A.pcol[k] = make_float4(acc.x, acc.y, acc.z, 0.0f);
                A.pd[k] = make_float4(ray.d.x, ray.d.y, ray.d.z, 0.0f);
            }
        } else {
            A.po[k] = make_float4(ray.o.x, ray.o.y, ray.o.z, importance);
            A.pd[k] = make_float4(ray.d.x, ray.d.y, ray.d.z, 1.0f);
            A.pc[k] = make_float4(c.x, c.y, c.z, 0.0f);
        }
        if (!(done && fin)) A.prng[k] = make_float2(st.x, st.y);
    }
    return !DIRECT && !done;
}

// Appends slot k (where go) to list / count: one atomic per workgroup, the workgroup's slots
// kept in increasing order.  Every thread of the workgroup must call it.
__device__ inline void append_slots(bool go, int k, uint32_t key, int* list, uint32_t* keys, int* count) {
    __shared__ int wcnt[kBlock / 64];
    __shared__ int wbase;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(go);
    if (lane == 0) wcnt[w] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < kBlock / 64; ++i) t += wcnt[i];
        wbase = t ? atomicAdd(count, t) : 0;
    }
    __syncthreads();
    int off = wbase;
    for (int i = 0; i < w; ++i) off += wcnt[i];
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    if (go) {
        const int pos = off + __popcll(m & below);
        list[pos] = k;
        if (keys) keys[pos] = key;
    }
}

// Heavy first (ORT_OPT_HEAVY_FIRST): the key of a path appended to the next bounce's list gets
// a 2-bit cost class above its coherence bits, from the steps c that bounce's walk took in
// the previous frame of the same shape: 0 for c >= 4T, 1 for >= 2T, 2 for >= T, 3 below (T =
// A.heavy) -- the list sort then puts the longest walks first, each class in coherence order,
// and the persistent trace starts them early instead of in its drain tail.
#ifndef ORT_HEAVY_LEVELS
#define ORT_HEAVY_LEVELS 3  // classes above the lightest (1: one threshold)
#endif
#ifndef ORT_HEAVY_RATIO_LOG2
#define ORT_HEAVY_RATIO_LOG2 1  // class thresholds T, 2T, 4T
#endif
static_assert(ORT_HEAVY_LEVELS >= 1 && ORT_HEAVY_LEVELS <= 7, "ORT_HEAVY_LEVELS: 1..7 classes above the lightest");
constexpr int kHeavyKeyBits = ORT_HEAVY_LEVELS > 3 ? 3 : (ORT_HEAVY_LEVELS > 1 ? 2 : 1);
// the class sits above the path key's bits in a 32-bit radix key (sortListBounded's end bit)
static_assert(ort::kPathKeyBits + kHeavyKeyBits <= 32, "heavy-first class bits + path key bits exceed 32");
// Heavy first after a camera move: the class from the new ray alone -- bounce walks of rays that
// leave the root box soon run longest (the C5 slab, bounce 1: exit within 1.2x the box's
// smallest extent, half of the rays, 29 % of them >= 256 steps; beyond 6.8x, 0.5 %;
// tools/bounce_texit.py).  Classes 0-2 by the thresholds gthr, 3 beyond (as light_bit's).
__device__ __forceinline__ uint32_t geo_class_bits(const float* gb, const float* th, float4 o, float4 d) {
    float tx = 3.0e38f;
    const float oa[3] = {o.x, o.y, o.z}, da[3] = {d.x, d.y, d.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float inv = 1.0f / da[a];  // (+-inf for a zero component: that axis never bounds)
        const float t = fmaxf((gb[a] - oa[a]) * inv, (gb[3 + a] - oa[a]) * inv);
        tx = fminf(tx, t);
    }
    const uint32_t cls = tx <= th[0] ? 0u : (tx <= th[1] ? 1u : (tx <= th[2] ? 2u : 3u));
    return min(cls, (uint32_t)ORT_HEAVY_LEVELS) << ort::kPathKeyBits;
}
__device__ __forceinline__ uint32_t light_bit(const uint16_t* bcost_r, int heavy, int k) {
    if (!bcost_r) return 0u;
    const int c = bcost_r[k];
    uint32_t cls = ORT_HEAVY_LEVELS;
    for (int l = 0; l < ORT_HEAVY_LEVELS; ++l) cls -= c >= (heavy << (ORT_HEAVY_RATIO_LOG2 * l)) ? 1u : 0u;
    return cls << ort::kPathKeyBits;
}
// The sort key of path k (its state just stored) with its heavy-first class.
__device__ __forceinline__ uint32_t path_key_class(const PipeArgs& A, int k) {
    const float4 o = A.po[k], d = A.pd[k];
    return ort::path_key(o, d, A.mp, A.key_spread) |
           (A.geo_heavy ? geo_class_bits(A.gbox, A.gthr, o, d) : light_bit(A.bcost_r, A.heavy, k));
}

// One ray per lane over the compact layout (default): the tile-block order of the path
// slots keeps each wave on an 8x8 pixel block, whose rays walk nearly the same nodes.
// DEEP: trees deeper than 8 levels need the 96-bit level masks (ort_trace_compact_deep).
// One path slot k of the compact-layout trace (the per-lane walk); counts accumulate in cnt.
// FUSE: 0 the walk's hit record is stored (shaded by ort_shade_kernel); 1 (1 sample, 1 bounce)
// the kernel shades its ray into the final pixel; 2 (bounce 0 of a multi-bounce frame) the
// kernel shades its ray into the path state and returns whether the path goes on.
// UNI: every lane of the wave holds a slot of the same tile (slot_coords); tile pairs: of either.
template <bool COUNT, bool PRIMARY, bool DEEP, int FUSE, int UNI = 1>
__device__ __forceinline__ bool trace_slot(PipeArgs& A, LdsView& L, int k, ort::Counters& cnt) {
    bool alive;
    ort_rng rng0;  // FUSE: the camera ray's RNG state, kept for the shading after the walk
    const ort::Ray ray = slot_ray<PRIMARY, UNI>(A, k, alive, FUSE ? &rng0 : nullptr);
    if (!alive) {
        if (FUSE == 1) shade_direct_padding<UNI>(A, k);
        if (FUSE == 2) {
            A.pd[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // never alive (ort_shade_kernel's hole)
            if (A.final_out && A.sample == A.pp.ns - 1) shade_direct_padding<UNI>(A, k);  // band padding rows
        }
        return false;
    }
    ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
    // camera rays (jittered: practically never a zero component) keep the plain check, which
    // costs the hot kernel less (C3 +0.7 %); bounce rays take zero components fast too
    if constexpr (PRIMARY && !COUNT && FUSE != 0) {
        if (A.hbits && ((A.hbits[k >> 5] >> (k & 31)) & 1u)) return false;  // ort_trace_split walks and shades it
    }
    if (A.exact_only || !(PRIMARY ? ort::fast_path_ok(ray, inv, 0.001f, ORT_MAXFLOAT) : ort::fast_prepare(A.S, ray, inv))) {
        A.defer_list[atomicAdd(A.sync, 1)] = k;  // ort_trace_exact walks (and, FUSE, shades) it
        if (PRIMARY && !COUNT && A.pcost) A.pcost[k] = 0;
        return false;
    }
    if (COUNT) cnt.v[5] += 1;
    float t = 0.0f;
    int entry = -1;
    using Masks = typename std::conditional<DEEP, ort::Masks96, ort::Masks64>::type;
    ort::Ray walked;
    int steps = 0;
    const bool hit = ort::traverse_fast_t<COUNT, Masks>(A.S, L.planes, L.lut, ray, inv, 0.001f, ORT_MAXFLOAT, entry, t,
                                                        L.fr, cnt, FUSE ? &walked : nullptr,
                                                        (PRIMARY && !COUNT) ? &steps : nullptr);
    if (PRIMARY && !COUNT) {  // the cost order's record for the next frame (cost_order_slot)
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(4))) const PipeArgs KernArgs;
        KernArgs* kp = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        uint16_t* pc = kp->pcost;
#else
        uint16_t* pc = A.pcost;
#endif
        if (pc) pc[k] = (uint16_t)min(steps, 65535);
    }
    if (FUSE) {
        // shade with the ray rebuilt from the walk state (bit-identical, no registers held
        // across the walk) and the RNG state kept from the camera ray (2 registers) -- 4 %
        // faster at C3 than regenerating both after the walk; the kernel arguments are re-read
        // through a laundered pointer: held across the walk they overflow the SGPRs
        int k2 = k;
        asm volatile("" : "+v"(k2));
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(4))) const PipeArgs KernArgs;  // the kernarg segment
        KernArgs* kp = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const PipeArgs A2 = *kp;
#else
        const PipeArgs& A2 = A;
#endif
        if constexpr (FUSE == 1) {
            shade_direct<UNI>(A2, k2, walked, rng0, hit, entry, t);
        } else {
            int col, row;
            (void)slot_coords<UNI>(A2, k2, col, row);
            out_coords(A2, row, col, -1, row, col);
            return shade_state<0, true, false>(A2, k2, row, col, walked, rng0, hit ? entry : -1, t);
        }
    } else {
        A.hit[k] = make_int2(hit ? entry : -1, __float_as_int(t));
    }
    return false;
}

// Cost order (ORT_OPT_COST_ORDER): a wave runs as long as its slowest lane, and the camera
// rays of one 8x8 block differ by up to several times in walk steps (background next to a
// sphere's silhouette).  Each workgroup deals its 256 slots to its 4 waves by the walk steps
// their rays took in the previous frame (pcost, a bucket per 4 steps, stable counting sort:
// equal buckets keep tile order), so rays of like cost share a wave.  Only which lane walks
// which slot changes -- every slot's ray, path state and pixel are the same (bit-identical
// frames).  A first frame (pcost cleared) keeps tile order.  Scratch: the first 512 ints of the
// frame columns (free before the walk; lds_bytes >= 2 levels).
#ifndef ORT_COST_SHIFT
// bucket = steps >> shift (64 buckets): 2-step buckets since tile pairs (C3 +1.3 % in A/B over
// 4-step ones, profiles/r04_c3_xr.log; with one tile per workgroup they measured alike)
#define ORT_COST_SHIFT 1
#endif
#ifndef ORT_COST_SHIFT_DEEP
#define ORT_COST_SHIFT_DEEP 2  // the depth 9-10 camera kernel's bucket width
#endif
template <int SHIFT>
__device__ __forceinline__ int cost_order_slot(const uint16_t* pcost, int* sc, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t b = min((uint32_t)pcost[k] >> SHIFT, 63u);
    uint64_t m = ~0ull;  // the lanes of this wave in the same bucket
    for (int i = 0; i < 6; ++i) {
        const uint64_t bal = __ballot((b >> i) & 1u);
        m &= ((b >> i) & 1u) ? bal : ~bal;
    }
    const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    int* cnt = sc;         // [wave][bucket]: lanes, then first position
    int* perm = sc + 256;  // position -> thread of the natural order
    cnt[tid] = 0;
    __syncthreads();
    if (below == 0) cnt[wave * 64 + b] = __popcll(m);
    __syncthreads();
    if (wave == 0) {  // lane = bucket: exclusive scan of the bucket totals
        const int c0 = cnt[lane], c1 = cnt[64 + lane], c2 = cnt[128 + lane], c3 = cnt[192 + lane];
        const int tot = c0 + c1 + c2 + c3;
        int incl = tot;
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        const int base = incl - tot;
        cnt[lane] = base;
        cnt[64 + lane] = base + c0;
        cnt[128 + lane] = base + c0 + c1;
        cnt[192 + lane] = base + c0 + c1 + c2;
    }
    __syncthreads();
    perm[cnt[wave * 64 + b] + below] = tid;
    __syncthreads();
    const int kk = (k & ~(kBlock - 1)) | perm[tid];
    __syncthreads();  // the frame columns are the walk's from here
    return kk;
#else
    (void)pcost;
    (void)sc;
    return k;
#endif
}

// Cost order over a tile pair (ORT_OPT_TILE_PAIRS): the 512 slots of workgroup b (slots 512b ..
// 512b + 511, two tiles) in eight blocks of 64 by last frame's walk steps (the stable counting
// sort of cost_order_slot, buckets of 2^SHIFT steps: 2 by default), and wave w walks block 7 - w and then block w: a
// workgroup holds its LDS until its slowest wave ends, and with one block per wave the cost
// order left 12-13 % of the waves' time idle inside the workgroups (tools/tile_clock.py); the
// longest-processing-time pairs (7,0) (6,1) (5,2) (4,3) even the waves out.  Scratch: the
// first 1024 ints of the frame columns (free before the walk; lds_bytes >= 4 levels).
template <int SHIFT>
__device__ __forceinline__ void cost_order_pair(const uint16_t* pcost, int* sc, int base, int& kk0, int& kk1) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t b0 = min((uint32_t)pcost[base + tid] >> SHIFT, 63u);
    const uint32_t b1 = min((uint32_t)pcost[base + 256 + tid] >> SHIFT, 63u);
    uint64_t m0 = ~0ull, m1 = ~0ull;  // the lanes of this wave in the same bucket, per item
    for (int i = 0; i < 6; ++i) {
        const uint64_t bal0 = __ballot((b0 >> i) & 1u), bal1 = __ballot((b1 >> i) & 1u);
        m0 &= ((b0 >> i) & 1u) ? bal0 : ~bal0;
        m1 &= ((b1 >> i) & 1u) ? bal1 : ~bal1;
    }
    const int below0 = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
    const int below1 = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
    int* cnt = sc;         // [virtual wave 0..7][bucket]: items, then first position
    int* perm = sc + 512;  // position -> item (0..511)
    cnt[tid] = 0;
    cnt[256 + tid] = 0;
    __syncthreads();
    if (below0 == 0) cnt[wave * 64 + b0] = __popcll(m0);
    if (below1 == 0) cnt[(4 + wave) * 64 + b1] = __popcll(m1);
    __syncthreads();
    if (wave == 0) {  // lane = bucket: exclusive scan of the bucket totals, then the virtual waves in order
        int c[8];
        int tot = 0;
        for (int v = 0; v < 8; ++v) {
            c[v] = cnt[v * 64 + lane];
            tot += c[v];
        }
        int incl = tot;
        for (int off = 1; off < 64; off <<= 1) {
            const int x = __shfl_up(incl, off);
            if (lane >= off) incl += x;
        }
        int pos = incl - tot;
        for (int v = 0; v < 8; ++v) {
            cnt[v * 64 + lane] = pos;
            pos += c[v];
        }
    }
    __syncthreads();
    perm[cnt[wave * 64 + b0] + below0] = tid;
    perm[cnt[(4 + wave) * 64 + b1] + below1] = 256 + tid;
    __syncthreads();
    kk0 = base + perm[64 * (7 - wave) + lane];
    kk1 = base + perm[64 * wave + lane];
    __syncthreads();  // the frame columns are the walk's from here
#else
    (void)pcost;
    (void)sc;
    kk0 = base + (int)threadIdx.x;
    kk1 = kk0 + 256;
#endif
}

// Analysis builds only (-DORT_TILE_CLOCK=1, tools/tile_clock.py): the per-tile camera-ray
// kernels record per wave {start, end, XCC id, the longest walk of its lanes} into wclock.
#ifndef ORT_TILE_CLOCK
#define ORT_TILE_CLOCK 0
#endif
#if ORT_TILE_CLOCK && defined(__HIP_DEVICE_COMPILE__)
template <bool ON>
__device__ inline void tile_clock_record(int k0, int k1, unsigned long long tclk0) {
    if (!ON) return;
    typedef __attribute__((address_space(4))) const PipeArgs KernArgs;
    KernArgs* kp = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    int st = kp->pcost ? max((int)kp->pcost[k0], (int)kp->pcost[k1]) : 0;
    for (int o = 32; o >= 1; o >>= 1) st = max(st, __shfl_xor(st, o));
    const int gw = (int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
    if (kp->wclock && (threadIdx.x & 63) == 0 && gw < kp->wclock_n) {
        const unsigned xcc = __builtin_amdgcn_s_getreg((15 << 11) | 20);  // XCC_ID
        kp->wclock[gw] = make_ulonglong4(tclk0, __builtin_amdgcn_s_memrealtime(), xcc & 15u, (unsigned long long)st);
    }
}
#endif
template <bool COUNT, bool PRIMARY, bool DEEP, int FUSE>
__device__ __forceinline__ void trace_compact_body(PipeArgs& A, unsigned char* smem) {
    if (!PRIMARY && A.qlist && (int)(blockIdx.x * kBlock) >= *A.qcount) return;  // whole block past the list
#if ORT_TILE_CLOCK && defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long tclk0 = __builtin_amdgcn_s_memrealtime();
#endif
    LdsView L = setup_lds<true>(smem, A.S);
    int k = blockIdx.x * kBlock + threadIdx.x;
    if (PRIMARY && !COUNT && A.pcost) {  // (the counting pass: tile order)
        k = cost_order_slot<DEEP ? ORT_COST_SHIFT_DEEP : ORT_COST_SHIFT>(A.pcost, L.fr.co, k);
#if defined(__HIP_DEVICE_COMPILE__)
        // heavy priority: the few waves holding the frame's longest walks start with the first
        // workgroups but, sharing their SIMD with 7 others, finish long after the rest of a small
        // tile (tools/tile_clock.py); they get the SIMD's issue slots first
        if (A.prio_steps > 0 && __ballot((int)A.pcost[k] >= A.prio_steps)) __builtin_amdgcn_s_setprio(3);
#endif
    }
    if (!PRIMARY && !list_slot(A, k)) return;
    ort::Counters cnt;
    for (int q = 0; q < 6; ++q) cnt.v[q] = 0;
    const bool go = trace_slot<COUNT, PRIMARY, DEEP, FUSE>(A, L, k, cnt);
    (void)go;
    if constexpr (FUSE == 2) {  // the paths that go on join the next bounce's list
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(4))) const PipeArgs KernArgs;
        KernArgs* kp = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        uint32_t key = 0;
        if (go && kp->qnext_keys) {  // the state just stored
            const float4 o = kp->po[k], d = kp->pd[k];
            key = ort::path_key(o, d, kp->mp, kp->key_spread) |
                  (kp->geo_heavy ? geo_class_bits(kp->gbox, kp->gthr, o, d) : light_bit(kp->bcost_r, kp->heavy, k));
        }
        append_slots(go, k, key, kp->qnext, kp->qnext_keys, kp->qnext_count);
#endif
    }
    flush_counts<COUNT>(cnt, A.counters);
#if ORT_TILE_CLOCK && defined(__HIP_DEVICE_COMPILE__)
    tile_clock_record<PRIMARY && !COUNT>(k, k, tclk0);
#endif
}

// Tile pairs (ORT_OPT_TILE_PAIRS): a workgroup renders the two tiles of pair blockIdx.x, each
// wave a heavy and then a light 64-slot block (cost_order_pair).  Between the blocks the kernel
// arguments are re-read through a laundered pointer (hoisted out of the loop they stay live
// across the walk and spill) and the second block's slot is kept in one VGPR.
template <bool COUNT, bool PRIMARY, bool DEEP, int FUSE>
__device__ __forceinline__ void trace_pair_body(PipeArgs& A, unsigned char* smem) {
#if ORT_TILE_CLOCK && defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long tclk0 = __builtin_amdgcn_s_memrealtime();
#endif
    LdsView L0 = setup_lds<true>(smem, A.S);
    const int base = blockIdx.x * (2 * kBlock);
    int kk0 = base + threadIdx.x, kk1 = kk0 + kBlock;
    if (!COUNT && A.pcost) cost_order_pair<DEEP ? ORT_COST_SHIFT_DEEP : ORT_COST_SHIFT>(A.pcost, L0.fr.co, base, kk0, kk1);
    ort::Counters cnt;
    for (int q = 0; q < 6; ++q) cnt.v[q] = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(4))) const PipeArgs KernArgs;
        KernArgs* kp = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        PipeArgs A1 = *kp;
#else
        PipeArgs& A1 = A;
#endif
        LdsView L = lds_view<true>(smem, A1.S.depth);
        int k = j ? kk1 : kk0;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(k));
        if (!COUNT && A1.pcost && A1.prio_steps > 0) {  // heavy priority, per block
            if (__ballot((int)A1.pcost[k] >= A1.prio_steps)) __builtin_amdgcn_s_setprio(3);
            else __builtin_amdgcn_s_setprio(0);
        }
#endif
        const bool go = trace_slot<COUNT, PRIMARY, DEEP, FUSE, 2>(A1, L, k, cnt);
        (void)go;
        if constexpr (FUSE == 2) {  // the paths that go on join the next bounce's list
#if defined(__HIP_DEVICE_COMPILE__)
            KernArgs* kq = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
            uint32_t key = 0;
            if (go && kq->qnext_keys) {
                const float4 o = kq->po[k], d = kq->pd[k];
                key = ort::path_key(o, d, kq->mp, kq->key_spread) |
                      (kq->geo_heavy ? geo_class_bits(kq->gbox, kq->gthr, o, d) : light_bit(kq->bcost_r, kq->heavy, k));
            }
            append_slots(go, k, key, kq->qnext, kq->qnext_keys, kq->qnext_count);
#endif
        }
    }
    flush_counts<COUNT>(cnt, A.counters);
#if ORT_TILE_CLOCK && defined(__HIP_DEVICE_COMPILE__)
    tile_clock_record<PRIMARY && !COUNT>(kk0, kk1, tclk0);
#endif
}

// FUSE: 1 sample, 1 bounce -- the kernel also shades (shade_direct), no hit records.
template <bool COUNT, bool PRIMARY, int FUSE>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_TRACE_WAVES))) ort_trace_compact(PipeArgs A) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];  // plane tables: 1 KiB-aligned
    trace_compact_body<COUNT, PRIMARY, false, FUSE>(A, smem);
}
template <bool COUNT, bool PRIMARY, int FUSE>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_TRACE_WAVES_DEEP)))
ort_trace_compact_deep(PipeArgs A) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];  // plane tables: 1 KiB-aligned
    trace_compact_body<COUNT, PRIMARY, true, FUSE>(A, smem);
}
// camera rays, tile pairs (ORT_OPT_TILE_PAIRS)
template <bool COUNT, int FUSE>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_TRACE_WAVES))) ort_trace_pair(PipeArgs A) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];  // plane tables: 1 KiB-aligned
    trace_pair_body<COUNT, true, false, FUSE>(A, smem);
}
template <bool COUNT, int FUSE>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_TRACE_WAVES_DEEP)))
ort_trace_pair_deep(PipeArgs A) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];  // plane tables: 1 KiB-aligned
    trace_pair_body<COUNT, true, true, FUSE>(A, smem);
}
// Heavy camera rays (ORT_OPT_SPLIT_HEAVY): the slots whose walk took >= T steps in the previous
// frame (pcost), listed (the first `cap` of them) and marked in a bitmap the per-tile kernel
// reads.  A wave's slots are listed in slot order after one atomic.
// One wave scans 1024 slots from `base` (a multiple of 1024; n a multiple of 256): 16 per lane,
// read as two 16-byte loads, one atomic per wave, each lane pair writing one bitmap word.
struct HeavyScan {
    const uint16_t* pcost;
    int n, T, cap;
    uint32_t* bits;
    int* list;
    int* count;
};
__device__ inline void heavy_scan_wave(const HeavyScan& H, int base) {
    const int lane = threadIdx.x & 63;
    const int s0 = base + 16 * lane;
    uint32_t m = 0;
    if (s0 < H.n) {
        const uint4 a = *(const uint4*)(H.pcost + s0), b = *(const uint4*)(H.pcost + s0 + 8);
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        for (int i = 0; i < 8; ++i) {
            m |= (uint32_t)((int)(w[i] & 0xffffu) >= H.T) << (2 * i);
            m |= (uint32_t)((int)(w[i] >> 16) >= H.T) << (2 * i + 1);
        }
    }
    const int c = __popc(m);
    int incl = c;  // inclusive scan of the lanes' counts
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    const int total = __shfl(incl, 63);
    int at = 0;
    if (lane == 0 && total) at = atomicAdd(H.count, total);
    int pos = __shfl(at, 0) + incl - c;
    uint32_t mh = 0;  // the listed ones (past the cap the per-tile kernel walks them itself)
    for (uint32_t r = m; r; r &= r - 1, ++pos) {
        const int i = __builtin_ctz(r);
        if (pos < H.cap) {
            H.list[pos] = s0 + i;
            mh |= 1u << i;
        }
    }
    const uint32_t other = (uint32_t)__shfl_xor((int)mh, 1);
    if (s0 < H.n && !(lane & 1)) H.bits[s0 >> 5] = mh | (other << 16);
}
__global__ void __launch_bounds__(kBlock) k_heavy_scan(HeavyScan H) {
    for (int base = (int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 1024; base < H.n;
         base += (int)(gridDim.x * (kBlock / 64)) * 1024)
        heavy_scan_wave(H, base);
}

// The heavy camera rays of k_heavy_scan's list, each walked by a group of 8 lanes that deal its
// walk's level-split_level subtrees round robin (traverse_split), then shaded like the per-tile
// kernel shades (FUSE 1: shade_direct).  Runs on the context's second stream beside the per-tile
// kernel and ahead of it in the GPU's dispatch, at raised issue priority: the frame's longest
// walks, run by one lane each, are what a small tile's frame waits for (tools/tile_clock.py).
constexpr int kSplitLanes = 8;
template <bool DEEP, int FUSE>
__global__ void __launch_bounds__(kBlock) ort_trace_split(PipeArgs A) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];  // plane tables: 1 KiB-aligned
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_s_setprio(3);
#endif
#if ORT_TILE_CLOCK && defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long sclk0 = __builtin_amdgcn_s_memrealtime();
    int sitems = 0;
#endif
    if (A.hsync_next && blockIdx.x == 0 && threadIdx.x < 2) A.hsync_next[threadIdx.x] = 0;
    const int count = min(A.hsync[0], A.hcap);
    if (count == 0) return;
    LdsView L = setup_lds<true>(smem, A.S);
    using Masks = typename std::conditional<DEEP, ort::Masks96Split, ort::Masks64Split>::type;
    const int lane = threadIdx.x & 63, g = lane / kSplitLanes, j = lane % kSplitLanes;
    constexpr int kNoHit = 0x7fffffff;
    for (;;) {
        int base = 0;
        if (lane == 0) base = atomicAdd(A.hsync + 1, 64 / kSplitLanes);
        base = __shfl(base, 0);
        if (base >= count) break;
        const int idx = base + g;
        const int k = idx < count ? A.hlist[idx] : -1;
#if ORT_TILE_CLOCK && defined(__HIP_DEVICE_COMPILE__)
        sitems += min(64 / kSplitLanes, count - base);
#endif
        int pos = kNoHit, entry = -1, steps = 0, own = 0;
        float t = 0.0f;
        bool walked = false;
        ort_rng rng0;
        ort::Ray ray;
        ray.o = ray.d = ort::mk(0.0f, 0.0f, 0.0f);
        if (k >= 0) {
            bool alive;
            ray = slot_ray<true>(A, k, alive, &rng0);
            const ort::V3 inv = ort::mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
            if (alive && !A.exact_only && ort::fast_path_ok(ray, inv, 0.001f, ORT_MAXFLOAT)) {
                walked = true;
                ort::traverse_split<Masks>(A.S, L.planes, L.lut, ray, inv, A.split_level, kSplitLanes, j, pos, entry, t,
                                           L.fr, steps, own);
            } else if (alive && j == 0) {  // (a moved camera: rare) the exact kernel walks and shades it
                A.defer_list[atomicAdd(A.sync, 1)] = k;
                if (A.pcost) A.pcost[k] = 0;
            }
        }
        // the group's result: the hit with the lowest DFS position; the walk's steps as ONE walk
        // would take them (the next frame's cost order and heavy list read them): the longest
        // stretch above the level plus every lane's own subtree steps
        steps -= own;
        for (int o = 1; o < kSplitLanes; o <<= 1) {
            const int op = __shfl_xor(pos, o, kSplitLanes);
            const int oe = __shfl_xor(entry, o, kSplitLanes);
            const float ot = __shfl_xor(t, o, kSplitLanes);
            if (op < pos) {
                pos = op;
                entry = oe;
                t = ot;
            }
            steps = max(steps, __shfl_xor(steps, o, kSplitLanes));
            own += __shfl_xor(own, o, kSplitLanes);
        }
        steps += own;
        if (walked && j == 0) {
            if (A.pcost) A.pcost[k] = (uint16_t)min(steps, 65535);
            if constexpr (FUSE == 1) {
                shade_direct(A, k, ray, rng0, pos != kNoHit, entry, t);
            } else {  // bounce 0 of a multi-bounce frame: path state, and the next bounce's list
                int col, row;
                (void)slot_coords(A, k, col, row);
                out_coords(A, row, col, -1, row, col);
                if (shade_state<0, true, false>(A, k, row, col, ray, rng0, pos != kNoHit ? entry : -1, t)) {
                    const int q = atomicAdd(A.qnext_count, 1);
                    A.qnext[q] = k;
                    if (A.qnext_keys)
                        A.qnext_keys[q] = path_key_class(A, k);
                }
            }
        }
    }
#if ORT_TILE_CLOCK && defined(__HIP_DEVICE_COMPILE__)
    {   // analysis: per wave {start, end, 1 << 63 (a split-kernel record), rays walked}, from the records' end
        const int gw = (int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
        if (A.wclock && (threadIdx.x & 63) == 0 && gw < A.wclock_n)
            A.wclock[A.wclock_n - 1 - gw] =
                make_ulonglong4(sclk0, __builtin_amdgcn_s_memrealtime(), 1ull << 63, (unsigned long long)sitems);
    }
#endif
}

// One-ray-per-lane trace for the explicit layout (MODE 1) and brute force (MODE 2).
template <int MODE, bool COUNT, bool PRIMARY>
__global__ void __launch_bounds__(kBlock) ort_trace_kernel(PipeArgs A) {
    int k = blockIdx.x * kBlock + threadIdx.x;
    if (!PRIMARY && !list_slot(A, k)) return;
    bool alive;
    const ort::Ray ray = slot_ray<PRIMARY>(A, k, alive);
    if (!alive) return;
    ort::Counters cnt;
    for (int q = 0; q < 6; ++q) cnt.v[q] = 0;
    ort::LocalFrames unused;
    float t;
    int entry;
    int st;
    if constexpr (MODE == 1) {
        int snode[ORT_MAX_STACK];
        float stmin[ORT_MAX_STACK];
        st = ort::trace_ray<MODE, COUNT>(A.S, nullptr, nullptr, ray, false, t, entry, unused, snode, stmin, cnt);
    } else {
        st = ort::trace_ray<MODE, COUNT>(A.S, nullptr, nullptr, ray, false, t, entry, unused, nullptr, nullptr, cnt);
    }
    A.hit[k] = make_int2(st == ORT_TRACE_HIT ? entry : -1, __float_as_int(t));
    flush_counts<COUNT>(cnt, A.counters);
}

// Exact compact walk (traverse_compact) for the deferred rays; grid-stride loop.
template <bool COUNT, bool PRIMARY, int FUSE>
__global__ void __launch_bounds__(kBlock) ort_trace_exact(PipeArgs A) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];  // plane tables: 1 KiB-aligned
    const int n = *A.sync;
    // the next launch's counters (the other set: its last users ended before this launch began),
    // instead of a memset node per launch (a fill kernel: ~5 us of a 0.33 ms band frame)
    if (A.sync_next && blockIdx.x == 0 && threadIdx.x < 16) A.sync_next[threadIdx.x] = 0;
    if (A.scan_pcost) {  // the next frame's heavy list from this frame's final steps (split frames)
        const HeavyScan H{A.scan_pcost, (int)A.total, A.scan_T, A.hcap, A.scan_bits, A.scan_list, A.scan_count};
        for (int base = (int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 1024; base < H.n;
             base += (int)(gridDim.x * (kBlock / 64)) * 1024)
            heavy_scan_wave(H, base);
    }
    if ((int)(blockIdx.x * kBlock) >= n) return;  // usually no deferred ray at all: skip the LDS image copy
    LdsView L = setup_lds<false>(smem, A.S);
    ort::Counters cnt;
    for (int q = 0; q < 6; ++q) cnt.v[q] = 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int k = A.defer_list[i];
        bool alive;
        ort_rng rng;
        const ort::Ray ray = slot_ray<PRIMARY>(A, k, alive, FUSE ? &rng : nullptr);
        float t;
        int entry;
        const int st = ort::trace_ray<0, COUNT>(A.S, L.planes, nullptr, ray, false, t, entry, L.fr, nullptr, nullptr, cnt);
        if (FUSE == 1) {
            shade_direct(A, k, ray, rng, st == ORT_TRACE_HIT, entry, t);
        } else if (FUSE == 2) {  // bounce 0 shaded here; the rare deferred path joins the list alone
            int col, row;
            (void)slot_coords(A, k, col, row);
            out_coords(A, row, col, -1, row, col);
            if (shade_state<0, true, false>(A, k, row, col, ray, rng, st == ORT_TRACE_HIT ? entry : -1, t)) {
                const int pos = atomicAdd(A.qnext_count, 1);
                A.qnext[pos] = k;
                if (A.qnext_keys)
                    A.qnext_keys[pos] = path_key_class(A, k);
            }
        } else {
            A.hit[k] = make_int2(st == ORT_TRACE_HIT ? entry : -1, __float_as_int(t));
        }
    }
    flush_counts<COUNT>(cnt, A.counters);
}

// Bounce shading (glsl:607-627) of path slot k.  FIRST: bounce 0 (c = 1, importance = 1).
// DIRECT (1 sample, 1 bounce): writes the final pixel.  Returns true when the path goes on
// to the next bounce.
template <int MODE, bool FIRST, bool DIRECT, bool PLAIN = false>
__device__ __forceinline__ bool shade_slot(const PipeArgs& A, int k) {
    int col, row;
    const bool in_tile = FIRST ? slot_coords<true>(A, k, col, row) : slot_coords(A, k, col, row);
    const int y = in_tile ? tile_row_to_y(A.tm, row) : 0;
    if (!in_tile || y >= A.pp.H) {
        if (DIRECT && in_tile) store_padding(A, row, col);
        if (FIRST && !DIRECT) A.pd[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // never alive (compaction)
        return false;
    }
    bool alive = true;
    ort::Ray ray;
    ort_rng st;
    if (FIRST) {
        if (A.sample == 0) {
            ort::pixel_rng_init(A.pp, A.tm.x0 + col, y, st);
        } else {
            const float2 v = A.prng[k];
            st.x = v.x;
            st.y = v.y;
        }
        ray = ort::primary_ray(A.pp, A.tm.x0 + col, y, A.sample, st);
    } else {
        ray = load_ray(A, k, alive);
        if (!alive) return false;
        const float2 r2 = A.prng[k];
        st.x = r2.x;
        st.y = r2.y;
    }
    int2 h = make_int2(-1, 0);
    if (!A.nobounce) h = A.hit[k];
    int orow, ocol;
    out_coords<PLAIN>(A, row, col, y, orow, ocol);
    return shade_state<MODE, FIRST, DIRECT, PLAIN>(A, k, orow, ocol, ray, st, h.x, __int_as_float(h.y));
}


// Shades every path slot of its workgroup (slot order); with A.qnext, the paths that go on
// are appended to the next bounce's list (the compaction, without a separate select pass).
template <int MODE, bool FIRST, bool DIRECT, bool PLAIN>
__device__ __forceinline__ void shade_kernel_body(const PipeArgs& A) {
    int k = blockIdx.x * kBlock + threadIdx.x;
    bool in = true;
    if (!FIRST && A.qlist) {  // the bounce's alive paths in append order (not the sorted trace list)
        const int n = *A.qcount;
        if ((int)(blockIdx.x * kBlock) >= n) return;  // whole workgroup past the list
        in = k < n;
        if (in) k = A.qlist[k];
    }
    const bool go = in && shade_slot<MODE, FIRST, DIRECT, PLAIN>(A, k);
    if (!DIRECT && A.qnext) {
        uint32_t key = 0;
        if (go && A.qnext_keys)  // the state just stored
            key = path_key_class(A, k);
        append_slots(go, k, key, A.qnext, A.qnext_keys, A.qnext_count);
    }
}
// The bounce-0 instance (FIRST, not DIRECT) is compiled for ort_render's own output alone (RGB32F,
// tile placement, tight rows); a frame of any other output runs ort_shade_first_any for that
// bounce (launch_shade_mode).
template <int MODE, bool FIRST, bool DIRECT>
__global__ void __launch_bounds__(kBlock) ort_shade_kernel(PipeArgs A) {
    shade_kernel_body<MODE, FIRST, DIRECT, FIRST && !DIRECT>(A);
}
template <int MODE>
__global__ void __launch_bounds__(kBlock) ort_shade_first_any(PipeArgs A) {
    shade_kernel_body<MODE, true, false, false>(A);
}

// col / ns, gamma (glsl:659-661) for the multi-sample / multi-bounce case.
__global__ void __launch_bounds__(kBlock) ort_finalize_kernel(PipeArgs A) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    int col, row;
    if (!slot_coords<true>(A, k, col, row)) return;
    const int y = tile_row_to_y(A.tm, row);
    if (y >= A.pp.H) {
        store_padding(A, row, col);
        return;
    }
    ort::V3 acc = ort::mk(0.0f, 0.0f, 0.0f);
    if (A.pp.ns > 0) {
        const float4 a = A.pcol[k];
        acc = ort::mk(a.x, a.y, a.z);
    }
    store_pixel(A, row, col, y, ort::finish_pixel(acc, A.pp.ns));
}

// ---------------------------------------------------------------------------------------
// Whole-pixel paths (ORT_OPT_PIXEL_PATHS): main() of the fragment shader (glsl:636-664) for
// every pixel in ONE launch -- all samples, all bounces -- instead of the wavefront pipeline's
// per-sample, per-bounce launches (trace, exact walk, shade, list sort: ~10 launches per bounce).
// Samples cannot be batched across launches: the RNG state runs on from one sample to the next
// (randState, glsl:640), so a pixel's samples are a sequential chain.  Each lane therefore owns
// a pixel and steps it one bounce at a time, regenerating the path when it ends (the pixel's
// next sample starts in the same iteration: lanes stay on the walk code whatever sample or
// bounce they are at), and a lane whose pixel is done takes the next pixel of its wave's chunk
// (persistent grid, one atomic per 64-pixel chunk, pixels in the tile-block order of the path
// slots: a chunk is an 8x8 block).  Every pixel runs exactly shade_pixel's chain (render_core.h),
// so the frames are the pipeline's bit for bit.  MODE 0: compact octree (DEEP: depth 9-10, the
// camera walk's 96-bit masks over the forward tables; else the bounce walk's Masks64Plain), the
// exact walk inline for the rays the fast walk cannot take; MODE 2: brute force.
// The grid's work cursor and done count (A.sync[1], [2]) start at zero (the counter set of the
// launch) and the last workgroup to finish resets them.
template <int MODE, bool DEEP, bool LDS>
__device__ __forceinline__ bool pixel_trace(const PipeArgs& A, const ort::KScene& S, LdsView& L, const ort::Ray& r,
                                            float& t, int& entry) {
    ort::Counters cnt;  // (not counted: counting renders take the pipeline)
    entry = -1;
    t = 0.0f;
    if (MODE == 2) return ort::traverse_brute<false>(S, r, 0.001f, ORT_MAXFLOAT, entry, t, cnt);
    ort::V3 inv = ort::mk(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
    if (!A.exact_only && ort::fast_prepare(S, r, inv)) {
        using Masks = typename std::conditional<DEEP, ort::Masks96,
                                                typename std::conditional<LDS, ort::Masks64PlainLds, ort::Masks64Plain>::type>::type;
        return ort::traverse_fast_t<false, Masks>(S, L.planes, L.lut, r, inv, 0.001f, ORT_MAXFLOAT, entry, t, L.fr, cnt);
    }
    return ort::traverse_compact<false>(S, L.planes, r, 0.001f, ORT_MAXFLOAT, entry, t, L.fr, cnt);
}

// Whole-pixel paths take last frame's heaviest 8x8 blocks first (ORT_OPT_PIXEL_HEAVY_FIRST).
constexpr int kPixelClasses = 32;  // cost classes of a block: mean bounces per sample in quarters
// Accounts one slot of a block (a finished pixel and the bounces it traced, or a slot that is no
// pixel): the block's last slot files the block under its cost class for the next frame and
// clears its accumulator (cost in the high word, slots in the low word).
__device__ __forceinline__ void block_account(const PipeArgs& A, int slot, int bounces) {
    unsigned long long* acc = A.pl_cost + (slot >> 6);
    const unsigned long long add = ((unsigned long long)min(bounces, 1 << 24) << 32) | 1ull;
    const unsigned long long old = atomicAdd(acc, add);
    if ((unsigned)(old & 0xffffffffu) == 63u) {
        const unsigned long long cost = (old >> 32) + (unsigned long long)min(bounces, 1 << 24);
        *acc = 0;
        const unsigned long long quarters = cost / (16ull * (unsigned long long)A.pp.ns);
        const int q = kPixelClasses - 1 - (int)min(quarters, (unsigned long long)(kPixelClasses - 1));
        const int pos = atomicAdd(A.pl_wcnt + q, 1);
        A.pl_w[(size_t)q * A.pl_stride + pos] = slot >> 6;
    }
}

#ifndef ORT_PIXEL_WAVES
#define ORT_PIXEL_WAVES 4
#endif


// LDS: small scenes (depth <= 8) walk the workgroup's copies of nk[] and leaf_sph[] in LDS
// (ds_read, ~50 cycles) instead of global memory: the kernel waits on memory for most of its
// cycles (SQ_WAIT_ANY 0.64 at config.h's default scene, profiles/r06/), and a walk is a chain
// of dependent record loads.
// SPEC: samples in parallel.  A pixel's samples form a chain only through the RNG state, and
// the state a sample ends with depends on the path only through how many draws it took -- so
// with a static or slowly moving camera it repeats from frame to frame.  SPEC launches take
// (8x8 block, sample s) items: sample s >= 1 starts from the state sample s-1 ended with LAST
// frame (sp_prev), writes its radiance and end state, and flags the pixel when its end state
// differs from last frame's -- the samples after it then started from a wrong state.
// ort_sample_resolve sums each pixel's samples in order up to the first flagged one and lists
// the pixels that need the rest; a whole-pixel launch over that list (fx_*) continues them
// from the true state.  Every pixel's samples are thus the sequential chain's, summed in the
// chain's order: the frames stay bit-identical, and a frame is no longer as long as its longest
// pixel's chain (16 samples x 8 bounces at config.h's default).
// PM: 0 whole pixels, 1 SPEC samples, 2 whole pixels that record their samples' end states or
// run the fixup list (kept apart from 0: its registers are the ones-sample frames' too), 3 a pass
// of an accumulation (accum.inc: samples A.sample .. A.sp_chunk - 1 of every pixel, the chains'
// states and sums kept per slot between passes; instantiated there, after every kernel of this file),
// 4 a pass that also keeps the slot's second luminance moment m2 (accum_moments.inc, after every other
// kernel): the plane after the three colour-sum planes, read, added to and written at each sample's
// end -- sample ends are rare next to walk steps, and nothing more lives across the walk,
// 5 an adaptive pass (adaptive.inc, after every other kernel): a moments pass in which every pixel
// starts at its own count, the int plane after m2, and only where adaptive_traces says so; its end
// sample is recomputed at each sample's end from the still-unwritten count, as m2 is; with fx_slot it
// takes its candidates from that list of *fx_n slots (the pre-pass listed the pixels to trace) instead
// of the tile's blocks.  (The host sends it in tile order only where the decision can find nothing but
// k >= N, and the pre-pass has decided for a list; the full decision stays at the refill all the same:
// with the plain s >= ns test in its place the all-traced pass measured 4.5 % slower on stats114)
ORT_FN bool adaptive_traces(int k, int N, int min_samples, float threshold, float luminance_floor, ort::V3 col, float m2);
template <int MODE, bool DEEP, bool LDS, int PM = 0>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ORT_PIXEL_WAVES)))
ort_pixel_paths(PipeArgs A) {
    constexpr bool SPEC = PM == 1;
    constexpr bool PASS = PM == 3 || PM == 4 || PM == 5;
    // a SPEC launch in a fall-back frame, and the fixup launch's workgroups beyond what its list
    // needs, only count themselves out (before any LDS set-up)
    const bool idle_wg = (SPEC && A.sp_ctl[2] == 0) ||
                         ((PM == 2 || PM == 5) && A.fx_slot && (long long)blockIdx.x * kBlock >= (long long)*A.fx_n + kBlock);
    if (idle_wg) {
        if (threadIdx.x == 0 && atomicAdd(A.sync + 2, 1) == (int)gridDim.x - 1) {
            atomicExch(A.sync + 1, 0);
            atomicExch(A.sync + 2, 0);
            if (PM == 2 && A.fx_slot) {
                if (A.sp_ctl[2]) atomicExch(A.sp_ctl + 1, *A.fx_n);  // speculated: the list = the moved pixels
                atomicExch(A.fx_n, 0);
            }
        }
        return;
    }
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];  // plane tables: 1 KiB-aligned
    LdsView L{};
    ort::KScene S = A.S;
    if (LDS) {  // before setup_lds's barrier
        uint4* dn = reinterpret_cast<uint4*>(smem + A.lds_nk_off);
        uint4* ds = reinterpret_cast<uint4*>(smem + A.lds_sph_off);
        const uint4* sl = reinterpret_cast<const uint4*>(A.S.leaf_sph);
        for (int i = threadIdx.x; i < A.lds_nk_n16; i += kBlock) dn[i] = A.S.nk[i];
        for (int i = threadIdx.x; i < A.lds_sph_n16; i += kBlock) ds[i] = sl[i];
        S.lds_nk = (uint32_t)(size_t)(const __attribute__((address_space(3))) unsigned char*)(smem + A.lds_nk_off);
        S.lds_sph = (uint32_t)(size_t)(const __attribute__((address_space(3))) unsigned char*)(smem + A.lds_sph_off);
    }
    if (MODE == 0) L = setup_lds<true>(smem, A.S);
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int maxd = A.pp.maxDepth, ns = A.pp.ns;
    // the work items: 8x8 blocks, last frame's heaviest class first (a longest-first list
    // schedule: a frame ends with its longest pixels -- a pixel's samples run one after another --
    // and a block keeps its pixels' rays coherent), else in tile order; SPEC: (block, sample)
    // pairs, a block's samples one after another; the fixup list: 64 of its entries at a time.
    // Lane q < 32 holds the inclusive prefix of the class counts.
    const bool fixup = PM == 2 && A.fx_slot;
    const bool alist = PM == 5 && A.fx_slot;  // an adaptive pass over the listed slots (adaptive.inc), 64 entries at a time
    const int n_alist = alist ? *A.fx_n : 0;   // (read once: nothing appends during the pass)
    const int n_blocks = A.total >> 6;
    const int n_items = SPEC ? n_blocks * A.sp_nch : (fixup ? (*A.fx_n + 63) >> 6 : (alist ? (n_alist + 63) >> 6 : n_blocks));
    int cls_end = 0;
    if (A.pl_r) {
        cls_end = lane < kPixelClasses ? A.pl_rcnt[lane] : 0;
        for (int d = 1; d < kPixelClasses; d <<= 1) {
            const int v = __shfl_up(cls_end, d);
            if (lane >= d) cls_end += v;
        }
    }
    const bool listed = !fixup && A.pl_r && __shfl(cls_end, kPixelClasses - 1) == n_blocks;
    int k = -1;              // the lane's path slot (pixel), -1 idle
    int nb = 0;              // bounces traced for the lane's pixel so far (its cost class)
    int px = 0, py = 0, s = 0, b = 0;
    ort::Ray ray;
    ray.o = ray.d = ort::mk(0.0f, 0.0f, 0.0f);
    ort::V3 c = ort::mk(1.0f, 1.0f, 1.0f), col = ort::mk(0.0f, 0.0f, 0.0f);
    float importance = 1.0f;
    ort_rng st;
    st.x = st.y = 0.0f;
    int next = 0, end = 0;   // wave-uniform: the rest of the wave's block (or fixup entries)
    int item_s = 0;          // wave-uniform, SPEC: the sample of those slots
    bool drained = false;    // wave-uniform: the cursor passed the last item
#if ORT_PIXEL_CLOCK  // analysis: per wave the cycles of the refill, the walk and the shading, and the walk's lanes
    unsigned long long ck_refill = 0, ck_trace = 0, ck_shade = 0, ck_iter = 0, ck_lanes = 0, ck_t = 0;
    const unsigned long long ck_rt0 = __builtin_amdgcn_s_memrealtime();
#define ORT_CK_MARK(acc)                                            \
    do {                                                            \
        const unsigned long long now = __builtin_amdgcn_s_memtime(); \
        acc += now - ck_t;                                          \
        ck_t = now;                                                 \
    } while (0)
#else
#define ORT_CK_MARK(acc) do { } while (0)
#endif
    for (;;) {
#if ORT_PIXEL_CLOCK
        ck_t = __builtin_amdgcn_s_memtime();
#endif
        const unsigned long long idle = __ballot(k < 0);
        if (idle && !drained) {  // refill: idle lanes take the item's next pixels
            if (next == end) {  // the next item
                int j = 0;
                if (lane == 0) j = atomicAdd(A.sync + 1, 1);
                j = __shfl(j, 0);
                if (j >= n_items) {
                    drained = true;
                } else if (fixup || alist) {
                    next = j << 6;
                    end = min(next + 64, alist ? n_alist : *A.fx_n);
                } else {  // SPEC: block j / nch (its pixels' chunk j % nch), heavy blocks first as well
                    const int jb = SPEC ? j / A.sp_nch : j;
                    int blk = jb;
                    if (listed) {  // item jb of the class lists: class q = the first with jb < its prefix end
                        const unsigned long long in = __ballot(lane < kPixelClasses && jb < cls_end);
                        const int q = __builtin_ctzll(in);
                        const int before = q ? __shfl(cls_end, q - 1) : 0;
                        blk = A.pl_r[(size_t)q * A.pl_stride + (jb - before)];
                    }
                    next = blk << 6;
                    end = next + 64;
                    if (SPEC) item_s = j - jb * A.sp_nch;
                }
            }
            if (!drained) {
                const int n_idle = __popcll(idle);
                const int take = min(n_idle, end - next);
                if (k < 0) {
                    const int rank = __popcll(idle & below);
                    if (rank < take) {
                        const int cand = fixup || alist ? A.fx_slot[next + rank] : next + rank;
                        bool pixel = false;
                        int cx, cy;
                        if (slot_coords(A, cand, cx, cy)) {
                            const int y = tile_row_to_y(A.tm, cy);
                            if (y < A.pp.H) {  // a pixel: its first sample's camera ray
                                k = cand;
                                nb = 0;
                                px = A.tm.x0 + cx;
                                py = y;
                                b = 0;
                                c = ort::mk(1.0f, 1.0f, 1.0f);
                                importance = 1.0f;
                                if (SPEC) {  // chunk item_s from last frame's end state of chunk item_s - 1
                                    s = item_s * A.sp_chunk;
                                    if (item_s == 0) {
                                        ort::pixel_rng_init(A.pp, px, py, st);
                                    } else {
                                        const float2 v = A.sp_prev[(size_t)(item_s - 1) * A.total + k];
                                        st.x = v.x;
                                        st.y = v.y;
                                    }
                                } else if (fixup) {  // the rest of the pixel's chain from its true state
                                    const int e = next + rank;
                                    s = A.fx_s0[e];
                                    const float2 v = A.fx_st[e];
                                    st.x = v.x;
                                    st.y = v.y;
                                    col = ort::mk(A.fx_col[e], A.fx_col[(size_t)A.total + e], A.fx_col[2 * (size_t)A.total + e]);
                                } else if (PASS) {  // the pass's first sample, from the slot's stored state and sum
                                    s = A.sample;
                                    if (PM == 5 && s != 0) s = (reinterpret_cast<const int*>(A.fx_col) + 4 * (size_t)A.total)[k];  // the pixel's own count
                                    if (s == 0) {
                                        ort::pixel_rng_init(A.pp, px, py, st);
                                        col = ort::mk(0.0f, 0.0f, 0.0f);
                                    } else {
                                        const float2 v = A.fx_st[k];
                                        st.x = v.x;
                                        st.y = v.y;
                                        col = ort::mk(A.fx_col[k], A.fx_col[(size_t)A.total + k], A.fx_col[2 * (size_t)A.total + k]);
                                    }
                                } else {
                                    ort::pixel_rng_init(A.pp, px, py, st);
                                    s = 0;
                                    col = ort::mk(0.0f, 0.0f, 0.0f);
                                }
                                if (PM == 5) {  // adaptive: held pixels only show their stored sum
                                    const float m2 = s >= 2 ? A.fx_col[3 * (size_t)A.total + k] : 0.0f;
                                    if (!adaptive_traces(s, ns, A.hcap, A.gthr[0], A.gthr[1], col, m2)) {
                                        if (A.out) store_pixel(reread_args(A), cy, cx, py, ort::finish_pixel(col, s));
                                        k = -1;
                                    }
                                }
                                if (PM != 5 || k >= 0) ray = ort::primary_ray(A.pp, px, py, s, st);
                                pixel = true;
                            } else if (PASS) {  // ... of an accumulation pass: with a picture only
                                if (A.out) store_padding(reread_args(A), cy, cx);
                            } else if (!SPEC) {  // a band's padding row (past the frame): zeros, as the pipeline writes
                                store_padding(reread_args(A), cy, cx);
                            }
                        }
                        if (!SPEC && A.pl_w && !pixel) block_account(A, cand, 0);
                    }
                }
                next += take;
            }
        }
        ORT_CK_MARK(ck_refill);
        if (!__ballot(k >= 0)) {
            if (drained) break;
            continue;
        }
#if ORT_PIXEL_CLOCK
        ck_iter += 1;
        ck_lanes += __popcll(__ballot(k >= 0));
#endif
        if (k >= 0) {  // one bounce of the lane's current path (radiance(), glsl:604-627)
            float t;
            int entry;
            const bool hit = pixel_trace<MODE, DEEP, LDS>(A, S, L, ray, t, entry);
#if ORT_PIXEL_CLOCK
            __builtin_amdgcn_wave_barrier();
#endif
            ORT_CK_MARK(ck_trace);
            ort::HitRec h;
            if (hit) h = ort::hit_record<MODE>(A.S, ray, t, entry);
            bool ended = ort::shade_bounce(hit, h, ray, c, importance, st);
            ++b;
            ++nb;
            ended = ended || b >= maxd || importance < 0.01f;
            if (ended && SPEC) {  // the sample's radiance; the chunk's next sample, or its end state
                const size_t i = (size_t)s * A.total + k;
                A.sp_col[i] = c.x;
                A.sp_col[(size_t)ns * A.total + i] = c.y;
                A.sp_col[2 * (size_t)ns * A.total + i] = c.z;
                if (++s < ns && s % A.sp_chunk != 0) {
                    b = 0;
                    c = ort::mk(1.0f, 1.0f, 1.0f);
                    importance = 1.0f;
                    ray = ort::primary_ray(A.pp, px, py, s, st);
                } else {
                    A.sp_cur[(size_t)((s - 1) / A.sp_chunk) * A.total + k] = make_float2(st.x, st.y);
                    k = -1;
                }
            } else if (ended) {  // col += radiance(r) (glsl:655); the pixel's next sample, or its final colour
                col = ort::add(col, c);
                if (PM == 4 || PM == 5) {  // m2 += l * l, l the sample's luminance (sample 0 starts it at 0)
                    const float l = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
                    float* m2 = A.fx_col + 3 * (size_t)A.total + k;
                    const float m = s == 0 ? 0.0f : *m2;
                    *m2 = m + l * l;
                }
                if (PM == 2 && A.sp_cur && ((s + 1) % A.sp_chunk == 0 || s + 1 == ns))  // a chunk's end state, for SPEC
                    A.sp_cur[(size_t)(s / A.sp_chunk) * A.total + k] = make_float2(st.x, st.y);
                int s_end = PASS ? A.sp_chunk : ns;
                if (PM == 5) {  // the pixel's own end: its count, unwritten until then, plus the pass's samples
                    const PipeArgs R = reread_args(A);
                    const int k0 = R.sample ? (reinterpret_cast<const int*>(R.fx_col) + 4 * (size_t)R.total)[k] : 0;
                    s_end = min(k0 + R.sp_nch, ns);
                }
                if (++s < s_end) {
                    b = 0;
                    c = ort::mk(1.0f, 1.0f, 1.0f);
                    importance = 1.0f;
                    ray = ort::primary_ray(A.pp, px, py, s, st);
                } else if (PASS) {  // the pass's last sample: the slot's state and sum, and the picture of s samples
                    A.fx_st[k] = make_float2(st.x, st.y);
                    A.fx_col[k] = col.x;
                    A.fx_col[(size_t)A.total + k] = col.y;
                    A.fx_col[2 * (size_t)A.total + k] = col.z;
                    if (PM == 5) (reinterpret_cast<int*>(A.fx_col) + 4 * (size_t)A.total)[k] = s;
                    const PipeArgs R = reread_args(A);
                    if (R.out) {
                        int cx, cy;
                        (void)slot_coords(A, k, cx, cy);
                        store_pixel(R, cy, cx, py, ort::finish_pixel(col, s));
                    }
                    k = -1;
                } else {
                    int cx, cy;
                    (void)slot_coords(A, k, cx, cy);
                    store_pixel(reread_args(A), cy, cx, py, ort::finish_pixel(col, ns));
                    if (A.pl_w) block_account(A, k, nb);  // its block's cost for the next frame
                    k = -1;
                }
            }
        }
        ORT_CK_MARK(ck_shade);
    }
#if ORT_PIXEL_CLOCK
    {
        const int gw = (int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
        if (A.wclock && lane == 0 && !fixup && 2 * gw + 1 < A.wclock_n) {  // (the fixup launch keeps none)
            A.wclock[2 * gw] = make_ulonglong4(ck_refill, ck_trace, ck_shade, ck_iter);
            A.wclock[2 * gw + 1] = make_ulonglong4(ck_lanes, ck_rt0, __builtin_amdgcn_s_memrealtime(), 1ull);
        }
    }
#endif
#undef ORT_CK_MARK
    // the last workgroup out resets the cursor and the done count for the next launch (and the
    // fixup list's length, read by every wave at its start)
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(A.sync + 2, 1) == (int)gridDim.x - 1) {
            atomicExch(A.sync + 1, 0);
            atomicExch(A.sync + 2, 0);
            if (fixup) {
                if (A.sp_ctl[2]) atomicExch(A.sp_ctl + 1, *A.fx_n);  // speculated: the list = the moved pixels
                atomicExch(A.fx_n, 0);
            }
            // the class counts read this frame become the next frame's write counts
            if (A.pl_rcnt && !SPEC)  // (SPEC frames read the lists, and keep them)
                for (int q = 0; q < kPixelClasses; ++q) atomicExch(A.pl_rcnt + q, 0);
        }
    }
}

// SPEC frames: per slot, the pixel's samples summed in order up to the end of the first chunk
// whose end state differs from last frame's (all of them when none does: every chunk started
// from its true state) -> the final pixel, or an entry of the fixup list (the pixel's next
// sample, its true start state, the sum so far).  Padding rows: zeros.
__global__ void __launch_bounds__(256) ort_sample_resolve(PipeArgs A) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= A.total) return;
    int cx, cy;
    if (!slot_coords(A, k, cx, cy)) return;
    if (tile_row_to_y(A.tm, cy) >= A.pp.H) {
        store_padding(A, cy, cx);
        return;
    }
    const int ns = A.pp.ns;
    if (A.sp_ctl[2] == 0) {  // a fall-back frame: the whole chain from sample 0
        ort_rng st;
        ort::pixel_rng_init(A.pp, A.tm.x0 + cx, tile_row_to_y(A.tm, cy), st);
        const int e = atomicAdd(A.fx_n, 1);
        A.fx_slot[e] = k;
        A.fx_s0[e] = 0;
        A.fx_st[e] = make_float2(st.x, st.y);
        A.fx_col[e] = 0.0f;
        A.fx_col[(size_t)A.total + e] = 0.0f;
        A.fx_col[2 * (size_t)A.total + e] = 0.0f;
        return;
    }
    int bad = A.sp_nch - 1;  // the first chunk whose end state moved (the last: none did)
    for (int c = 0; c < A.sp_nch - 1; ++c) {
        const size_t i = (size_t)c * A.total + k;
        const float2 u = A.sp_cur[i], v = A.sp_prev[i];
        if (__float_as_uint(u.x) != __float_as_uint(v.x) || __float_as_uint(u.y) != __float_as_uint(v.y)) {
            bad = c;
            break;
        }
    }
    const int last = min((bad + 1) * A.sp_chunk, ns) - 1;  // samples 0..last are the chain's
    const size_t plane = (size_t)ns * A.total;
    ort::V3 col = ort::mk(0.0f, 0.0f, 0.0f);
    for (int s = 0; s <= last; ++s) {
        const size_t i = (size_t)s * A.total + k;
        col = ort::add(col, ort::mk(A.sp_col[i], A.sp_col[plane + i], A.sp_col[2 * plane + i]));
    }
    if (last == ns - 1) {
        store_pixel(A, cy, cx, -1, ort::finish_pixel(col, ns));
        return;
    }
    const int e = atomicAdd(A.fx_n, 1);
    A.fx_slot[e] = k;
    A.fx_s0[e] = last + 1;
    A.fx_st[e] = A.sp_cur[(size_t)bad * A.total + k];
    A.fx_col[e] = col.x;
    A.fx_col[(size_t)A.total + e] = col.y;
    A.fx_col[2 * (size_t)A.total + e] = col.z;
}

// The mode of a frame whose states last frame recorded: speculate while at most 1/kSpecMovedMax
// of the pixels moved last frame (sp_ctl[1]), else fall back; a fall-back frame recounts them.
__global__ void ort_sample_decide(int* ctl, long long pixels, long long moved_max) {
    if (threadIdx.x == 0) {
        const int spec = (long long)ctl[1] * moved_max <= pixels;
        ctl[2] = spec;
        if (!spec) ctl[1] = 0;
    }
}

// A frame that ran the pixels' chains whole (recording their chunk end states): the pixels whose
// chunk end states differ from last frame's -- the ones a SPEC frame would have re-traced -- into
// *count (the camera or the scene moved: the next frame then does not speculate).
__global__ void __launch_bounds__(256) ort_sample_moved(PipeArgs A, int* count) {
    if (A.sp_ctl[2] != 0) return;  // a speculating frame: its fixup list counted them
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    bool moved = false;
    int cx, cy;
    if (k < A.total && slot_coords(A, k, cx, cy) && tile_row_to_y(A.tm, cy) < A.pp.H)
        for (int c = 0; c < A.sp_nch - 1 && !moved; ++c) {
            const size_t i = (size_t)c * A.total + k;
            const float2 u = A.sp_cur[i], v = A.sp_prev[i];
            moved = __float_as_uint(u.x) != __float_as_uint(v.x) || __float_as_uint(u.y) != __float_as_uint(v.y);
        }
    const unsigned long long m = __ballot(moved);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
}

__global__ void __launch_bounds__(kBlock) k_interleave_nk(const uint2* node, const uint2* kid, uint4* nk, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint2 a = node[i], b = kid[i];
    nk[i] = make_uint4(a.x, a.y, b.x, b.y);
}

// KScene::leaf16 from node[] and leaf_sph[] (n_ent entries), record by record through
// ort::leaf16_record -- the function the host emulation fills its own array with.
__global__ void __launch_bounds__(kBlock) k_leaf16(const uint2* node, const uint4* leaf_sph, int64_t n_ent, uint4* leaf16, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint2 rec = node[i];
    uint4 sp = make_uint4(0u, 0u, 0u, ort::kLeaf16ListTag);  // (an offset outside leaf_sph[]: the list form)
    if (rec.y == 1u && (int64_t)rec.x < n_ent) sp = leaf_sph[rec.x];
    leaf16[i] = ort::leaf16_record(rec, sp);
}

// KScene::cam_node (defined after every other kernel, at the end of this file, so that each keeps its place)
__global__ void __launch_bounds__(kBlock) k_cam_node(const uint2* node, const uint4* leaf16, uint2* cam, int64_t n);

}  // namespace

// The host half, in the one translation unit (a kernel template is emitted where it is first
// named, so the order of these includes, host_launch.inc's dispatchers above all, is the code
// object's): the context and its state, the scene, the dispatchers, the two render paths.
#include "host_context.inc"
#include "host_scene.inc"
#include "host_launch.inc"
#include "host_frame.inc"
#include "host_pixel_paths.inc"
#include "host_pipeline.inc"

// The test-only host emulation (ort_debug_*): the analysis library only (libort_analysis.so).
#if ORT_ANALYSIS
#include "host_emulation.inc"
#endif

// Ray queries (ort_trace_rays, ort_last_query_ms, ort_debug_query_rays): after the render path, so
// that its kernels keep their places in the code object.
#include "ray_query.inc"
// Progressive frames (ort_accum_*): last, so that the passes' ort_pixel_paths<..., 3> instances and
// the resolve kernel follow every other kernel.
#include "accum.inc"
// Camera queries (ort_trace_camera, ort_debug_camera_query): after ray_query.inc, whose walk and
// buffers they share, and after accum.inc, so that every earlier kernel keeps its place.
#include "camera_query.inc"
// Query modes (ort_trace_rays_ex, ort_debug_query_rays_ex): last, so that every earlier kernel keeps its place.
#include "ray_modes.inc"
// Radiance queries (ort_trace_radiance, ort_debug_radiance_rays): last, so that every earlier kernel keeps its place.
#include "radiance_query.inc"

// the denoiser (ort_denoise): its kernels follow every other kernel in the code object
#include "denoise.inc"
// Accumulations that keep luminance moments (ort_accum_begin_ex, ort_accum_read_moments): the
// ort_pixel_paths<..., 4> instances and the moments resolve kernel, after every earlier kernel.
#include "accum_moments.inc"

// the camera walk's records with repeat masks (build_cam_node): last, so that every earlier kernel keeps its place
namespace {
// KScene::cam_node from node[] and the finished leaf16[], record by record through
// ort::leaf_repeat_masks / ort::cam_record -- the functions the host emulation fills its own array
// with.  A leaf-children node reads its eight children's records only where all eight lie inside the
// arrays (cam_has_masks: co + 8 <= n).
__global__ void __launch_bounds__(kBlock) k_cam_node(const uint2* node, const uint4* leaf16, uint2* cam, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint2 rec = node[i];
    uint32_t ab = 0;
    if (ort::cam_has_masks(rec, n)) {
        uint4 k[8];
        for (int o = 0; o < 8; ++o) k[o] = leaf16[(int64_t)rec.x + o];
        ab = ort::leaf_repeat_masks(k, rec.y & 0xffu);
    }
    cam[i] = ort::cam_record(rec, ab);
}
}  // namespace

// Adaptive accumulations (ORT_ACCUM_ADAPTIVE, ort_accum_render_adaptive, ort_accum_read_counts,
// ort_accum_adaptive_stats): the ort_pixel_paths<..., 5> instances, the counts resolve and the stats
// reduction, after accum_moments.inc and every other kernel.
#include "adaptive.inc"
// Temporal reprojection (ort_history_*, ort_debug_history_update): after denoise.inc, whose helpers it
// shares, and last, so that every earlier kernel keeps its place.
#include "reproject.inc"
