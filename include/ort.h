/*
 * ort.h -- C ABI of the MI355X octree ray tracer (libort.so).
 *
 * This is the drop-in boundary that replaces the reference's OpenGL path:
 *
 *   reference (GL, Tiago27Cruz/OctreeRayTracer)                         this ABI
 *   ---------------------------------------------------------------------------------------
 *   Raytracer::initialize -> startGLFW/setupQuad/setupShader         ort_create
 *     (src/raytracer.cpp:32-60, src/main.cpp:60-102)
 *   Raytracer::setupBuffers: 7x glBufferData SSBOs + static uniforms ort_upload_scene /
 *     (src/raytracer.cpp:74-152; SSBO bindings glsl:20-46)             ort_upload_octree
 *   per-frame uniforms view/cameraPosition/cameraZoom + glDrawArrays ort_render
 *     (src/raytracer.cpp:491-499; uniforms glsl:13-18, 48-53)
 *   Raytracer::cleanupBuffers (src/raytracer.cpp:154-162)            ort_destroy
 *   (GL errors never checked; shader errors printed, shader.cpp:52-78) ort_last_error
 *
 * Conventions: every call returns an int status (ORT_OK == 0); no C++ exception crosses
 * the ABI.  The context owns all device memory; host arrays passed in are copied.  One
 * context per device; calls on one context are not thread-safe, different contexts may
 * be driven from different threads.  ort_render is synchronous when stream == NULL and
 * stream-ordered (asynchronous) otherwise.
 *
 * Deliberate deviation: node offsets are int32, not float as in the
 * reference's vec4.w packing (src/raytracer.cpp:98-99), which is exact only below 2^24.
 */
#ifndef ORT_H
#define ORT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORT_OK 0
#define ORT_ERR_INVALID_ARG 1
#define ORT_ERR_HIP 2
#define ORT_ERR_NO_SCENE 3
#define ORT_ERR_OUT_OF_MEMORY 4
#define ORT_ERR_UNSUPPORTED 5
#define ORT_ERR_INTERNAL 6
#define ORT_ERR_TIMEOUT 7     /* a bounded wait expired (ort_group_wait: the message names the slot and the
                                 ranks whose render or band send had not completed) */

typedef struct ort_ctx ort_ctx;

/* The shader's uniforms (glsl:13-18, 48-53).  view is column-major like glm::mat4
 * (view[4*col + row]); model/projection are unused by the reference shader.
 *
 * num_samples must be at least 1: every call that renders (ort_render, ort_render_ex,
 * ort_count_traffic, ort_group_submit[_fmt], ort_group_render[_fmt]) refuses a smaller value with
 * ORT_ERR_INVALID_ARG "num_samples must be at least 1" before anything is allocated or launched,
 * and leaves the output untouched.  (The shader divides the sum of zero samples by zero -- a
 * frame of NaN -- and gives a frame of +0 for a negative count; neither is of use to a caller.)
 * max_depth <= 0 is a frame: radiance() returns (1, 1, 1) without tracing a ray, so every
 * channel of every pixel is 1.0 (255 in ORT_FORMAT_RGBA8), whatever the scene. */
typedef struct ort_params {
    int32_t width, height;      /* iResolution.xy of the FULL frame (src/raytracer.cpp:150) */
    int32_t num_samples;        /* numSamples (src/config.h:20) */
    int32_t max_depth;          /* maxDepth: bounces per path (src/config.h:23, MAXRAYSDEPTH) */
    int32_t use_octree;         /* useOctree: 1 octree traversal, 0 brute force (glsl:500-506) */
    float view[16];             /* view matrix uniform */
    float camera_position[3];   /* cameraPosition uniform */
    float camera_zoom;          /* cameraZoom uniform: vertical field of view in degrees */
} ort_params;

/* Which pixels to render.  Output row j (0-based) is pixel row
 *     y = y0 + (j / band_height) * band_stride + (j % band_height)
 * (band_height <= 0 means one band: y = y0 + j).  Pixel rows are GL rows: y = 0 is the
 * BOTTOM row of the image.  Columns are x0 .. x0+width-1.  Rows with y >= height are
 * written as zeros.  The row limit: y0 >= 0, band_stride >= band_height, and the pixel row of
 * the tile's last row (j = rows - 1, the largest: computed in 64 bits) is at most 2^31 - 1; a
 * tile past it is refused with ORT_ERR_INVALID_ARG before anything is allocated or launched
 * and the output is untouched.  The limit is INT_MAX itself, not INT_MAX - 15: the kernels lay
 * the tile out in 16-row blocks, but every site that turns a slot's row into a pixel row does
 * so only for rows j < rows (slot_coords' bound, or the row loop's).
 * The RNG seed and the camera always use the full-frame resolution,
 * so any tiling produces the same pixels as a full-frame render.
 * A tile of no pixels (width == 0 or rows == 0) is valid: ort_render, ort_render_ex and
 * ort_count_traffic return ORT_OK without launching anything, the output is left untouched
 * (a NULL data pointer is accepted for it; every counter is zero), and the context's per-frame
 * state is as it was. */
typedef struct ort_tile {
    int32_t x0, width;
    int32_t y0, rows;
    int32_t band_height;
    int32_t band_stride;
} ort_tile;

/* Per-scene information after upload. */
typedef struct ort_scene_info {
    int32_t n_spheres;
    int32_t n_nodes;
    int64_t n_indices;
    int32_t layout;            /* ORT_LAYOUT_* actually selected */
    int32_t tree_depth;        /* deepest node level (root = 0) */
    int64_t device_bytes;      /* device memory held for the scene */
} ort_scene_info;

#define ORT_LAYOUT_COMPACT 0   /* 8-byte node records, boxes re-derived from per-axis split planes */
#define ORT_LAYOUT_EXPLICIT 1  /* reference record layout, boxes read from memory */

/* Options (ort_set_option). */
#define ORT_OPT_FORCE_LAYOUT 1     /* -1 auto (default), or ORT_LAYOUT_* */
#define ORT_OPT_EXACT_TRAVERSAL 2  /* 1: disable the sign-specialised fast walk (A/B testing; same pixels) */
#define ORT_OPT_REFILL 3           /* persistent trace: refill a wave when >= value of its 64 lanes idle (16) */
#define ORT_OPT_PERSISTENT 4       /* persistent trace kernel with per-lane ray refill: 0 off, 2 (default)
                                      bounce >= 1 traces only: their incoherent rays gain from
                                      refilling idle lanes (C5 -4.5 %); 1 (every trace) was removed in
                                      round 4 (C5 -19 %): ORT_ERR_UNSUPPORTED */
#define ORT_OPT_SORT_PATHS 6       /* order of the alive paths between bounces (coherence; same pixels):
                                      2 (default) radix-sort the compacted list by direction octant +
                                      origin cell + direction; the list's length stays on the device
                                      (the sort's size is the same bounce's length in the previous
                                      frame of the same shape + 1/64 + 1024, read back asynchronously;
                                      a longer list goes on unsorted): no host wait; 1 sort every
                                      slot's key; 0 slot order */
#define ORT_OPT_XCD_SWIZZLE 8      /* workgroup -> tile order (same pixels): 2 each XCD renders runs of
                                      consecutive raster tiles (about 1/15 of a tile row, a power of
                                      two: 16 at 3840 px); 1: each XCD renders 128x128-pixel
                                      super-tiles; 0: raster order (tile b on XCD b % 8); -1 (default):
                                      0 for one-tile workgroups on tiles of at most 1.5 M pixels (a
                                      C3 1/8 band at one frame in flight -3 %), 2 otherwise */
#define ORT_OPT_KID_SKIP 9         /* 1 (default): a lane skips one-sphere leaf children holding the sphere it
                                      last rejected at a tmin <= theirs (they cannot end the walk; same
                                      pixels, kid_table.h), a node's record and kid entry loaded together
                                      from the interleaved copy; 2: the skip with the record and kid
                                      entry from their own arrays (testing; same pixels); 0: walk them
                                      as the reference does */
#define ORT_OPT_SORT_BOUND 10      /* testing: > 0 forces the size of the list sort (SORT_PATHS 2) to this
                                      bound -- below the list's length the list goes on in append
                                      order (same pixels); 0 (default): the hint described above */
#define ORT_OPT_COST_ORDER 11      /* 1 (default): each workgroup of the camera-ray trace deals its 16x16
                                      pixels to its waves ordered by the walk steps each pixel's ray took
                                      in the previous frame of the same shape (rays of like cost share a
                                      wave; same pixels); 0: the fixed 8x8 block per wave */
#define ORT_OPT_HEAVY_FIRST 12     /* T > 0 (default 64): the sorted bounce lists (SORT_PATHS 2, persistent
                                      trace) order paths by the steps their walk at that bounce took in
                                      the previous frame of the same shape -- >= 4T first, then >= 2T,
                                      >= T, the rest, each class in coherence order -- so the longest
                                      walks start early rather than in the launch's drain tail.  After a
                                      camera move (the steps are stale) the classes come from the rays
                                      themselves instead: the distance to the root box's exit, within
                                      1.2 / 2.7 / 6.8 x its smallest extent.  Same pixels.  0: coherence
                                      order only */
#define ORT_OPT_HEAVY_PRIO 13      /* T > 0 (default 150): a wave of the camera-ray trace (cost order on)
                                      that holds a ray whose walk took >= T steps in the previous frame of
                                      the same shape runs at raised issue priority (s_setprio), so the
                                      frame's longest walks do not set its end -- while the camera stands
                                      still (after a move the steps are stale); 0: off.  Same pixels */
#define ORT_OPT_SPLIT_HEAVY 14     /* T > 0 (1 sample, cost order on): the camera rays whose walk took >= T
                                      steps in the previous frame of the same shape (up to 4096 a frame)
                                      are each walked by 8 lanes that deal the walk's subtrees of level
                                      ORT_OPT_SPLIT_LEVEL round robin (the first hit = the hit of the
                                      lowest such subtree in the walk's order), on a second stream beside
                                      the per-tile kernel: a small tile's frame no longer waits for its
                                      longest walks.  0: off.  -1 (default): T = 200 on tiles of at most
                                      2^21 pixels, off on larger ones (where the second stream costs more
                                      than the tail it cuts).  A caller that keeps several frames in
                                      flight should set 0: the next frames fill the tail (C3 1/8 band at
                                      3 in flight: 0.266 -> 0.227 ms/frame); pipelined groups do.
                                      Same pixels */
#define ORT_OPT_SPLIT_LEVEL 15     /* the level of those subtrees: 0 (default) = tree depth - 5 (at least 1) */
#define ORT_OPT_TILE_PAIRS 16      /* 1: a camera-ray workgroup renders two 16x16 tiles side by side, its 512
                                      pixels dealt to 8 blocks of 64 by last frame's walk steps and each
                                      wave walking a heavy and a light block (a workgroup keeps its LDS
                                      until its slowest wave ends); 0: a tile per workgroup; -1 (default):
                                      pairs on tiles of more than 2^21 pixels, or on any tile when
                                      ORT_OPT_SPLIT_HEAVY is 0 (on small tiles at one frame in flight the
                                      fewer, longer workgroups lengthen the frame's tail).  Same pixels */
#define ORT_OPT_DEBUG_FLAGS 18     /* analysis library only (libort_analysis.so, tools/ab_stream.py): 1 records
                                      no per-launch trace-timing events, 2 scans the heavy list at the start
                                      of each split frame; libort.so: ORT_ERR_UNSUPPORTED */
#define ORT_OPT_LAUNCH_TIMES 19    /* 1 (default): HIP events time every trace launch of a frame
                                      (ort_last_trace_ms, ort_trace_times_ms, ort_frame_trace_times_ms);
                                      0: only the frame's start and end are timed (ort_last_kernel_ms) --
                                      fewer event packets on the stream: a C3 1/8 band at one frame in
                                      flight 0.297 -> 0.291 ms; the per-launch queries then report
                                      no newer launch (ort_last_trace_ms: an error while none was ever
                                      timed).  Same pixels */
#define ORT_OPT_PIXEL_PATHS 20    /* whole-pixel paths: the frame in ONE launch, each lane stepping a pixel's
                                      samples and bounces in turn (the RNG state runs on from one sample to the
                                      next, glsl:640, so a pixel is a sequential chain) and taking the next
                                      pixel when done -- instead of the per-sample, per-bounce pipeline (trace,
                                      shade, list sort launches).  -1 (default): on for frames of more than one
                                      traversal per pixel on brute force, on trees of at most 2^19 nodes,
                                      2^23 with maxDepth 5-7 and 2^24 with maxDepth 8 or more (the
                                      reference's sweeps: launches and sorts dominate, more so the more
                                      bounces; larger trees keep the pipeline's sorted bounce rays); 0 off; 1 on wherever it applies (compact layout or brute
                                      force, maxDepth >= 1, not 1 sample x 1 bounce).  Same pixels */
#define ORT_OPT_PIXEL_LDS_SCENE 21 /* 1 (default): whole-pixel paths on scenes whose node records and leaf
                                      spheres fit 32 KB (depth <= 8) copy them into each workgroup's LDS and
                                      walk them there; 0: from global memory.  Same pixels */
#define ORT_OPT_PIXEL_HEAVY_FIRST 22 /* whole-pixel paths: the frame's 8x8 blocks taken in the order of the
                                      previous frame's cost (bounces per sample, 32 classes, heaviest first)
                                      when that frame had the same shape and scene, so the longest pixel
                                      chains start first and do not trail the frame; tile order otherwise.
                                      -1 (default): on for frames of 2 or more samples; 0 off; 1 on.  Same
                                      pixels (the order changes which lane traces a pixel, not its chain) */
#define ORT_OPT_PIXEL_SPECULATE 23 /* whole-pixel paths, 5+ samples: from the second frame of a shape on,
                                      a pixel's samples are traced as up to 4 chunks (of 4 or more
                                      samples) in parallel, chunk c
                                      starting from the RNG state chunk c-1 ended with in the previous
                                      frame (it only depends on how many draws the paths took); a pixel
                                      whose chunk ends in another state than last frame's has its later
                                      samples re-traced from the true state, and every pixel's samples
                                      are summed in order: same pixels, and a frame no longer waits for
                                      its longest pixel's chain.  -1 (default) and 1: on while the
                                      buffers (12 B per sample and path slot, 16 B per chunk) fit 8 GiB;
                                      0: off */
/* Retired option codes, reserved (ORT_ERR_UNSUPPORTED): options that lost to the defaults in
 * A/B and were removed -- 5 the wave-level packet walk (1.2-1.35x slower),
 * 7 the wave-level block queue (1/8 band 0.83 vs 0.61 ms), 17 longest-first workgroups
 * (C3 -25 %).  ORT_OPT_PERSISTENT value 1 is refused likewise (C5 -19 %). */
#define ORT_OPT_IS_RETIRED(o) ((o) == 5 || (o) == 7 || (o) == 17)

/* Traffic counters (ort_count_traffic), in the REFERENCE layout's terms. */
#define ORT_COUNT_NODES_POPPED 0
#define ORT_COUNT_CHILD_RECORDS 1
#define ORT_COUNT_LEAF_OBJECTS 2
#define ORT_COUNT_ACCEPTED_HITS 3
#define ORT_COUNT_PIXELS 4
#define ORT_COUNT_TRAVERSALS 5
#define ORT_COUNT_N 6

/* ---- device context ---------------------------------------------------------------- */
int ort_create(int device, ort_ctx** out);
int ort_destroy(ort_ctx* ctx);
/* Last error message for ctx (or of the calling thread when ctx == NULL). Never NULL. */
const char* ort_last_error(const ort_ctx* ctx);
int ort_set_option(ort_ctx* ctx, int option, int value);

/* Upload a scene in the reference's packing (src/raytracer.cpp:87-101), SoA:
 *   sphere_center_radius[4*i]  = center.xyz, radius          (SSBO binding 0)
 *   sphere_mat_albedo[4*i]     = float(materialType), albedo (SSBO binding 1)
 *   sphere_fuzz_ri[4*i]        = fuzz, refractionIndex, 0, 0 (SSBO binding 2)
 *   node_min[3*k], node_max[3*k], children_offset[k], objects_offset[k], object_count[k]
 *                                                            (SSBO bindings 3, 4, 5)
 *   object_indices[n_indices]                                (SSBO binding 6)
 * Replaces any previous scene on the context. */
int ort_upload_scene(ort_ctx* ctx,
                     const float* sphere_center_radius, const float* sphere_mat_albedo,
                     const float* sphere_fuzz_ri, int32_t n_spheres,
                     const float* node_min, const float* node_max,
                     const int32_t* children_offset, const int32_t* objects_offset,
                     const int32_t* object_count, int32_t n_nodes,
                     const int32_t* object_indices, int64_t n_indices);

/* Same, taking Octree::flattenedTree.data() directly (36-byte GPUOctreeNode records). */
int ort_upload_octree_nodes(ort_ctx* ctx,
                            const float* sphere_center_radius, const float* sphere_mat_albedo,
                            const float* sphere_fuzz_ri, int32_t n_spheres,
                            const void* gpu_octree_nodes, int32_t n_nodes,
                            const int32_t* object_indices, int64_t n_indices);

int ort_scene_get_info(const ort_ctx* ctx, ort_scene_info* info);

/* Build the octree ON THE GPU and make it ctx's scene: replaces Octree::build + setGPUData
 * (src/octree.cpp:47-95, 189-229, 231-242, 268-312) followed by ort_upload_scene, without the
 * host tree.  Same tree, byte for byte: root box from the sphere bounds, midpoint octants,
 * sphereIntersectsBox distribution, BFS numbering, objectIndices in BFS leaf order
 * (level-synchronous build, octreeraytracer_amd/csrc/gpu_build.hip).  n_spheres == 0 fails
 * with ORT_ERR_INVALID_ARG "Sphere list is empty" like the reference's std::invalid_argument.
 * keep_tree != 0 keeps the reference-layout arrays on the device for ort_scene_export_octree. */
int ort_build_scene(ort_ctx* ctx, const float* sphere_center_radius, const float* sphere_mat_albedo,
                    const float* sphere_fuzz_ri, int32_t n_spheres, int32_t max_depth, int32_t max_spheres_per_node,
                    int32_t keep_tree);
/* Copy the kept GPU-built tree to host arrays (sizes: ort_scene_get_info n_nodes x 3 floats /
 * n_nodes ints / n_indices ints): the Octree::flattenedTree fields and objectIndices. */
int ort_scene_export_octree(ort_ctx* ctx, float* node_min, float* node_max, int32_t* children_offset,
                            int32_t* objects_offset, int32_t* object_count, int32_t* object_indices);
/* Device time of the last ort_build_scene (HIP events; the reference's Octree::buildTime). */
int ort_last_build_ms(const ort_ctx* ctx, float* ms);

/* The context's own HIP stream (created non-blocking by ort_create), for callers that keep
   several frames in flight on several contexts: a frame rendered on each context's stream
   overlaps the tail of the previous frame (bench.py --inflight).  No reference counterpart. */
int ort_get_stream(const ort_ctx* ctx, void** stream);

/* Render the tile; rgb_out receives tile->rows * tile->width RGB float triples, row-major,
 * output row 0 first.  out_is_device != 0: rgb_out is a device pointer on ctx's device.
 * stream: a hipStream_t on ctx's device (stream-ordered, returns at once -- also for
 * multi-sample / multi-bounce frames: no step of the frame waits on the host; the first
 * frame of a new shape may allocate, and hipMalloc/hipFree synchronise the device), or NULL
 * for the context's own stream (then the call returns after the frame is complete).  The HIP
 * null stream has the NULL handle, so passing it also means "synchronous".  Two frames in
 * flight on one context must not overlap: render the next one on the same stream or wait. */
int ort_render(ort_ctx* ctx, const ort_params* params, const ort_tile* tile,
               float* rgb_out, int out_is_device, void* stream);

/* Where and in which form ort_render_ex writes the tile.  The reference's shader writes FragColor
 * into the GL default framebuffer (glsl:658-663), an 8-bit RGBA surface: ORT_FORMAT_RGBA8 is that
 * surface's content, quantised by the kernel itself (each channel: NaN -> 0, clamp to [0, 1],
 * x * 255 + 0.5 in float32, truncated -- the package's image.to_srgb8), 4 bytes per pixel in place
 * of 12. */
#define ORT_FORMAT_RGB32F 0   /* 3 floats per pixel (ort_render's) */
#define ORT_FORMAT_RGBA8  1   /* 4 bytes per pixel: R, G, B, A = 255; each channel to_srgb8's rounding */
#define ORT_PLACE_TILE  0     /* output row j is tile row j, column c is tile column c (ort_render's) */
#define ORT_PLACE_FRAME 1     /* data is a full frame: the pixel (x, y) lands at row y, column x */
typedef struct ort_output {
    void*   data;
    int32_t is_device;        /* != 0: data is a device pointer on ctx's device */
    int32_t format;           /* ORT_FORMAT_* */
    int32_t placement;        /* ORT_PLACE_* */
    int32_t reserved;         /* 0 */
    int64_t row_pitch_bytes;  /* 0: tight (tile width, or frame width with ORT_PLACE_FRAME, x bytes per pixel) */
} ort_output;
/* ort_render with the output described by *output: the pixel of output row R, column C is written
 * at data + R * row_pitch_bytes + C * bytes per pixel; the bytes of a row past its pixels are left
 * untouched.  ORT_PLACE_TILE: (R, C) = (tile row j, tile column), rows with y >= height written as
 * zeros (all four bytes of an RGBA8 pixel, alpha included: a padding row stays recognisable).
 * ORT_PLACE_FRAME: (R, C) = (y, x0 + column) in a frame of params->height rows, rows with
 * y >= height not written at all -- several tiles (a group's bands) land in one frame without an
 * assembly pass; device output only.  ORT_ERR_INVALID_ARG, before anything is launched, for an
 * unknown format or placement, reserved != 0, a row_pitch_bytes that is not a multiple of 4, is
 * below the row's bytes or is 2^31 or more, a data pointer that is not 4-byte aligned, and ORT_PLACE_FRAME with host
 * output.  Host output with a pitch is copied with hipMemcpy2DAsync.  stream: as ort_render.
 * ort_render(ctx, p, t, rgb_out, out_is_device, s) is this call with
 * {rgb_out, out_is_device, ORT_FORMAT_RGB32F, ORT_PLACE_TILE, 0, 0}. */
int ort_render_ex(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, const ort_output* output,
                  void* stream);

/* Duration in milliseconds of the last ort_render's kernels (the whole per-frame pipeline),
 * from HIP events recorded on its stream.  Only valid once that stream has passed the frame. */
int ort_last_kernel_ms(ort_ctx* ctx, float* ms);

/* Duration in milliseconds of the first trace kernel (camera rays + octree walk of bounce
 * 0, sample 0: the dominant kernel) of the last ort_render, from HIP events on its stream. */
int ort_last_trace_ms(ort_ctx* ctx, float* ms);

/* The same for the last n frames (at most 64), oldest first; returns how many were
 * written, or a negative ORT_ERR_* code. */
int ort_trace_times_ms(ort_ctx* ctx, int n, float* ms);

/* Per frame, the summed duration of ALL its trace kernels (every sample and bounce: camera
 * rays and the bounce >= 1 walks; at most the first 16 trace launches of a frame are timed),
 * last n frames (at most 64), oldest first; launches[i] (may be NULL) receives how many
 * launches frame i summed.  Returns how many frames were written, or a negative ORT_ERR_*.
 * Shading, path sorting and the deferred-ray exact walk are not included. */
int ort_frame_trace_times_ms(ort_ctx* ctx, int n, float* ms, int32_t* launches);

/* Run the counting variant of the kernel over the tile and return, summed over all
 * pixels, the reference-layout work counters ORT_COUNT_* (counts[ORT_COUNT_N]). */
int ort_count_traffic(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, uint64_t* counts);

/* ---- ray queries: what does this ray hit, and where? (picking, visibility, probe placement) ----
 * ort_trace_rays walks caller-supplied rays through the uploaded scene and returns, per ray, what
 * the shader's intersectScene(ray, 0.001, MAXFLOAT) finds (glsl:500-506), bit for bit: the walk
 * the pixels are made with.  That walk leaves the tree after the first leaf that holds a hit
 * (SURVEY.md F6), so with use_octree = 1 the sphere reported is the one that is DRAWN along the
 * ray, which is not always the geometrically nearest one; use_octree = 0 (bruteForceIntersect)
 * tests every sphere and reports the nearest, the lowest index among equals.
 *   ray     origin and direction, used as given: nothing is normalised, and t is in units of the
 *           direction's length (Sphere_hit).  Degenerate rays (zero, infinite or NaN components)
 *           terminate and miss.
 *   hit     t and the index of the sphere in the uploaded sphere arrays; a miss is {0.0f, -1}.
 *   normals NULL, or 3 floats per ray: IntersectInfo.normal = ((o + t d) - c) / r in float32,
 *           three zeros for a miss.
 * on_device != 0: rays, hits and normals are device pointers on the context's device; else host
 * pointers, staged through grow-only device buffers the context owns.  stream: as ort_render
 * (NULL: the context's stream and a synchronous call; a handle: stream-ordered, no host wait
 * inside the call -- host pointers always wait for their copies).  ORT_QUERY_SORT walks the rays
 * in the coherence order of the bounce paths (one radix sort of (key, index)); the records stay
 * in input order and hold the same values.  It applies to the octree walk of the compact layout
 * and is accepted and ignored elsewhere.  ORT_OPT_KID_SKIP, ORT_OPT_EXACT_TRAVERSAL and
 * ORT_OPT_REFILL apply as they do to bounce walks (same records under every value).  A query
 * keeps its own buffers and counters: it reads and writes no per-frame render state, so frames
 * before and after it are the frames without it.  (Queries of one context share those buffers among
 * themselves: order them on one stream, or let one finish before the next starts on another.)
 * n_rays == 0: ORT_OK, nothing launched.  ORT_ERR_INVALID_ARG, before anything is launched: NULL
 * q, n_rays < 0 or > 2^30, NULL rays or hits with n_rays > 0, unknown flag bits, reserved != 0,
 * pointers that are not 4-byte aligned.  ORT_ERR_NO_SCENE: no scene, or use_octree = 1 on a
 * scene uploaded without a tree.  Not in scope: queries on an ort_group.  (The nearest hit, any
 * hit and a caller-chosen (t_min, t_max): ort_trace_rays_ex below.  A frame's camera rays:
 * ort_trace_camera.) */
typedef struct ort_ray     { float origin[3]; float direction[3]; } ort_ray;   /* 24 bytes */
typedef struct ort_ray_hit { float t; int32_t sphere; } ort_ray_hit;           /* 8 bytes */
#define ORT_QUERY_SORT 1
typedef struct ort_ray_query {
    const ort_ray* rays;
    int64_t n_rays;
    ort_ray_hit* hits;     /* n_rays records */
    float* normals;        /* NULL, or 3 floats per ray */
    int32_t on_device;     /* != 0: all three pointers are device pointers on ctx's device */
    int32_t use_octree;    /* 1: the octree walk; 0: bruteForceIntersect (as ort_params.use_octree) */
    int32_t flags;         /* 0 or ORT_QUERY_SORT */
    int32_t reserved;      /* 0 */
} ort_ray_query;
int ort_trace_rays(ort_ctx* ctx, const ort_ray_query* q, void* stream);

/* Duration in milliseconds of the last query's kernels -- ort_trace_rays, ort_trace_rays_ex,
 * ort_trace_camera or ort_trace_radiance -- (the sort's included, the host
 * copies not), from HIP events on its stream.  Only valid once that stream has passed the query. */
int ort_last_query_ms(ort_ctx* ctx, float* ms);

/* ---- query modes: the nearest hit and any hit inside a per-ray interval (visibility, shadow and
 * segment tests, probe placement) -------------------------------------------------------------------
 * ort_trace_rays_ex is ort_trace_rays with a mode and an optional interval per ray.  Let c_k be what
 * Sphere_hit(k, ray, t_min, t_max) accepts for sphere k alone (glsl:224-273): its near root if that
 * lies in the open interval (t_min, t_max), else its far root if that one does; the float32
 * operations and their order are the shader's.
 *   ORT_QUERY_DRAWN    ort_trace_rays' record, by the same code path: bit-identical.  Takes no
 *                      t_range: the drawn record is the shader's interval by definition.
 *   ORT_QUERY_NEAREST  t = the minimum of c_k over all spheres, sphere = the lowest k attaining it;
 *                      a miss is {0.0f, -1}.  use_octree = 1 and 0, every layout and every option
 *                      value give the same record: the tree is acceleration only.
 *   ORT_QUERY_ANY      {c_k, k} of some sphere with a hit in the interval -- the first one the walk
 *                      finds; which one is unspecified -- or {0.0f, -1}.  Hit-or-miss is
 *                      deterministic and equals NEAREST's.
 * normals are allowed in both modes; in ANY they belong to the reported sphere.
 *   t_range   NULL: (0.001f, MAXFLOAT) for every ray.  Else 2 floats per ray {t_min, t_max}, a
 *             device pointer iff base.on_device (a host pointer is staged like the rays).  An
 *             interval must satisfy 0 <= t_min < t_max; anything else, NaN included, is a miss
 *             without a walk.  t_max = +inf is taken as MAXFLOAT; t_min == 0 is valid.  t is in
 *             units of the direction's length, as in ort_trace_rays: the segment a -> b is
 *             d = b - a with the interval (eps, 1 - eps).
 * Zero-axis rule (NEAREST and ANY; DRAWN keeps the shader's arithmetic): on an axis where the
 * direction component is +-0 a box constrains the ray only by min <= origin <= max, closed on both
 * sides, and contributes (-inf, +inf) to the box's entry and exit.  The NaN of the shader's
 * inf * 0, which makes its min/max drop a box whose plane the origin lies on exactly, is never
 * formed, so the walk finds what brute force finds on those rays too.
 * Degenerate rays (zero, infinite or NaN components) terminate and miss in every mode.
 * Shared with ort_trace_rays: the stream rules, the staging of host pointers, ort_last_query_ms,
 * the buffers (order queries of one context among themselves) and the isolation from render and
 * accumulation state.  ORT_QUERY_SORT, ORT_OPT_KID_SKIP, ORT_OPT_EXACT_TRAVERSAL and ORT_OPT_REFILL
 * are accepted and give the same records under every value.  n_rays == 0: ORT_OK, nothing
 * launched.  ORT_ERR_INVALID_ARG, before anything is launched and with the outputs untouched:
 * whatever ort_trace_rays refuses, an unknown mode, a non-zero reserved, a t_range that is not
 * 4-byte aligned, a t_range with ORT_QUERY_DRAWN.  ORT_ERR_NO_SCENE as ort_trace_rays.  Not in
 * scope: queries on an ort_group. */
#define ORT_QUERY_DRAWN   0   /* ort_trace_rays' record: intersectScene(ray, 0.001, MAXFLOAT) */
#define ORT_QUERY_NEAREST 1   /* the nearest hit inside the ray's interval */
#define ORT_QUERY_ANY     2   /* is there a hit inside the ray's interval? (first one found) */
typedef struct ort_ray_query_ex {
    ort_ray_query base;       /* rays, n_rays, hits, normals, on_device, use_octree, flags, reserved */
    const float* t_range;     /* NULL, or 2 floats per ray {t_min, t_max}; device pointer iff base.on_device */
    int32_t mode;             /* ORT_QUERY_* */
    int32_t reserved[3];      /* 0 */
} ort_ray_query_ex;
int ort_trace_rays_ex(ort_ctx* ctx, const ort_ray_query_ex* q, void* stream);

/* ---- camera queries: each pixel's camera ray and what it hits (picking under the cursor, id /
 * depth / normal images, guide buffers beside a progressive preview) -----------------------------
 * ort_trace_camera makes, for every pixel of a tile, the camera ray the shader makes for it and
 * walks it as ort_trace_rays walks a caller's ray: the caller restates neither the camera
 * (Camera_initFromViewMatrix, glsl:176-202) nor the pixel's RNG draws, and no ray crosses the bus.
 *   which   ORT_CAMERA_FIRST_SAMPLE: the ray radiance() receives for sample 0 of the pixel --
 *           the RNG seeded with FragCoord / iResolution (glsl:640), the two stratum draws of
 *           stratum (0, 0) of (int)sqrt(params->num_samples) (glsl:647-652), Camera_getRay's two
 *           jitter draws and its lens disk (glsl:205-221), radiance()'s normalize (glsl:602).  With
 *           num_samples = 1 the record is the first intersectScene of the pixel's only path.
 *           ORT_CAMERA_PIXEL_CENTRE: the pinhole ray through the pixel centre -- Camera_getRay at
 *           s = (x + 0.5) / width, t = (y + 0.5) / height with the jitter and the lens offset left
 *           out (origin = the camera's position), normalised twice as the shader does; no RNG
 *           draw, independent of num_samples.
 *   records one per tile pixel: index = output row j x tile->width + column, j -> pixel row y as
 *           ort_render maps it (ort_tile: bands, GL rows, y = 0 at the bottom).  Rows with
 *           y >= height get the miss record {0.0f, -1}, a zero normal and a zero ray.  The RNG
 *           seed and the camera always use the full frame's size: any tiling of a frame gives the
 *           full frame's records.
 *   rays    NULL, or the ray of every tile pixel as it was walked.
 *   hits    NULL, or intersectScene(ray, 0.001, MAXFLOAT) by params->use_octree on the resident
 *           layout: bit-identical to ort_trace_rays over the rays this call writes.  NULL with
 *           rays set is ray generation only: nothing is walked and no scene is needed.
 *   normals NULL, or 3 floats per tile pixel as ort_trace_rays writes them; needs hits.
 * params->max_depth is not read.  on_device, stream, the staging of host pointers and
 * ort_last_query_ms: as ort_trace_rays, whose buffers and events this call shares (order the
 * queries of one context on one stream, or let one finish before the next starts on another); it
 * reads and writes no per-frame render or accumulation state.  ORT_OPT_KID_SKIP,
 * ORT_OPT_EXACT_TRAVERSAL and ORT_OPT_REFILL apply as they do to ort_trace_rays (same records).
 * A tile of no pixels: ORT_OK, nothing launched.  ORT_ERR_INVALID_ARG, before anything is launched
 * and with the outputs untouched: a params or tile ort_render refuses (num_samples < 1 among
 * them), NULL q, unknown which, reserved != 0, rays and hits both NULL, normals without hits,
 * pointers that are not 4-byte aligned, a tile of more than 2^30 pixels.  ORT_ERR_NO_SCENE (with
 * hits): no scene, or use_octree = 1 on a scene uploaded without a tree.  Not in scope: samples
 * other than 0 (their RNG state depends on the earlier paths), queries on an ort_group, a
 * caller-chosen (t_min, t_max). */
#define ORT_CAMERA_FIRST_SAMPLE 0  /* the ray radiance() receives for sample 0 of the pixel */
#define ORT_CAMERA_PIXEL_CENTRE 1  /* pinhole ray through the pixel centre: no RNG draw, no lens offset */
typedef struct ort_camera_query {
    ort_ray*     rays;      /* NULL, or one record per tile pixel: the ray that was walked */
    ort_ray_hit* hits;      /* NULL, or one record per tile pixel */
    float*       normals;   /* NULL, or 3 floats per tile pixel (needs hits) */
    int32_t on_device;      /* != 0: all three are device pointers on ctx's device */
    int32_t which;          /* ORT_CAMERA_* */
    int32_t reserved[2];    /* 0 */
} ort_camera_query;
int ort_trace_camera(ort_ctx* ctx, const ort_params* params, const ort_tile* tile,
                     const ort_camera_query* q, void* stream);

/* ---- radiance queries: what does this ray see? (light and irradiance probes, environment
 * captures, fisheye / orthographic / stereo cameras, baking, re-shading a frame's pixels) --------
 * ort_trace_radiance path-traces caller-supplied rays: per ray the mean of `paths` evaluations of
 * the shader's radiance() (glsl:600-634), each drawing from the RNG state the one before left, in
 * float32 with the shader's operations in the shader's order.  Per ray i:
 *     st = states[i]; col = 0
 *     repeat `paths` times:
 *         ray = rays[i]; with ORT_RADIANCE_NORMALIZE direction = the shader's normalize(direction)
 *         c = the body of radiance() after its normalize (glsl:603-633): at most max_depth bounces,
 *             the `importance < 0.01` break, intersectScene(ray, 0.001, MAXFLOAT) by use_octree,
 *             Material_bsdf drawing from st, the sky colour on a miss
 *         col += c
 *     radiance[i] = col / (float)paths            (paths == 1: col itself)
 *     with ORT_RADIANCE_GAMMA: radiance[i] = pow(radiance[i], 1/2.2) per channel (glsl:659-661)
 *     states_out[i] = st
 * The paths of one ray are one sequential chain through st, exactly as a pixel's samples are;
 * different rays are independent.  A 1-sample frame's pixel is this call with ORT_RADIANCE_GAMMA
 * over the ray ort_trace_camera(ORT_CAMERA_FIRST_SAMPLE) returns and the pixel's seed advanced by
 * the six draws that made that ray.
 *   direction  used as given, as in ort_trace_rays, unless ORT_RADIANCE_NORMALIZE is set: the caller
 *              passes unit directions.  A ray returned by ort_trace_camera is already the ray
 *              radiance() walks: it must not be normalised again.
 *   states     2 floats per ray: the shader's randState, each component in [0, 1).  A state with a
 *              component outside [0, 1), NaN included, is not traced: its radiance is three zeros
 *              and its states_out is the state as given (rand2D's float -> uint conversion is only
 *              defined for states in that range).
 *   states_out NULL, or 2 floats per ray; may be equal to states (it must not overlap it otherwise).
 *   degenerate rays (zero, infinite or NaN components) terminate, as in ort_trace_rays, and get
 *              whatever the shader's arithmetic gives for a miss.
 * Shared with ort_trace_rays: on_device and the stream rules, the staging of host pointers through
 * grow-only buffers the context owns, ort_last_query_ms, the buffers (order the queries of one
 * context among themselves) and the isolation from render and accumulation state.  ORT_QUERY_SORT
 * orders the first walk by the rays' coherence keys on the compact layout and is accepted and
 * ignored on brute force; ORT_OPT_KID_SKIP, ORT_OPT_EXACT_TRAVERSAL and ORT_OPT_PIXEL_LDS_SCENE
 * apply as in accumulation passes.  The records are the same under every value.  n_rays == 0:
 * ORT_OK, nothing launched.  ORT_ERR_INVALID_ARG, before anything is launched and with the outputs
 * untouched: NULL q, n_rays < 0 or > 2^30, NULL rays, states or radiance with n_rays > 0, pointers
 * that are not 4-byte aligned, host states_out overlapping states without being equal to it,
 * max_depth < 1, paths outside 1 .. 65536, unknown flag bits, reserved != 0.  ORT_ERR_UNSUPPORTED:
 * use_octree = 1 on the explicit layout (the whole-pixel walk exists for the compact layout and
 * brute force, as for ort_accum_begin).  ORT_ERR_NO_SCENE as ort_trace_rays.  Not in scope:
 * queries on an ort_group, the explicit layout, a caller-chosen (t_min, t_max). */
#define ORT_RADIANCE_NORMALIZE 2   /* apply radiance()'s normalize (glsl:602) to the direction first */
#define ORT_RADIANCE_GAMMA     4   /* write pow(mean, 1/2.2) per channel (glsl:659-661) instead of the mean */
typedef struct ort_radiance_query {          /* 64 bytes */
    const ort_ray* rays;
    int64_t n_rays;
    const float* states;     /* 2 floats per ray: the shader's randState the ray's first path starts from */
    float*       radiance;   /* 3 floats per ray */
    float*       states_out; /* NULL, or 2 floats per ray: randState after the ray's last path; may be == states */
    int32_t on_device;       /* != 0: all pointers are device pointers on ctx's device */
    int32_t use_octree;      /* 1: the octree walk; 0: bruteForceIntersect */
    int32_t max_depth;       /* >= 1: maxDepth of radiance() */
    int32_t paths;           /* 1 .. 65536 paths per ray */
    int32_t flags;           /* ORT_QUERY_SORT | ORT_RADIANCE_* */
    int32_t reserved;        /* 0 */
} ort_radiance_query;
int ort_trace_radiance(ort_ctx* ctx, const ort_radiance_query* q, void* stream);

/* ---- progressive frames: a frame's samples accumulated over several calls --------------------
 * The loop of an interactive caller (the reference's, src/main.cpp:120-163, with a camera driven
 * by input): a cheap pass while the camera moves, a picture that keeps refining while it rests, a
 * preview long before a many-sample frame is finished, a long frame cut into bounded submissions.
 * An accumulation is an opaque object owned by its context.  It holds, per path slot of its tile,
 * the pixel's RNG state and colour sum (20 bytes): a pixel is one sequential chain through its
 * RNG state (glsl:640) and its samples are summed in order, so a frame accumulated in any number
 * of passes ends bit-identical to ort_render_ex's frame of the same params, tile and output.
 *   target   params->num_samples is the target N, fixed at ort_accum_begin: a sample's stratum is
 *            s % (int)sqrt(N), s / (int)sqrt(N) (glsl:647-652), so sample s exists only relative to N.
 *   begin    allocates the state and traces nothing.
 *   pass     ort_accum_render traces the next min(n_samples, N - done) samples of every pixel of
 *            the tile, each chain continued from its stored state, and stores the new state.
 *   preview  with a non-NULL output the pass writes the picture of the k samples done so far:
 *            pow(sum_k / k, 1/2.2) -- the divisor is the samples done, not N.  Any ort_output that
 *            ort_render_ex takes (both formats, pitch, tile or frame placement; padding rows as
 *            ort_render_ex writes them).  NULL output: accumulate without a picture.  With k == N
 *            the picture is ort_render_ex's frame bit for bit, whatever the split into passes; a
 *            preview at k < N with (int)sqrt(k) == (int)sqrt(N) is bit-identical to ort_render_ex
 *            with num_samples = k (the same chain, strata and divisor); any other preview is the
 *            first k samples of the N-sample chain, which no frame of k samples equals.
 *   finished when done == N before the call nothing is traced, and a non-NULL output receives the
 *            finished frame again, from the stored sums.
 *   no pixels an accumulation of a tile of no pixels (ort_tile) is valid: a pass launches nothing,
 *            leaves its output untouched (NULL data is accepted) and still counts its samples as
 *            done, so the accumulation finishes after N of them like any other.
 *   stream   as ort_render.  The passes of one accumulation are ordered by the caller: one stream,
 *            or a wait between them.
 *   isolation an accumulation keeps its own state, work counters and timing events, and neither
 *            reads nor writes the context's per-frame render state (counter sets, speculation
 *            buffers, heavy-first lists, frame timing): frames, ray queries and other accumulations
 *            between two passes change nothing, in either direction.  Several may be alive on one
 *            context.
 *   options  ORT_OPT_KID_SKIP, ORT_OPT_EXACT_TRAVERSAL and ORT_OPT_PIXEL_LDS_SCENE apply per pass
 *            (same pixels under every value).  Passes always take the whole-pixel kernel, whatever
 *            ORT_OPT_PIXEL_PATHS says; they visit the tile's blocks in tile order.
 *   scene    ort_upload_scene* / ort_build_scene invalidate the context's accumulations:
 *            ort_accum_render then returns ORT_ERR_NO_SCENE ("the scene changed ..."), and
 *            ort_accum_restart makes the accumulation usable again where the new scene allows it.
 * ORT_ERR_INVALID_ARG, before anything is launched and with the state untouched: NULL arguments,
 * n_samples < 1, params or a tile that ort_render refuses (num_samples < 1 included), an output
 * that ort_render_ex refuses, an accumulation of another context, ort_accum_restart with another
 * width, height, num_samples, max_depth or use_octree.  ORT_ERR_UNSUPPORTED at begin (and at a
 * restart on a new scene): use_octree = 1 on the explicit layout, max_depth < 1 -- the
 * whole-pixel kernel exists for the compact layout and brute force.  ORT_ERR_NO_SCENE: no scene.
 * Not in scope: passes through the per-bounce pipeline (faster on the largest trees),
 * speculation inside passes (ORT_OPT_PIXEL_SPECULATE), accumulations on an ort_group. */
typedef struct ort_accum ort_accum;
typedef struct ort_accum_info {
    int32_t samples_done, samples_total;
    int64_t device_bytes;     /* device memory the accumulation holds (state, counters, host-output staging) */
} ort_accum_info;
int ort_accum_begin(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, ort_accum** out);
int ort_accum_render(ort_ctx* ctx, ort_accum* accum, int32_t n_samples, const ort_output* output, void* stream);
/* A new camera (view, position, zoom) for the same shape: samples_done back to 0, nothing allocated. */
int ort_accum_restart(ort_ctx* ctx, ort_accum* accum, const ort_params* params);
int ort_accum_get_info(const ort_accum* accum, ort_accum_info* info);
/* Duration in milliseconds of the last pass's kernels (HIP events on its stream; the copy to a
 * host output not included).  Only valid once that stream has passed the pass. */
int ort_accum_last_pass_ms(ort_ctx* ctx, ort_accum* accum, float* ms);
/* Frees the accumulation (NULL: ORT_OK); ort_destroy frees what is left. */
int ort_accum_free(ort_ctx* ctx, ort_accum* accum);

/* ---- luminance moments of an accumulation: how noisy is each pixel still? ----------------------
 * ort_accum_begin_ex with ORT_ACCUM_MOMENTS begins an accumulation whose passes also keep, per path
 * slot, m2: the sum of the squared luminances of the pixel's samples (24 bytes a slot instead of
 * 20).  flags == 0 is ort_accum_begin exactly (state, device_bytes, kernels); unknown bits:
 * ORT_ERR_INVALID_ARG.  In float32, one operation each, at the end of sample s of a pixel, after
 * col += c (c the sample's radiance):
 *     l = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;   m2 = m2 + l * l
 * m2 starts at 0 with sample 0 (ort_accum_restart resets it with the colour sums).  The pictures a
 * moments accumulation writes are the plain accumulation's bit for bit: the moments only add state.
 * ort_accum_read_moments writes, for every tile pixel with k = samples_done:
 *     mean     = col / (float)k per channel (k == 1: col itself): linear, no gamma -- the division
 *                ort_accum_render's preview makes, so pow(mean, 1/2.2) is that preview bit for bit
 *     L        = (0.2126f * mean.x + 0.7152f * mean.y) + 0.0722f * mean.z;   e2 = m2 / (float)k
 *     variance = max(e2 - L * L, 0) / (float)(k - 1): the variance of the mean's luminance, in linear
 *                units; -1.0f = no estimate: k < 2, or e2 or L is not finite
 * mean works on any accumulation; variance needs ORT_ACCUM_MOMENTS.  Rows with y >= height get
 * mean = 0 and variance = -1.  The tile mapping (index = output row j x tile->width + column),
 * on_device, the stream rules and the staging of host pointers (buffers of the accumulation's own,
 * counted in device_bytes) are ort_accum_render's.  The call traces nothing and neither reads nor
 * writes render, query or other accumulations' state.  A tile of no pixels: ORT_OK, nothing written.
 * ORT_ERR_INVALID_ARG, with the outputs untouched: NULL arguments, mean and variance both NULL,
 * reserved != 0, pointers that are not 4-byte aligned, an accumulation of another context,
 * samples_done == 0, variance on an accumulation without ORT_ACCUM_MOMENTS.  ORT_ERR_NO_SCENE after
 * a scene change, as for a pass.  Not in scope: moments on an ort_group, in ort_render or in the
 * per-bounce pipeline.  (Sample counts driven by the variance: adaptive accumulations, below.) */
#define ORT_ACCUM_MOMENTS 1   /* the passes keep m2, the sum of the samples' squared luminances */
int ort_accum_begin_ex(ort_ctx* ctx, const ort_params* params, const ort_tile* tile, int32_t flags, ort_accum** out);
typedef struct ort_accum_moments {
    float* mean;       /* NULL, or 3 floats per tile pixel, tight, tile row j first: linear, no gamma */
    float* variance;   /* NULL, or 1 float per tile pixel, tight */
    int32_t on_device; /* != 0: both are device pointers on ctx's device */
    int32_t reserved[3]; /* 0 */
} ort_accum_moments;
int ort_accum_read_moments(ort_ctx* ctx, ort_accum* accum, const ort_accum_moments* moments, void* stream);

/* ---- adaptive sampling: passes that skip converged pixels --------------------------------------
 * ort_accum_begin_ex with ORT_ACCUM_ADAPTIVE (it implies ORT_ACCUM_MOMENTS) begins an accumulation
 * that keeps one more plane per path slot: an int32 count of the samples that pixel holds (28 bytes
 * a slot instead of 24).  flags == 0 and flags == ORT_ACCUM_MOMENTS stay what they are: state,
 * device_bytes, kernels.  A pixel's chain depends on the pixel alone, so a pixel that holds k samples
 * holds, bit for bit, the sums, m2 and RNG state of a moments accumulation after k uniform samples;
 * which pixel holds which count depends only on the sequence of the passes' parameters, never on
 * scheduling, options or layout.
 *   decision  once per pixel per pass, at the pass's start, from the pixel's stored state alone; N is
 *             num_samples, k the pixel's count.  k >= N: held.  Otherwise k < min_samples or
 *             threshold == 0: traced.  Otherwise with (mean, variance) as ort_accum_read_moments
 *             writes them for the pixel at k: variance < 0 (no estimate: k < 2, a non-finite sum):
 *             traced; else, in float32, one operation each,
 *                 L   = (0.2126f * mean.x + 0.7152f * mean.y) + 0.0722f * mean.z
 *                 ref = L > luminance_floor ? L : luminance_floor;   tol = threshold * ref
 *             and the pixel is held iff variance <= tol * tol: the standard error of the mean
 *             luminance is within `threshold` of it (of luminance_floor where the pixel is darker).
 *   traced    the pixel runs samples k .. min(k + n_samples, N) - 1 of its chain -- the same RNG
 *             chain, the strata of N, col += c, m2 as a moments pass -- and stores its state, sums
 *             and new count.
 *   held      nothing is traced and the pixel's state is untouched.
 *   preview   with a non-NULL output every pixel of the tile is written, held or traced:
 *             pow(sum / k, 1/2.2) with the pixel's own k, in every ort_output ort_accum_render takes;
 *             padding rows as a pass writes them.
 * On an adaptive accumulation the rest of ort_accum_* reads as follows.  ort_accum_render(n) is
 * ort_accum_render_adaptive with {n, 0, 0.0f, any floor}: driven by it alone the accumulation is a
 * moments accumulation bit for bit (previews, the finished frame, moments).  samples_done is the
 * largest count a pixel can have, min(N, sum of the passes' n_samples), no longer "every pixel has
 * this many": pixels may sit below N when it equals N, so a pass always launches (a tile of no
 * pixels still launches nothing) and the finished frame is never served from the stored sums alone.
 * ort_accum_read_moments uses each pixel's own k for mean and variance.  ort_accum_restart resets
 * the counts with the sums (nothing allocated, launched or waited for: the next pass ignores the
 * stored counts).  Scene changes, isolation, streams, host staging (counted in device_bytes, as is
 * the list of pixels to trace that a pass with a criterion builds: 4 bytes a slot, from the first such pass on),
 * several accumulations at once and the per-pass options (the same counts and state under every
 * value) hold as for any accumulation.
 * ort_accum_read_counts writes the counts: tight int32, one per tile pixel, in ort_accum_read_moments'
 * index order; rows with y >= height get 0.  ort_accum_adaptive_stats is synchronous (a small device
 * reduction and the readback of one record): over the tile pixels inside the frame, their number,
 * the sum and the extremes of their counts, and `pending`, the pixels a pass with *criterion would
 * trace now -- the loop of a camera at rest ends when pending == 0.  With no pixel inside the frame
 * min_count and max_count are 0.  The call takes no stream: it runs on the context's own stream (which
 * does not wait for other streams) and returns when the record is read.  Passes queued on a caller's
 * stream must have finished before it is called -- it would read counts that are still being written
 * and the loop's stop condition would be wrong; passes given no stream have finished when they return.
 * ORT_ERR_INVALID_ARG, before anything is launched and with state and outputs untouched: NULL
 * arguments, an accumulation that is not adaptive (these three calls), n_samples < 1,
 * min_samples < 0, a negative or NaN threshold (+inf is valid: whatever has an estimate is held), a
 * luminance_floor that is not finite and positive, reserved != 0, counts not 4-byte aligned, an output
 * ort_render_ex refuses, an accumulation of another context.  ORT_ERR_NO_SCENE and
 * ORT_ERR_UNSUPPORTED as for ort_accum_begin and ort_accum_render.
 * Known limit: a pixel stopped at k < N has only covered the first k strata of N (glsl:647-652), so
 * its estimate is not the stratified one a k-sample frame would give.  Not in scope: adaptive passes
 * on an ort_group, in ort_render or in the per-bounce pipeline; a decision after every sample
 * inside a pass. */
/* (4, not 2: ort_accum_begin_ex has refused flags == 2 as an unknown bit since ORT_ACCUM_MOMENTS came,
 * and callers written against that build keep that answer.) */
#define ORT_ACCUM_ADAPTIVE 4  /* per-pixel sample counts; implies ORT_ACCUM_MOMENTS */
typedef struct ort_accum_adaptive {      /* 32 bytes */
    int32_t n_samples;        /* >= 1: a traced pixel gets min(n_samples, N - k) more samples in this pass */
    int32_t min_samples;      /* >= 0: a pixel with k < min_samples is always traced */
    float   threshold;        /* >= 0: relative standard error of the mean luminance; 0: never held */
    float   luminance_floor;  /* > 0, finite: the luminance below which the error is taken absolute */
    int32_t reserved[4];      /* 0 */
} ort_accum_adaptive;
int ort_accum_render_adaptive(ort_ctx* ctx, ort_accum* accum, const ort_accum_adaptive* pass, const ort_output* output,
                              void* stream);
int ort_accum_read_counts(ort_ctx* ctx, ort_accum* accum, int32_t* counts, int32_t on_device, void* stream);
/* (A struct tag only: the record shares its name with the call, which C allows for a tag and not
 * for a typedef name.  Write `struct ort_accum_adaptive_stats`, in C and in C++.) */
struct ort_accum_adaptive_stats {        /* 40 bytes */
    int64_t pixels, samples, pending;
    int32_t min_count, max_count;
    int32_t reserved[2];
};
int ort_accum_adaptive_stats(ort_ctx* ctx, ort_accum* accum, const ort_accum_adaptive* criterion,
                             struct ort_accum_adaptive_stats* out);

/* ---- several GPUs, one process --------------------------------------
 * The reference renders on one GL context; a caller of Raytracer::render() reaches the 8-GPU
 * configs through a group: one context per listed device (scene replicated), the frame cut
 * into 16-row bands dealt round-robin (rank r renders bands r, r+N, ...; every rank the same
 * number of rows), ONE exchange -- the bands gathered to devices[0] -- and a de-interleave
 * kernel there.  Pixels equal a single-context render bit for bit (they depend only on the
 * global pixel and the frame size).  Transports:
 *   ORT_GROUP_TRANSPORT_RCCL  ncclSend/ncclRecv fused in one ncclGroupStart/End over
 *                             communicators from ncclCommInitAll (RCCL over xGMI); devices
 *                             must be distinct; RCCL is dlopen'ed (RTLD_LOCAL) on demand.
 *   ORT_GROUP_TRANSPORT_COPY  hipMemcpyPeerAsync (testing; a device may be listed twice).
 * Calls on one group are not thread-safe. */
typedef struct ort_group ort_group;
#define ORT_GROUP_MAX_DEVICES 64
#define ORT_GROUP_MAX_INFLIGHT 4
#define ORT_GROUP_TRANSPORT_RCCL 0
#define ORT_GROUP_TRANSPORT_COPY 1
/* One frame in flight (= ort_group_create_pipelined(..., 1, out)). */
int ort_group_create(const int32_t* devices, int32_t n_devices, int32_t transport, ort_group** out);
/* frames_in_flight (1..ORT_GROUP_MAX_INFLIGHT) frame slots, each with its own context per
 * device (its own scene copy, stream, band tiles and, with RCCL, communicators): frames
 * submitted in turn take the slots in turn, so frame k+1's renders fill the tail of frame k's
 * (a 1/N band tile leaves most of the GPU idle while its last blocks finish).  No reference
 * counterpart: the GL loop renders one frame at a time (src/raytracer.cpp:480-519). */
int ort_group_create_pipelined(const int32_t* devices, int32_t n_devices, int32_t transport,
                               int32_t frames_in_flight, ort_group** out);
int ort_group_destroy(ort_group* group);
/* Last error of the group (or of the calling thread when group == NULL).  Never NULL. */
const char* ort_group_last_error(const ort_group* group);
int ort_group_size(const ort_group* group);
int ort_group_frames_in_flight(const ort_group* group);
/* The context of rank `rank` in frame slot 0 (owned by the group), e.g. for ort_scene_get_info. */
int ort_group_context(ort_group* group, int32_t rank, ort_ctx** ctx);
/* ort_set_option on every context (every slot). */
int ort_group_set_option(ort_group* group, int option, int value);
/* ort_upload_scene / ort_build_scene on every context of every slot (same arguments). */
int ort_group_upload_scene(ort_group* group, const float* sphere_center_radius, const float* sphere_mat_albedo,
                           const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                           const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                           const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices,
                           int64_t n_indices);
int ort_group_build_scene(ort_group* group, const float* sphere_center_radius, const float* sphere_mat_albedo,
                          const float* sphere_fuzz_ri, int32_t n_spheres, int32_t max_depth,
                          int32_t max_spheres_per_node);
/* Enqueue one full frame (width x height RGB floats, row 0 = bottom) into rgb_out -- host
 * memory (pinned for a fully asynchronous copy), or (out_is_device != 0) device memory on
 * devices[0] -- and return at once with its ticket (0, 1, 2, ...).  Every rank's render is
 * enqueued before any of them runs (no host wait inside); the only wait is for the frame that
 * last used this frame's slot, frames_in_flight frames earlier.  The bands are received (and
 * then de-interleaved) on a gather stream of devices[0], each as soon as its rank has rendered
 * it, while rank 0 may still be rendering.  rgb_out must stay untouched until
 * ort_group_wait(ticket) returns.  With the RCCL transport, frames_in_flight > 1 runs several
 * slots' communicators concurrently: not yet measured between distinct devices. */
int ort_group_submit(ort_group* group, const ort_params* params, float* rgb_out, int32_t out_is_device,
                     int64_t* ticket);
/* Wait until frame `ticket` is in rgb_out (gathered, assembled and, for host output, copied).
 * The wait is bounded (ort_group_set_timeout): when it expires the call returns
 * ORT_ERR_TIMEOUT and ort_group_last_error names the frame, its slot and every rank whose
 * render / band send had not completed (or the gather and assembly on devices[0]); the frame
 * stays submitted, so a later ort_group_wait may still see it complete. */
int ort_group_wait(ort_group* group, int64_t ticket);
/* The bound of every wait of the group on a frame (ort_group_wait, ort_group_render, and the
 * wait of ort_group_submit for the frame that last used its slot), in milliseconds: default
 * 120000; 0 = poll once (ORT_ERR_TIMEOUT unless the frame has already completed). */
int ort_group_set_timeout(ort_group* group, int64_t timeout_ms);
/* submit + wait for it and every earlier frame: synchronous. */
int ort_group_render(ort_group* group, const ort_params* params, float* rgb_out, int32_t out_is_device);
/* ort_group_submit / ort_group_render in the given ORT_FORMAT_*: out receives the whole tight
 * frame, width x height pixels of 12 (RGB32F) or 4 (RGBA8) bytes; the ranks render their bands in
 * that format, so the band tiles, the exchange and the de-interleave move a third of the bytes
 * with RGBA8.  ort_group_submit / ort_group_render are these calls with ORT_FORMAT_RGB32F. */
int ort_group_submit_fmt(ort_group* group, const ort_params* params, void* out, int32_t out_is_device,
                         int32_t format, int64_t* ticket);
int ort_group_render_fmt(ort_group* group, const ort_params* params, void* out, int32_t out_is_device,
                         int32_t format);
/* Device time, on devices[0], of the frame the last ort_group_wait / ort_group_render waited
 * for: from its submission on devices[0]'s stream to its assembly (renders, gather,
 * de-interleave; HIP events), taken when that frame completed -- the frame's latency, not its
 * share of a pipelined throughput.  The group keeps the times of the last 64 frames: waiting
 * for an older ticket leaves the time unknown (ORT_ERR_NO_SCENE here). */
int ort_group_last_frame_ms(ort_group* group, float* ms);

/* ---- host scene-build stage (kept reference API, src/raytracer.cpp + src/octree.cpp) -- */

/* Raytracer::generateRandomSpheres (src/raytracer.cpp:254-337) with std::mt19937(seed)
 * in place of std::random_device.  Writes n records to each SoA array (4 floats each). */
int ort_scene_random(int32_t n, uint32_t seed, float* sphere_center_radius,
                     float* sphere_mat_albedo, float* sphere_fuzz_ri);
/* Raytracer::generatePreBuiltSpheres (src/raytracer.cpp:164-252): 83 spheres.
 * Pass NULL arrays to query *n_out only. */
int ort_scene_prebuilt(float* sphere_center_radius, float* sphere_mat_albedo,
                       float* sphere_fuzz_ri, int32_t* n_out);
/* The DEBUG scene (src/raytracer.cpp:342-347): 3 spheres. */
int ort_scene_debug(float* sphere_center_radius, float* sphere_mat_albedo,
                    float* sphere_fuzz_ri, int32_t* n_out);

typedef struct ort_octree ort_octree;
/* Octree(max_depth, max_spheres_per_node).build(spheres) (src/octree.cpp:47-95). */
int ort_octree_build(const float* sphere_center_radius, int32_t n_spheres, int32_t max_depth,
                     int32_t max_spheres_per_node, ort_octree** out);
int ort_octree_sizes(const ort_octree* tree, int64_t* n_nodes, int64_t* n_indices, double* build_seconds);
/* Copy out in SoA form (any pointer may be NULL to skip that array). */
int ort_octree_export(const ort_octree* tree, float* node_min, float* node_max,
                      int32_t* children_offset, int32_t* objects_offset, int32_t* object_count,
                      int32_t* object_indices);
/* Zero-copy views: GPUOctreeNode[n_nodes] (36-byte records) and objectIndices. */
const void* ort_octree_nodes(const ort_octree* tree);
const int32_t* ort_octree_indices(const ort_octree* tree);
void ort_octree_free(ort_octree* tree);

/* Camera(position, world_up, yaw, pitch).GetViewMatrix() (src/opengl/camera.h:45-67,115-126):
 * view_out[16] column-major. */
int ort_camera_view(const float position[3], const float world_up[3], float yaw_deg, float pitch_deg,
                    float view_out[16]);

/* Library version string. */
const char* ort_version(void);

/* ---- guided denoiser for few-sample previews: an edge-avoiding a-trous wavelet filter ------------
 * ort_denoise filters a rows x width RGB32F image with the edge-avoiding a-trous filter of Dammertz
 * et al. 2010, guided by what ort_trace_camera writes for the same pixels: the hit records
 * (t, sphere) and the normals.  It is made for the one-sample picture of a progressive preview
 * (ort_accum_render) while the camera moves: with many samples per pixel the filter blurs more than
 * it removes, unless the colour term is on.  It needs no scene and reads and writes no render,
 * accumulation or query state.
 * The arithmetic, every operation one float32 operation in this order (no contraction).  Iteration
 * i = 0 .. iterations-1 has step s = 2^i, reads the previous iteration's colours cur (the input for
 * i = 0) and writes new ones.  For pixel p the taps are q = p + s (dx, dy), dy = -2 .. 2 outside,
 * dx = -2 .. 2 inside, the centre at its place; taps outside the image are skipped.  With
 * h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *     w = h[dy+2] * h[dx+2]
 *     if p and q are hits (sphere >= 0):
 *         a = clamp01((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z); normal_power times: a = a * a;  w *= a
 *         if sigma_depth > 0: w *= clamp01(1 - |t_p - t_q| * inv_z),  inv_z = 1 / (sigma_depth * (float)s)
 *     if sigma_color > 0: d = cur_p - cur_q; dc = (d.r d.r + d.g d.g) + d.b d.b;
 *         wc = clamp01(1 - dc * inv_c); w *= wc * wc,  inv_c = 1 / (sc * sc), sc = sigma_color * 2^-i
 *     the tap adds nothing (w = 0, and a non-finite cur_q is not multiplied) if exactly one of p and
 *         q is a hit, or ORT_DENOISE_SAME_SPHERE is set and the sphere ids differ, or cur_q has a
 *         non-finite channel
 *     sw += w; sum += w * cur_q per channel, in tap order;  next_p = sum / sw per channel
 * clamp01(x) is x < 0 ? 0 : (x > 1 ? 1 : x).  A pixel whose own cur_p has a non-finite channel is
 * copied through unchanged.  The last iteration's result is the output: as is for
 * ORT_FORMAT_RGB32F, through the render path's quantiser for ORT_FORMAT_RGBA8.
 *   color     the image, row r at color + r * color_pitch_bytes.
 *   hits, normals  rows * width records, tight, as ort_trace_camera writes them for the tile.
 *   output    any ort_output with ORT_PLACE_TILE (the tile is the image): both formats, with or
 *             without a pitch.  output->data == color (in place: RGB32F, the same pitch) is allowed
 *             for every iterations value: the input is read completely before the output is written.
 *   border    a tile denoised alone differs from the same pixels of the whole frame's filter within
 *             2 (2^iterations - 1) pixels of its border: the taps past the border are skipped, not
 *             mirrored.
 * on_device, the stream rules and the staging of host pointers (grow-only buffers the context owns,
 * the denoiser's own, separate from the queries') are ort_trace_rays'.  Denoises of one context
 * share those buffers: the caller orders them among themselves.  width * rows == 0: ORT_OK, nothing
 * launched.  ORT_ERR_INVALID_ARG, before anything is launched and with the output untouched: NULL
 * arguments, negative sizes or more than 2^30 pixels, iterations outside 1 .. 6, normal_power
 * outside 0 .. 7, a negative or NaN sigma, unknown flags, reserved != 0, pointers that are not
 * 4-byte aligned, a color_pitch_bytes that is not 0 or a multiple of 4 of at least 12 * width and
 * below 2^31, ORT_PLACE_FRAME, an output that ort_render_ex refuses, on_device disagreeing with
 * output->is_device.  Variance-guided weights for pictures of several samples: ort_denoise_ex.
 * Not in scope: albedo demodulation, denoising on an ort_group, banded tiles (their rows are not
 * neighbours in the frame).  Temporal reprojection: ort_history_update. */
#define ORT_DENOISE_SAME_SPHERE 1   /* a tap of another sphere id (a miss among them) adds nothing */
typedef struct ort_denoise_desc {
    const float*       color;             /* RGB32F, row r at color + r * color_pitch_bytes */
    int64_t            color_pitch_bytes; /* 0: tight (12 * width); else a multiple of 4, >= 12 * width, < 2^31 */
    const ort_ray_hit* hits;              /* rows * width records, tight (ort_trace_camera's) */
    const float*       normals;           /* 3 floats per pixel, tight */
    int32_t width, rows;
    int32_t on_device;                    /* color, hits, normals are device pointers; output->is_device must agree */
    int32_t iterations;                   /* 1 .. 6 */
    float   sigma_color, sigma_depth;     /* 0: term off */
    int32_t normal_power;                 /* 0 .. 7 */
    int32_t flags;                        /* 0 or ORT_DENOISE_SAME_SPHERE */
    int32_t reserved[2];                  /* 0 */
} ort_denoise_desc;
int ort_denoise(ort_ctx* ctx, const ort_denoise_desc* d, const ort_output* output, void* stream);
/* Duration in milliseconds of the last ort_denoise's kernels (the pack pass and the iterations; the
 * host copies not), from HIP events on its stream.  Only valid once that stream has passed it.
 * ORT_ERR_INVALID_ARG: NULL arguments, or no ort_denoise has launched anything on ctx yet. */
int ort_last_denoise_ms(ort_ctx* ctx, float* ms);

/* ---- variance-guided denoising: the filter for a picture that refines while the camera rests ---
 * ort_denoise_ex is ort_denoise with two optional additions: an SVGF-style edge-stopping term driven
 * by a per-pixel variance of the luminance (ort_accum_read_moments'), propagated through the
 * iterations, and a gamma on the output, so that the filter runs on linear radiance -- where the
 * variance lives -- and still writes the display picture.  With variance == NULL and no
 * ORT_DENOISE_GAMMA the call is ort_denoise bit for bit.  The term closes itself as the picture
 * converges: one setting serves 2 and 64 samples per pixel.
 * The arithmetic, float32, one operation each, in this order.  valid(x): x is finite and x >= 0.
 * lum(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b.
 *   prefilter (once, with the pack pass): for a pixel p with valid(v_p), var_p is the 3 x 3 binomial
 *     mean of the valid in-image neighbours: k = k3[dy+1] * k3[dx+1], k3 = (1/4, 1/2, 1/4), dy = -1 .. 1
 *     outside, dx = -1 .. 1 inside; ws += k; vs += k * v_q in that order; var_p = vs / ws.  Without a
 *     valid v_p, var_p = v_p (no estimate).
 *   iteration i, pixel p, tap q, after ort_denoise's terms and not for the taps that add nothing:
 *     if valid(var_p): inv_v = 1 / ((sigma_variance * sigma_variance) * var_p + 1e-12f), once per pixel;
 *         dl = lum(cur_p) - lum(cur_q);  wv = clamp01(1 - (dl * dl) * inv_v);  w = w * wv
 *         sv += (w * w) * (valid(var_q) ? var_q : 0), in tap order, beside sw and sum
 *     next_var_p = sv / (sw * sw) if valid(var_p), else var_p; a pixel copied through because its
 *     colour is not finite keeps var_p.  Every iteration reads the previous iteration's variances.
 *   A tap more than sigma_variance standard deviations away in luminance adds nothing; a converged
 *   pixel (var_p == 0) only takes taps of its own luminance; without a valid var_p the term is off
 *   for that pixel.
 *   ORT_DENOISE_GAMMA: the last iteration's result, pixels copied through included, goes through
 *     pow(x, 1/2.2) per channel (the render path's, glsl:659-661) before the RGB32F store or
 *     ORT_FORMAT_RGBA8's quantiser.
 * variance is rows * width floats, tight, a device pointer iff base.on_device; host pointers are
 * staged through the denoiser's own grow-only buffers.  ORT_ERR_INVALID_ARG, output untouched:
 * whatever ort_denoise refuses (base.flags may carry ORT_DENOISE_GAMMA here; ort_denoise still
 * refuses it), variance with sigma_variance <= 0 or NaN, sigma_variance != 0 without variance, a
 * variance that is not 4-byte aligned, reserved != 0.  ort_last_denoise_ms covers this call too.
 * Not in scope: albedo demodulation, denoising on an ort_group.  (Temporal reprojection, which
 * gives a moving camera's picture a variance to pass here: ort_history_update.) */
#define ORT_DENOISE_GAMMA 2   /* the output is pow(result, 1/2.2) per channel, then the format */
typedef struct ort_denoise_desc_ex {
    ort_denoise_desc base;     /* base.flags may carry ORT_DENOISE_GAMMA here */
    const float* variance;     /* NULL: term off.  Else rows * width floats, tight; device pointer iff base.on_device */
    float sigma_variance;      /* > 0 with variance, 0 without */
    int32_t reserved[3];       /* 0 */
} ort_denoise_desc_ex;
int ort_denoise_ex(ort_ctx* ctx, const ort_denoise_desc_ex* d, const ort_output* output, void* stream);

/* ---- temporal reprojection: a preview's history carried across camera moves ----------------------
 * An ort_history keeps, per pixel of a width x rows tile, an integrated linear colour, its history
 * length and two integrated luminance moments.  ort_history_update takes the new frame's linear
 * one-sample (or few-sample) picture with the pixel-centre rays and hit records of the same pixels
 * (ort_trace_camera, ORT_CAMERA_PIXEL_CENTRE), finds for every pixel where its surface point was in
 * the previous update's frame, fetches that history where it is the same sphere, blends the new
 * sample in and writes the integrated colour, a variance of its luminance (ort_accum_read_moments'
 * convention: -1.0f = no estimate) and the history length: SVGF's temporal stage (Schied et al.
 * 2017).  ort_denoise_ex takes the colour and the variance as they are.  The history is owned by
 * its context and opaque: two ping-pong sets of two 16-byte records per pixel, {r, g, b, n} and
 * {m1, m2, t, sphere}, 64 bytes per pixel, allocated by ort_history_begin (which launches nothing);
 * beside them the previous update's ort_params and tile origin and whether there is a previous
 * frame.  ort_upload_scene, ort_upload_octree_nodes and ort_build_scene make every history of the
 * context forget its previous frame (sphere ids mean something else); that is no error.  Several
 * histories may live on one context; an update reads and writes no render, accumulation, query or
 * denoise state, and needs no scene.
 * The arithmetic, every operation one float32 operation in this order (no contraction).  The pixel is
 * column c, tile row j: frame pixel (x, y) = (tile->x0 + c, tile->y0 + j), record index p = j * width
 * + c.  Primed names belong to the previous update: the camera frame O', LL', hor', ver', w' (origin,
 * lower left corner, horizontal, vertical, w of Camera_initFromViewMatrix, glsl:176-202, for its
 * params), its frame size W', H' and tile origin x0', y0'.  lum is ort_denoise_ex's.
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.  finite(v): neither NaN nor infinite.
 *   1 row past the frame (y >= height): the records are {0, 0, 0, 0} and {0, 0, 0, sphere -1}; the
 *     outputs colour 0, variance -1, length 0; no input is read.
 *   2 sample: s = color[p], l = lum(s), (t, id) = hits[p], (o, d) = rays[p].
 *   3 the history of the pixel: prev_X for X in r, g, b, m1, m2, n -- or none.
 *     no previous frame (the first update, after ort_history_reset or a scene upload): none.
 *     same camera -- width, height, view, camera_position, camera_zoom of params and the tile's x0, y0
 *       are bitwise those of the previous update: the pixel's own previous record q, nothing
 *       projected (a resting camera does not resample its history); none unless n_q > 0 and
 *       sphere_q == id; prev_X = X_q.
 *     otherwise: e = (o + t * d) - O' per component for a hit (id >= 0), e = d for a miss (the sky
 *       is at infinity: only a rotation moves it);  z = -dot(e, w'); none unless z > 0;
 *       k = 10.0f / z;  q = (k * e + O') - LL' per component;
 *       a = dot(q, hor') / dot(hor', hor');  b = dot(q, ver') / dot(ver', ver') (the denominators
 *       made once per call);  fx = (a * (float)W' - 0.5f) - (float)x0';  fy = (b * (float)H' - 0.5f)
 *       - (float)y0';  none unless fx and fy are finite, -1 <= fx < (float)width and -1 <= fy <
 *       (float)rows;  ix = floorf(fx), wx = fx - ix, iy = floorf(fy), wy = fy - iy.
 *       The taps are the previous records at column ix + i, row iy + jj, for (i, jj) = (0, 0), (1, 0),
 *       (0, 1), (1, 1), with w = (i ? wx : 1 - wx) * (jj ? wy : 1 - wy).  A tap counts if it lies in
 *       the tile (0 <= column < width, 0 <= row < rows), n_q > 0, sphere_q == id (-1 matches -1)
 *       and, for a hit with depth_tolerance > 0, fabsf(t_q - dist) <= depth_tolerance * dist with
 *       dist = sqrtf(dot(e, e)).  Over the counting taps in tap order: ws += w; sum_X += w * X_q.
 *       none unless ws >= 0.01f;  prev_X = sum_X / ws.
 *   4 blend, with ok = finite(s.r) and finite(s.g) and finite(s.b):
 *     no history: ok: c = s, m1 = l, m2 = l * l, n = 1;  else c = 0, m1 = m2 = 0, n = 0.
 *     history: n = ok ? prev_n + 1 : prev_n;  a = 1 / n;  if a < alpha: a = alpha;
 *       ok: X = prev_X + a * (new_X - prev_X) for r, g, b, m1 (new value l) and m2 (new value l * l);
 *       else X = prev_X: a sample with a non-finite channel is never blended.
 *   5 the records {c, n} and {m1, m2, t, id} go to the other set;  out_color = c;  out_length = n;
 *     out_variance: with history, ne = 1 / a;  v = m2 - m1 * m1;  if v < 0: v = 0;  r = v / (ne - 1);
 *       the value is r if ne > 1 and r is finite, else -1.0f.  Without history -1.0f.
 * With alpha = 0 and a resting camera this is the running mean of the samples and, as the variance,
 * the variance of that mean which ort_accum_read_moments reports.  alpha > 0 bounds the weight of
 * old samples (an exponential average once 1 / n < alpha).
 *   params    width, height, view, camera_position, camera_zoom are read (num_samples must be >= 1,
 *             as for ort_render).
 *   tile      one band; width and rows are the history's, x0 and y0 may change between updates.
 *   color     this frame's linear RGB32F picture, row j at color + j * color_pitch_bytes
 *             (ort_denoise's pitch rule).
 *   rays, hits  rows * width records, tight, as ort_trace_camera(ORT_CAMERA_PIXEL_CENTRE) writes them
 *             for the tile.
 *   out_color, out_variance, out_length  each NULL or tight: 3, 1 and 1 floats per pixel.  All three
 *             NULL is allowed: the history still advances.
 * on_device: every pointer is a device pointer on ctx's device; otherwise host pointers, staged
 * through grow-only buffers of the history's own (counted in device_bytes).  The stream rules are
 * ort_accum_render's: stream NULL is the context's stream and the call returns when the work is
 * done; with a stream and device pointers the call returns at once; host pointers always wait.
 * Updates of one history are ordered by the caller.  A history of no pixels is valid: its updates
 * launch nothing.  ort_history_reset: the next update has no previous frame (nothing launched).
 * ort_history_get_info: width, rows, the updates since begin, the last reset or the last scene
 * upload, and the device memory held.  ort_history_last_update_ms: the last update's kernel from
 * HIP events on its stream (ORT_ERR_INVALID_ARG before any update launched one).
 * ort_history_free: a NULL history is ORT_OK; ort_destroy frees what is left.
 * ORT_ERR_INVALID_ARG, before anything is launched and with the history and the outputs untouched:
 * NULL arguments, a history of another context, width or rows < 0 or more than 2^30 pixels at
 * begin, a tile whose width or rows are not the history's, a banded tile (band_height > 0 and
 * band_height < rows), params or a tile that ort_render refuses, alpha outside [0, 1] or NaN, a
 * negative or NaN depth_tolerance, flags != 0, reserved != 0, pointers that are not 4-byte aligned,
 * a color_pitch_bytes that ort_denoise refuses, NULL color, rays or hits for a history of pixels.
 * Not in scope: histories on an ort_group, normals in the tap test (a sphere id decides it here),
 * a spatial variance estimate for young pixels (they report -1 and the filter's variance term is off
 * for them).  (Motion of the scene itself: ort_history_update_ex with ORT_HISTORY_MOTION.) */
typedef struct ort_history ort_history;
typedef struct ort_history_frame {
    const ort_params*  params;
    const ort_tile*    tile;
    const float*       color;             /* linear RGB32F, row j at color + j * color_pitch_bytes */
    int64_t            color_pitch_bytes; /* 0: tight (12 * width); else a multiple of 4, >= 12 * width, < 2^31 */
    const ort_ray*     rays;              /* rows * width records, tight (ORT_CAMERA_PIXEL_CENTRE) */
    const ort_ray_hit* hits;              /* rows * width records, tight */
    float*             out_color;         /* NULL, or 3 floats per pixel, tight */
    float*             out_variance;      /* NULL, or 1 float per pixel: -1.0f = no estimate */
    float*             out_length;        /* NULL, or 1 float per pixel: the history length n */
    int32_t on_device;                    /* every pointer above but params and tile is a device pointer */
    float   alpha;                        /* 0 .. 1: the least weight of the new sample */
    float   depth_tolerance;              /* >= 0; 0: no depth test */
    int32_t flags;                        /* 0 */
    int32_t reserved[4];                  /* 0 */
} ort_history_frame;
typedef struct ort_history_info {
    int32_t width, rows;
    int64_t updates;                      /* since begin, the last reset or the last scene upload */
    int64_t device_bytes;
} ort_history_info;
int ort_history_begin(ort_ctx* ctx, int32_t width, int32_t rows, ort_history** out);
int ort_history_update(ort_ctx* ctx, ort_history* history, const ort_history_frame* f, void* stream);
int ort_history_reset(ort_ctx* ctx, ort_history* history);
int ort_history_get_info(const ort_history* history, ort_history_info* info);
int ort_history_last_update_ms(ort_ctx* ctx, ort_history* history, float* ms);
int ort_history_free(ort_ctx* ctx, ort_history* history);

/* ---- temporal reprojection that follows moving spheres ------------------------------------------
 * ort_history_update_ex is ort_history_update with one optional addition, ORT_HISTORY_MOTION in
 * base.flags: the caller vouches that sphere ids keep meaning the same spheres across scene
 * replacements, and a pixel's surface point is moved back with its sphere before it is projected
 * into the previous camera.  Spheres carry no texture and no orientation, so a translation and a
 * uniform scale describe a sphere's motion completely.  With base.flags == 0 the call is
 * ort_history_update bit for bit: records, outputs, state and `updates`.
 * State a history gains, private, allocated by its first MOTION update:
 *   the snapshot: the resident scene's sphere_center_radius (upload index order, the order hit
 *     records use) at the history's last MOTION update, 16 bytes per sphere with the sphere count,
 *     counted in device_bytes (grow-only), copied device to device on the update's stream behind the
 *     kernel;
 *   the stale mark: a scene replacement still leaves the history without a previous frame and with
 *     updates == 0, but remembers that there was a previous frame and the updates value it had,
 *     through several replacements in a row.
 * Any plain update (ort_history_update, or this call with base.flags == 0) drops the snapshot and the
 * stale mark, and so does ort_history_reset; what those calls do is unchanged.
 * A MOTION update needs a resident scene.  It first revives the history -- the previous frame counts
 * as present again and updates goes on from its remembered value -- if the history is stale, has a
 * snapshot and the snapshot's sphere count equals the resident scene's; with another count there is
 * no previous frame (no error).  A history that is not stale and has a previous frame but no snapshot
 * (the update before was a plain one) treats every sphere as unmoved.  The stale mark is dropped.
 * With now[k] the scene's four floats of sphere k, snap[k] the snapshot's and n the sphere count,
 * moved(id) is true when there is a snapshot, 0 <= id < n and at least one of the four floats
 * differs bitwise; an id outside [0, n) reads no sphere and counts as unmoved, as does a miss.
 * ort_history_update's steps change only here:
 *   3 same camera applies only where !moved(id); a moved pixel takes the projected route, the
 *     previous camera being the bitwise same one (a resting camera still follows a moving sphere).
 *   3 otherwise, for a hit with moved(id): P = o + t * d per component;  s = snap[id].w / now[id].w;
 *     P' = snap[id].xyz + s * (P - now[id].xyz) per component (one subtraction, one multiplication,
 *     one addition, no contraction);  e = P' - O';  from z on as there, the depth test included
 *     (dist = sqrtf(dot(e, e)) against the stored t_q).  A non-finite s makes fx non-finite: none.
 *   With !moved(id) the arithmetic is ort_history_update's: the pixels of an unmoved sphere and the
 *   misses are the plain update's bit for bit.
 * Known limits: the light that a moved sphere casts or blocks on OTHER spheres (reflections,
 * occlusion of the sky) lags and is bounded only by alpha; a changed material is not seen at all.
 * ORT_ERR_NO_SCENE, before anything is launched and with the history untouched: ORT_HISTORY_MOTION
 * without a resident scene.  ORT_ERR_INVALID_ARG: whatever ort_history_update refuses (base.flags
 * may carry ORT_HISTORY_MOTION here; ort_history_update still refuses it), unknown bits in
 * base.flags, reserved != 0 in either struct.  ort_history_last_update_ms covers this call's kernel
 * too (the snapshot copy not).  Not in scope: groups, rotation, a motion-vector output. */
#define ORT_HISTORY_MOTION 1   /* hit points are moved back with their sphere before they are projected */
typedef struct ort_history_frame_ex {
    ort_history_frame base;   /* base.flags may carry ORT_HISTORY_MOTION here; ort_history_update still refuses it */
    int32_t reserved[4];      /* 0 */
} ort_history_frame_ex;
int ort_history_update_ex(ort_ctx* ctx, ort_history* history, const ort_history_frame_ex* f, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ORT_H */
