// ort_internal.h -- internal declarations shared by the host .cpp files and the .hip file.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/ort.h"

namespace ort {
void set_thread_error(const std::string& msg);
const char* thread_error();
}  // namespace ort

// The ort_debug_* entry points below exist in the analysis library only (Makefile `analysis`,
// -DORT_ANALYSIS=1: octreeraytracer_amd/lib/libort_analysis.so); libort.so exports include/ort.h.
extern "C" {
// TEST-ONLY: run the kernel's per-pixel code (render_core.h, compact or explicit layout)
// on the host CPU, single-threaded, for CPU-side validation of the traversal logic
// against the independent oracle.  Never called by ort_render (which has no CPU path).
int ort_debug_emulate_render(const float* sphere_center_radius, const float* sphere_mat_albedo,
                             const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                             const float* node_max, const int32_t* children_offset,
                             const int32_t* objects_offset, const int32_t* object_count, int32_t n_nodes,
                             const int32_t* object_indices, int64_t n_indices, int32_t layout,
                             const ort_params* params, const ort_tile* tile, float* rgb_out, uint64_t* counts);
// TEST-ONLY: the picture an accumulation shows after samples_done of params->num_samples samples
// (ort_accum_render's preview, stated on the CPU): the first samples_done samples of each pixel's
// num_samples-sample chain -- in num_samples' strata -- divided by samples_done.  samples_done
// 1 .. num_samples; -1 = all of them (ort_debug_emulate_render).
int ort_debug_emulate_render_prefix(const float* sphere_center_radius, const float* sphere_mat_albedo,
                                    const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                                    const float* node_max, const int32_t* children_offset,
                                    const int32_t* objects_offset, const int32_t* object_count, int32_t n_nodes,
                                    const int32_t* object_indices, int64_t n_indices, int32_t layout,
                                    const ort_params* params, const ort_tile* tile, int32_t samples_done,
                                    float* rgb_out, uint64_t* counts);
// TEST-ONLY: the ort_group partition and assembly with an in-memory transport: each of the
// `world` band tiles rendered by ort_debug_emulate_render, then assembled by the device
// kernel's row map (group_map.h).  Full frame into rgb_out (host).
int ort_debug_group_emulate(const float* sphere_center_radius, const float* sphere_mat_albedo,
                            const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                            const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                            const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices,
                            int64_t n_indices, int32_t world, const ort_params* params, float* rgb_out);
// TEST-ONLY: the fast walk's traversal order for direction-sign mask m = (d.z<0)<<2 |
// (d.x<0)<<1 | (d.y<0) (render_core.h rank_perm: order[r] = perm(r) ^ m) and its rank LUT
// rows (rank_lut_entry) for every child mask: lut256[cmask] (checked against the shader's
// tables, tests/golden/traversal_orders.json).
int ort_debug_fast_order(int32_t m, int32_t* order8, uint8_t* lut256);
// TEST-ONLY: the kernels' RGBA8 quantiser (render_core.h pack_rgba8) on the host: out[i] = the
// packed word of the pixel rgb[3 i .. 3 i + 2] (checked against image.to_srgb8).
int ort_debug_pack_rgba8(const float* rgb, int64_t n_pixels, uint32_t* out);
// TEST-ONLY: the split walk (render_core.h traverse_split, the walk of ort_trace_split) of each
// ray run by `lanes` lanes one after another, level-`level` subtrees dealt round robin, merged by
// the lowest DFS position; out[4 i] = {hit entry (-1 none), t bits, position, summed steps}.
int ort_debug_split_rays(const float* sphere_center_radius, int32_t n_spheres, const float* node_min,
                         const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                         const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices,
                         int64_t n_indices, const float* rays, int32_t n_rays, int32_t level, int32_t lanes,
                         int32_t* out);
// TEST-ONLY: per ray (origin.xyz, direction.xyz in rays[6 i]) the fast walk where the kernels
// would take it (fast_prepare) and the exact walk (traverse_compact, literal GLSL min/max);
// out[5 i] = {fast taken, fast entry, fast t bits, exact entry, exact t bits}.  bounce != 0:
// the bounce walk (no inline leaf children, the rejected-sphere skip).
int ort_debug_trace_rays(const float* sphere_center_radius, int32_t n_spheres, const float* node_min,
                         const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                         const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices, int64_t n_indices,
                         const float* rays, int32_t n_rays, int32_t bounce, int32_t* out);
// TEST-ONLY: ort_trace_rays on the host CPU: render_core.h query_ray (the kernels' own per-ray
// function) for every ray (origin.xyz, direction.xyz in rays[6 i]) -- layout ORT_LAYOUT_COMPACT
// or ORT_LAYOUT_EXPLICIT with use_octree 1, brute force with use_octree 0.  hits: n_rays
// records; normals: NULL or 3 floats per ray.
int ort_debug_query_rays(const float* sphere_center_radius, int32_t n_spheres, const float* node_min,
                         const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                         const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices, int64_t n_indices,
                         int32_t layout, int32_t use_octree, const float* rays, int64_t n_rays, ort_ray_hit* hits,
                         float* normals);
// TEST-ONLY: ort_trace_rays_ex on the host CPU: as ort_debug_query_rays, with the mode (ORT_QUERY_*)
// and t_range (NULL, or 2 floats per ray) of ort_ray_query_ex -- render_core.h query_ray_mode, the
// mode kernels' own per-ray function; ORT_QUERY_DRAWN is ort_debug_query_rays itself.
int ort_debug_query_rays_ex(const float* sphere_center_radius, int32_t n_spheres, const float* node_min,
                            const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                            const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices, int64_t n_indices,
                            int32_t layout, int32_t use_octree, const float* rays, int64_t n_rays, int32_t mode,
                            const float* t_range, ort_ray_hit* hits, float* normals);
// TEST-ONLY: ort_trace_camera on the host CPU: the kernels' per-pixel ray (camera_query.inc
// camera_query_ray) for every pixel of the tile, then ort_debug_query_rays over those rays by
// params->use_octree.  rays (6 floats), hits, normals (3 floats) per tile pixel, each may be NULL
// as in ort_camera_query; with hits NULL no scene array is read.
int ort_debug_camera_query(const float* sphere_center_radius, int32_t n_spheres, const float* node_min,
                           const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                           const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices, int64_t n_indices,
                           int32_t layout, const ort_params* params, const ort_tile* tile, int32_t which, float* rays,
                           ort_ray_hit* hits, float* normals);
// TEST-ONLY: ort_trace_radiance on the host CPU: per ray the chain of `paths` paths from its state,
// the kernels' own per-bounce functions (render_core.h trace_ray, hit_record, shade_bounce) in
// shade_pixel's order -- layout ORT_LAYOUT_COMPACT with use_octree 1, brute force with use_octree 0
// (the explicit layout with use_octree 1: ORT_ERR_UNSUPPORTED, as the entry point).  flags:
// ORT_RADIANCE_* (ORT_QUERY_SORT is accepted and changes nothing).  radiance: 3 floats per ray;
// states_out: NULL or 2 floats per ray, may be == states.
int ort_debug_radiance_rays(const float* sphere_center_radius, const float* sphere_mat_albedo,
                            const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                            const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                            const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices,
                            int64_t n_indices, int32_t layout, int32_t use_octree, const float* rays,
                            const float* states, int64_t n_rays, int32_t max_depth, int32_t paths, int32_t flags,
                            float* radiance, float* states_out);
// TEST-ONLY: ort_denoise on the host CPU: the pack pass and every iteration through denoise.inc's
// denoise_pixel, the kernels' own per-pixel function, one pixel after another.  d's pointers and
// output->data are host pointers (d->on_device and output->is_device 0); what ort_denoise refuses
// is refused here, with the output untouched.
int ort_debug_denoise(const ort_denoise_desc* d, const ort_output* output);
// TEST-ONLY: ort_denoise_ex on the host CPU, as ort_debug_denoise: the variance prefilter, the
// iterations through denoise_pixel<true> with the variances propagated, the optional gamma.
int ort_debug_denoise_ex(const ort_denoise_desc_ex* d, const ort_output* output);
// TEST-ONLY: ort_history_update on the host CPU, stateless: one update through reproject.inc's
// reproject_pixel, the kernel's own per-pixel function, one pixel after another.  prev_params (NULL: no
// previous frame), prev_x0, prev_y0: the previous update's params and tile origin; prev_a, prev_b: its
// record planes {r, g, b, n} and {m1, m2, t, sphere}, 4 floats per pixel each (not read without a
// previous frame); f: the frame, host pointers (f->on_device 0), the history's shape being its tile's;
// next_a, next_b receive the next record planes, f's outputs as ort_history_update writes them.  What
// ort_history_update refuses of a frame is refused here, with everything untouched.
int ort_debug_history_update(const ort_params* prev_params, int32_t prev_x0, int32_t prev_y0, const float* prev_a,
                             const float* prev_b, const ort_history_frame* f, float* next_a, float* next_b);
// TEST-ONLY: ort_history_update_ex on the host CPU, stateless, as ort_debug_history_update.  With
// ORT_HISTORY_MOTION in f->base.flags: now is the scene's sphere_center_radius (n_spheres records of 4
// floats, upload order; NULL: ORT_ERR_NO_SCENE) and snap the snapshot's (NULL: none, every sphere counts
// as unmoved), through reproject_pixel<true>; without the flag now, snap and n_spheres are not read
// and the call is ort_debug_history_update.  What ort_history_update_ex refuses of a frame is refused.
int ort_debug_history_update_ex(const ort_params* prev_params, int32_t prev_x0, int32_t prev_y0, const float* prev_a,
                                const float* prev_b, const ort_history_frame_ex* f, const float* now, const float* snap,
                                int32_t n_spheres, float* next_a, float* next_b);
// TEST-ONLY: one transition of what decides whether an update has a previous frame (host_context.inc
// HistoryState, the histories' own): st = {updates, has_prev, stale, the updates a replacement took
// away, has a snapshot, its sphere count}; op 0: the scene is replaced, 1: ort_history_reset, 2: a plain
// update, 3: a MOTION update on a scene of n_spheres (reads_snapshot, if not NULL: whether it reads
// the snapshot; 0 for the other ops).
int ort_debug_history_state(int64_t* st, int32_t op, int32_t n_spheres, int32_t* reads_snapshot);
// TEST-ONLY: finish_pixel(v, 1) -- pow(x, 1/2.2) per channel, ORT_DENOISE_GAMMA's -- of n_pixels RGB
// triples on the host (ort_powf is not restated in numpy; out may be rgb).
int ort_debug_gamma(const float* rgb, int64_t n_pixels, float* out);
// TEST-ONLY: what ort_accum_read_moments returns after samples_done (1 .. num_samples) samples of an
// accumulation of params and tile: ort_debug_emulate_render_prefix's arguments; mean (3 floats per
// tile pixel) and variance (1 float per tile pixel), either may be NULL.
int ort_debug_emulate_moments(const float* sphere_center_radius, const float* sphere_mat_albedo,
                              const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                              const float* node_max, const int32_t* children_offset,
                              const int32_t* objects_offset, const int32_t* object_count, int32_t n_nodes,
                              const int32_t* object_indices, int64_t n_indices, int32_t layout,
                              const ort_params* params, const ort_tile* tile, int32_t samples_done,
                              float* mean, float* variance);
// TEST-ONLY: an adaptive accumulation (ort_accum_render_adaptive) of params and tile driven by the
// n_passes passes of `passes`, on the host CPU: per pixel the shared decision (adaptive.inc's
// adaptive_traces) on shade_pixel's chain at the pixel's count.  ort_debug_emulate_moments' scene
// arguments; counts (1 int per tile pixel), mean and variance as ort_accum_read_counts and
// ort_accum_read_moments write them afterwards, each may be NULL.
int ort_debug_emulate_adaptive(const float* sphere_center_radius, const float* sphere_mat_albedo,
                               const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                               const float* node_max, const int32_t* children_offset,
                               const int32_t* objects_offset, const int32_t* object_count, int32_t n_nodes,
                               const int32_t* object_indices, int64_t n_indices, int32_t layout,
                               const ort_params* params, const ort_tile* tile, const ort_accum_adaptive* passes,
                               int32_t n_passes, int32_t* counts, float* mean, float* variance);
// TEST-ONLY: the shared decision itself for one pixel's stored state: 1 traced, 0 held (k the
// pixel's count, n_total the target N, col the colour sum, m2 the sum of squared luminances), or
// -1 where ort_accum_render_adaptive refuses the criterion.
int ort_debug_adaptive_decision(int32_t k, int32_t n_total, const ort_accum_adaptive* criterion, const float* col, float m2);
// ANALYSIS-ONLY: lane overlap of sampled 8x8 primary-ray blocks (tools/wave_stats.py).
int ort_debug_wave_stats(const float* sphere_center_radius, const float* sphere_mat_albedo,
                         const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                         const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                         const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices,
                         int64_t n_indices, const ort_params* params, int32_t block_step, double* stats,
                         int32_t n_stats);
// ANALYSIS-ONLY: the per-step work of the fast walk (the kernel's own fast_step, inline leaf
// children) for the 64 lanes of sampled 8x8 primary-ray blocks (tools/walk_sim.py).
// lens[64 * w + l] = steps of lane l of sampled wave w (0: not a fast-walk lane); steps[] =
// the lanes' steps back to back, one uint16 each: objects tested (bits 0-7, saturated),
// leaf children tested (bits 8-11), bit 15 = the step's node has leaf children (LEAFKIDS).
// Returns the number of steps (or, if cap is too small, minus the number needed).
int ort_debug_bounce_walks(const float* sphere_center_radius, const float* sphere_mat_albedo,
                           const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min, const float* node_max,
                           const int32_t* children_offset, const int32_t* objects_offset, const int32_t* object_count,
                           int32_t n_nodes, const int32_t* object_indices, int64_t n_indices, const ort_params* params,
                           const ort_tile* tile, int32_t bounce, float* rays, int32_t* walks, int64_t cap,
                           int64_t* n_out);
int64_t ort_debug_walk_steps(const float* sphere_center_radius, const float* sphere_mat_albedo,
                             const float* sphere_fuzz_ri, int32_t n_spheres, const float* node_min,
                             const float* node_max, const int32_t* children_offset, const int32_t* objects_offset,
                             const int32_t* object_count, int32_t n_nodes, const int32_t* object_indices,
                             int64_t n_indices, const ort_params* params, int32_t block_step, int32_t* lens,
                             int64_t n_lens, uint16_t* steps, int64_t cap);
// TEST-ONLY: the image a workgroup copies into LDS for a tree of this depth (render_core.h
// lds_layout: what k_lds_image writes, by the same fill_fast_planes), built on the host from the
// forward plane tables planes[3 (2^depth + 1)].  layout[7] = {image bytes, rank LUT offset,
// plane table bytes, pop table 1 offset (-1: none), pop table 2 offset, entries per pop table,
// Masks64::kPopTable of this build}; image: NULL, or cap_words 32-bit words to receive it.
int ort_debug_lds_image(int32_t depth, const float* planes, uint32_t* image, int64_t cap_words, int32_t* layout);
// TEST-ONLY: how often the host's depth <= 8 camera walks (fast_pop, inline leaf children) popped
// mask bit hb = 8 L + 7 - rank (hb_pops[64]) and under which direction-sign mask m
// (sign_masks[8], counted per pop) since the last reset; reset != 0 clears the counts.
int ort_debug_pop_coverage(uint64_t* hb_pops, uint64_t* sign_masks, int32_t reset);
// TEST-ONLY: the compact layout of a tree as the host emulation walks it: node[] (2 words a node),
// leaf_sph[] (4 words an entry) and the 16-byte leaf records derived from them (render_core.h
// leaf16_record; 4 words a node, none for a tree deeper than 8 or a build without
// Masks64::kLeafInline), each copied when its pointer is given.  sizes[3] = {nodes, entries,
// leaf records}: call once with null arrays for the sizes.
int ort_debug_leaf16(const float* sphere_center_radius, int32_t n_spheres, const float* node_min, const float* node_max,
                     const int32_t* children_offset, const int32_t* objects_offset, const int32_t* object_count,
                     int32_t n_nodes, const int32_t* object_indices, int64_t n_indices, uint32_t* node,
                     uint32_t* leaf_sph, uint32_t* leaf16, int64_t* sizes);
// TEST-ONLY: a context's device leaf records (k_leaf16) copied to out[4 cap]; *n = their number.
int ort_debug_ctx_leaf16(ort_ctx* ctx, uint32_t* out, int64_t cap, int64_t* n);
// TEST-ONLY: ort_debug_lds_image with the choice of tables explicit: rev_tables != 0 gives the
// reversed-table image a depth 9-10 scene keeps beside the default one (lds_rev).
int ort_debug_lds_image_rev(int32_t depth, const float* planes, int32_t rev_tables, uint32_t* image, int64_t cap_words,
                            int32_t* layout);
// TEST-ONLY: one array of the compact layout the host emulation builds for a tree, by name: "node",
// "kid", "leaf_sph", "leaf_idx", "planes", "leaf16", "cam_node" (none for a tree deeper than 8), or the scalars
// "depth" and "ordered" (one int32 each).  *bytes = its size; copied to out when given (cap_bytes).
int ort_debug_layout(const float* sphere_center_radius, int32_t n_spheres, const float* node_min, const float* node_max,
                     const int32_t* children_offset, const int32_t* objects_offset, const int32_t* object_count,
                     int32_t n_nodes, const int32_t* object_indices, int64_t n_indices, const char* name, void* out,
                     int64_t cap_bytes, int64_t* bytes);
// TEST-ONLY: one device array of a context's scene, by name, copied to out after the context's stream
// has drained: those of ort_debug_layout, "nk", "lds_img", "lds_rev" (0 bytes where the scene has
// none), or the scalars "depth", "ordered", "layout" (one int32 each).  *bytes = its size.
int ort_debug_ctx_array(ort_ctx* ctx, const char* name, void* out, int64_t cap_bytes, int64_t* bytes);
// TEST-ONLY: sphere tests and accepted hits of the host's depth <= 8 camera walks per leaf record
// form since the last reset: {inline tests, inline hits, list tests, list hits}.
int ort_debug_leaf_forms(uint64_t* out4, int32_t reset);
// TEST-ONLY: the leaf children of the non-counting host camera walks (depth <= 8) since the last
// reset: {tested (trips of leaf_kids), dropped untested by a repeat mask (Masks64::kLeafDedup) on a
// trip that did not hit, the build's Masks64::kLeafDedup}.
int ort_debug_leaf_dedup(uint64_t* out3, int32_t reset);
// TEST-ONLY: the depth <= 8 camera walk's two child tests on the host: render_core.h child_drops (eight
// min3/max3 tests) and child_order_keep (twelve order bits and the two order tables of
// render_lds_image.inc), both as kept ranks in the reversed layout (rank 0 at bit 7).
//   mode 0: in[10 i] = {tNA, tNB, tMA, tMB, tFA, tFB, nN, nF, cN, cF} for n cases;
//           out[2 i] = child_drops' keep bits, out[2 i + 1] = child_order_keep's.
//   mode 1: a native sweep: in = an ascending grid of n values; per axis every tN <= tM <= tF from it (ties
//           included), the three axes crossed with every t_min of tmins[n_tmin] and every closest of
//           closests[n_closest], folded into the C axis as fast_visit folds them.  out[4] = {cases with
//           X >= E, of them the two forms disagree, cases with X < E, of them child_drops keeps a child}.
//   mode 2: the internal-node visits of the host's order-bit walks since the last reset (n != 0 resets):
//           out[6] = {visits, those breaking tN <= tM <= tF (A, B) or nN <= nF or cN <= cF, those below the
//           root with X < E, those where the two forms keep different children, internal roots whose
//           premise X >= E failed under the folds (fast_begin clears their child mask),
//           Masks64::kOrderBits}.
//   mode 3: out[128] = the host's order tables, table 0 then table 1; mode 4: the device's (g_order_tables, read by a kernel on
//           the current device).
int ort_debug_child_order(int32_t mode, const float* in, int64_t n, const float* tmins, int32_t n_tmin,
                          const float* closests, int32_t n_closest, uint64_t* out);
// ANALYSIS-ONLY: ort_debug_walk_steps with production != 0: the non-counting walk's step records
// (leaf children tested after the build's repeat masks, sphere tests) instead of the counting walk's.
int64_t ort_debug_walk_steps_ex(const float* sphere_center_radius, const float* sphere_mat_albedo, const float* sphere_fuzz_ri,
                                int32_t n_spheres, const float* node_min, const float* node_max, const int32_t* children_offset,
                                const int32_t* objects_offset, const int32_t* object_count, int32_t n_nodes,
                                const int32_t* object_indices, int64_t n_indices, const ort_params* p, int32_t block_step,
                                int32_t production, int32_t* lens, int64_t n_lens, uint16_t* steps, int64_t cap);
}
