// render_core.h -- per-pixel path of the MI355X kernel (__host__ __device__).
//
// Restates shaders/octree_fragment_shader.glsl for one pixel:
//   main()                    glsl:636-664   -> shade_pixel
//   radiance()                glsl:597-633   -> radiance
//   Material_bsdf/refract/    glsl:508-589   -> bsdf
//     schlick
//   skyColor                  glsl:592-595
//   Camera_getRay             glsl:205-221   -> camera_ray
//   random_in_unit_*/cosine   glsl:104-173
//   Sphere_hit                glsl:224-273   -> sphere_hit_t
//   traverseOctree            glsl:290-481   -> traverse_compact (fast layout) /
//                                               traverse_explicit (reference layout)
//   bruteForceIntersect       glsl:484-498   -> traverse_brute
//
// traverse_compact reproduces the reference's stack DFS exactly but stores it as one
// FRAME per tree level (children offset, parent tmin, and an 8-bit mask of the children
// still to visit, in traversal-order rank), and re-derives every box from per-axis split
// planes (see layout.h).  The reference pushes the surviving children of a node in
// reverse traversal order and always pops the top, so its stack is exactly "for every
// ancestor level, the not-yet-visited surviving siblings in traversal order": popping
// the lowest rank bit of the deepest non-empty frame pops the same node with the same
// tmin.  A hit ends the walk after its leaf (glsl:336), so `closest` is still t_max at
// every push, and the 200-entry cap (glsl:471) cannot bind for depth <= 28 (<= 7d+1
// entries); the compact layout is only used for depth <= ORT_COMPACT_MAX_DEPTH.
#pragma once

#include <stdint.h>

#include "../../include/ort_math.h"


#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORT_FN __host__ __device__ __forceinline__
#else
#define ORT_FN static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define ORT_COMPACT_MAX_DEPTH 10
#define ORT_MAX_STACK 200
#define ORT_INTERNAL_FLAG 0x80000000u
#define ORT_LEAFKIDS_FLAG 0x40000000u  // internal node whose existing children are all leaves
// internal record bits 8-15: which existing (pushable) children are leaves, octant space
#define ORT_LEAFMASK_SHIFT 8
#define ORT_MAXFLOAT 3.402823466e+38f

// The pieces, in dependency order; each relies on the ones before it.
#include "render_base.inc"
#include "render_lds_image.inc"
#include "render_fast_math.inc"
#include "render_walks_exact.inc"
#include "render_fast_records.inc"
#include "render_fast_state.inc"
#include "render_fast_walk.inc"
#include "render_shade.inc"
#include "render_query.inc"
