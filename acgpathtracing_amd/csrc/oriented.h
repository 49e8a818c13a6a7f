// oriented.h — oriented-box overlap queries on the scene's BVH: pt_query_overlap_oriented, pt_query_overlap_oriented_any,
// pt_query_overlap_oriented_lists and pt_pose_boxes (include/acgpt.h states the contract; tests/oriented_ref.py is the NumPy statement
// and the brute force).  Kernels in oriented.hip, the query record OBoxQuery in oriented_device.h; the lists form is lists.hip's fill
// and sort instantiated for that record.  Nothing here is read by an existing kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "overlap.h"      // kOverlapMaxPrims: one limit for both box queries

namespace ptd {

// The record is searchable only if its axes u, v, w (the columns of the 3 x 3 part) are orthonormal to this tolerance: the six numbers
// |dot(a, a) - 1| and |dot(a, b)| are all <= kOBoxOrthoTol.  Part of the statement (include/acgpt.h), so bit-defined.
constexpr float kOBoxOrthoTol = 0x1p-10f;

// The margin of the walk (DESIGN.md section 38 has the derivation in full).  With A the 3 x 3 part, the statement accepts a triangle only
// if, on the local coordinates it computes, the triangle meets the cube |q_j| <= h_j.  Those coordinates differ from the exact A^T (p - c)
// of the vertices the leaf boxes were built from (v0, fl(v0 + e1), fl(v0 + e2)) by at most d = 22 u (S + C), u = 2^-24, S the scene's
// largest |coordinate|, C = max |c_k|: v0 - c rounds by u (S + C) per component, a three-term dot product by 3.02 u |a| |p| with
// |p| <= sqrt 3 (S + C), the edge's by 3.02 u sqrt 3 * 2 S, the sum P0 + E by 1.75 u (S + C), the corner sum by u S per component.
// So some point p of the triangle the tree knows has |a_j . (p - c)| <= h_j + d on every box axis j.  Two families of axes prune:
//   box axes    for a child box of centre b and half extent g that holds p:  |a_j . (b - c)| <= h_j + d + sum_k |A_kj| g_k.  This needs no
//               orthonormality, and it already follows from the three face conditions of the statement.
//   world axes  p - c = A^-T q with |q_j| <= h_j + d.  A^-T = A (A^T A)^-1 and the tolerance bounds every entry of (A^T A)^-1 - I by
//               1.004 * 2^-10, so |A^-T_kj - A_kj| <= 1.75 * 2^-10 and |p_k - c_k| <= H_k + 1.75 * 2^-10 (hx + hy + hz) + 1.75 d,
//               H_k = sum_j |A_kj| h_j: the gap between c and the child box on axis k is at most that.
// The walk's own arithmetic adds: the fp16 decode (7 u S on centre and half extent, as overlap.h), c minus the node space's centre
// (u (S + C)), the projection of b - c (5.3 u (2 S + C)) and of g (11 u S), and relative errors of a few u on H, h and the sums.  All
// absolute terms together stay below 84 u (S + C); they are taken as 128 u (S + C) = 2^-17 (S + C), the relative ones as
// 2^-17 (hx + hy + hz), the orthonormality slack as 2^-9 (hx + hy + hz) on the world axes:
//   m = S * kOBoxScene + (C + hx + hy + hz) * kOBoxQuery;   world: gap_k <= H_k + m + (hx + hy + hz) * kOBoxOrtho;   box: as above with d -> m.
constexpr float kOBoxScene = 0x1p-17f;
constexpr float kOBoxQuery = 0x1p-17f;
constexpr float kOBoxOrtho = 0x1p-9f;
// The nine cross axes cross(world axis, box axis) of the full box-against-box test were built and measured against the six above
//  and are not in the product; their arm of the measurement takes the orthonormality slack as
// (hx + hy + hz) * kOBoxOrthoCross (oriented_device.h).
constexpr float kOBoxOrthoCross = 0x1p-7f;

// scene_lo / scene_hi: the scene box the builder (or the last refit) recorded.  The product is taken in double and rounded up.
float oriented_scene_term(const float scene_lo[3], const float scene_hi[3]);

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  boxes: n records of four float4 {m0 m1 m2 m3 |
// m4 m5 m6 m7 | m8 m9 m10 m11 | hx hy hz -}.  The outputs and their combinations are launch_query_overlap's (overlap.h), word for word.
// scene_term: oriented_scene_term of the scene.
hipError_t launch_query_oriented(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                 uint32_t* prims, uint32_t* counts, hipStream_t stream);
hipError_t launch_query_oriented_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint8_t* hit,
                                     hipStream_t stream);
// The counting walk, and per box how many inner nodes it visited and how many triangles it tested (acgpt_test.h
// pt_debug_overlap_oriented_visits).
// cross: the same walk with the nine cross axes in the admission (pt_debug_overlap_oriented_visits_cross).
hipError_t launch_oriented_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t* counts,
                                  uint2* visits, bool cross, hipStream_t stream);
// The fill and the sort of lists.h for oriented records (defined in lists.hip, beside the two it instantiates already).
hipError_t launch_oriented_lists(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, const uint32_t* offsets,
                                 uint32_t* prims, uint32_t capacity, uint32_t* found, uint32_t* flag, uint32_t phases, hipStream_t stream);

// poses: P records of three float4 (a row-major 3 x 4 matrix each); out: P oriented-box records.  Record p is pose p with its fourth
// column replaced by the posed local centre (cx, cy, cz), then {hx, hy, hz, 0}.  1 <= P <= 2^31 - 1; both DEVICE, 16-byte aligned.
hipError_t launch_pose_boxes(const float4* poses, uint32_t P, float cx, float cy, float cz, float hx, float hy, float hz, float4* out, hipStream_t stream);

}  // namespace ptd
