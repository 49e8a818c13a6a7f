// tridist.h — the distance between query triangles and the scene's triangles: pt_query_triangle_distance (include/acgpt.h states the
// contract; tests/tridist_ref.py is the NumPy statement of the whole record).  Kernels in tridist.hip; they read the render kernels'
// headers, nearest.h's constants and segment.h's absolute term and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "segment.h"

namespace ptd {

// The pruning threshold of the walk is the segment query's: a child box is entered iff the lower bound of its squared distance to the
// query triangle is at most
//   min(best_d2, r2) * kNearRel + (scene_scale^2 + query_scale^2) * kNearAbs,
// query_scale = the largest |coordinate| of the three vertices (segment_abs_term, formed per lane).  DESIGN.md section 33 re-derives
// the constants for the triangle's bounds: the errors that are absolute in the scene's coordinates come to 80 * 2^-24 scene_scale and
// those that are absolute in the query's — now also a closest point on the query triangle and the projections of its vertices onto
// the computed normal — to 83 * 2^-24 query_scale; both stay within the 84 * 2^-24 whose square kNearAbs = 2^-25 already holds.

// Bound (b) switched off (the test hook's flag, for tools/tridist_timing.py): the normal contributes 0.
constexpr uint32_t kTriDistNoPlane = 1u;

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  tris: n records of three float4
// {a0, max_radius | a1, ignored | a2, ignored}; out: n records of three float4 (pt_triangle_distance_hit).  Both DEVICE, 16-byte
// aligned, n >= 1.  abs_term: nearest_abs_term of the scene.
hipError_t launch_query_triangle_distance(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* tris, uint32_t n, float4* out,
                                          hipStream_t stream);
// The same walk, and per query how many inner nodes it visited and how many triangles it tested (acgpt_test.h
// pt_debug_triangle_distance_visits).  flags: kTriDistNoPlane.
hipError_t launch_triangle_distance_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* tris, uint32_t n, float4* out,
                                           uint2* visits, uint32_t flags, hipStream_t stream);

}  // namespace ptd
