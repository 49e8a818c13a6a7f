// nearest_k.h — the K closest triangles of a point and the within-radius test: pt_query_nearest_k, pt_query_within_any
// (include/acgpt.h states the contract; tests/nearest_k_ref.py is the NumPy statement of every record, count and byte).  Kernels in
// nearest_k.hip; they read the render kernels' headers and nearest.h's constants and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "nearest.h"

namespace ptd {

// The largest list a lane keeps (PT_QUERY_NEAREST_MAX).
constexpr uint32_t kNearestMaxK = 8u;

// The pruning threshold is nearest.h's, with the d2 it follows exchanged: a child box is entered iff the lower bound of its squared
// distance is at most
//   cut * kNearRel + abs_term,   cut = r2 with counts, min(d2 of entry max_k - 1, r2) without (r2 while that entry is empty).
// DESIGN.md section 24 derives the two constants per triangle — a triangle whose computed d2 is at most the cut lies in boxes whose
// bound is at most cut * kNearRel + abs_term — and nothing in it asks which d2 the cut is (section 31).

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  points: n float4 {x, y, z, max_radius}; out:
// n * max_k records of two float4 (pt_nearest), point-major, null with max_k = 0; counts: n words or null.  All DEVICE, points and
// out 16-byte aligned, n >= 1, max_k <= kNearestMaxK, out and counts not both null.  abs_term: nearest_abs_term of the scene.
hipError_t launch_query_nearest_k(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint32_t max_k,
                                  float4* out, uint32_t* counts, hipStream_t stream);
// hit: n bytes, 1 where the point has a candidate; the lane's walk ends at its first.
hipError_t launch_query_within_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint8_t* hit,
                                   hipStream_t stream);
// The same walks, and per query how many inner nodes it visited and how many triangles it tested (acgpt_test.h
// pt_debug_nearest_k_visits).  mode 0: the list, pruned at entry max_k - 1 unless counts is given; mode 1: the within-radius walk,
// which writes hit and leaves out and counts alone.
hipError_t launch_nearest_k_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint32_t max_k,
                                   float4* out, uint32_t* counts, uint8_t* hit, uint2* visits, uint32_t mode, hipStream_t stream);

}  // namespace ptd
