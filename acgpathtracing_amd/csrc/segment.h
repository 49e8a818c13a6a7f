// segment.h — closest points between segments and the scene's triangles: pt_query_segments (include/acgpt.h states the contract;
// tests/segment_ref.py is the NumPy statement of the whole record).  Kernels in segment.hip; they read the render kernels' headers and
// nearest.h's constants and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "nearest.h"

namespace ptd {

// The pruning threshold of the walk: a child box is entered iff the lower bound of its squared distance to the segment is at most
//   min(best_d2, r2) * kNearRel + (scene_scale^2 + query_scale^2) * kNearAbs,
// scene_scale = the largest |coordinate| of the scene box (nearest_abs_term, formed on the host), query_scale = the largest
// |coordinate| of the segment's two ends (formed per lane).  DESIGN.md section 30 derives it: the errors that are absolute in the
// scene's coordinates come to 84 * 2^-24 scene_scale, and those that are absolute in the query's coordinates — the rounding of
// p0 + d s, of the midpoint and half extent the bounds use, of the crossing test — to 52 * 2^-24 query_scale; the square of their sum
// is at most twice the sum of their squares, and 257 * 2 * (84^2, 52^2) * 2^-48 = (2^-26.2, 2^-27.6) lie below kNearAbs = 2^-25.
__device__ __forceinline__ float segment_abs_term(float scene_abs_term, float query_scale)
{
    return __builtin_fmaf(query_scale * query_scale, kNearAbs, scene_abs_term);
}

// Bound (b) switched off (the test hook's flag, for tools/segments_timing.py): the three axes contribute 0.
constexpr uint32_t kSegmentNoAxes = 1u;

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  segments: n records of two float4
// {p0, max_radius | p1, ignored}; out: n records of two float4 (pt_segment_hit).  Both DEVICE, 16-byte aligned, n >= 1.  abs_term:
// nearest_abs_term of the scene.
hipError_t launch_query_segments(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* segments, uint32_t n, float4* out,
                                 hipStream_t stream);
// The same walk, and per query how many inner nodes it visited and how many triangles it tested (acgpt_test.h pt_debug_segments_visits).
// flags: kSegmentNoAxes.
hipError_t launch_segments_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* segments, uint32_t n, float4* out,
                                  uint2* visits, uint32_t flags, hipStream_t stream);

}  // namespace ptd
