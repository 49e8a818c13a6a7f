// nearest.h — closest-point queries on the scene's BVH: pt_query_nearest (include/acgpt.h states the contract; tests/nearest_ref.py
// is the NumPy statement of the whole record).  Kernels in nearest.hip; they read the render kernels' headers and change nothing in
// them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// The pruning threshold of the walk: a child box is entered iff the lower bound of its squared distance is at most
//   min(best_d2, r2) * kNearRel + scene_scale^2 * kNearAbs,   scene_scale = the largest |coordinate| of the scene box.
// Both constants are derived in DESIGN.md section 24: with kappa = 2^-8, (a + b)^2 <= (1 + kappa) a^2 + (1 + 1 / kappa) b^2 turns the
// absolute error b <= 2^-17 scene_scale between a box's bound and its triangle's computed distance into a relative factor
// (1 + 2^-8) (1 + 16 * 2^-24) <= 1.004 and the absolute term 257 * 2^-34 (1 + 8 * 2^-24) <= 2^-25.
constexpr float kNearRel = 1.004f;
constexpr float kNearAbs = 0x1p-25f;

// scene_lo / scene_hi: the scene box the builder (or the last refit) recorded.  The product is taken in double and rounded up.
float nearest_abs_term(const float scene_lo[3], const float scene_hi[3]);

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  points: n float4 {x, y, z, max_radius}; out: n
// records of two float4 (pt_nearest).  Both DEVICE, 16-byte aligned, n >= 1.  abs_term: nearest_abs_term of the scene.
hipError_t launch_query_nearest(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, float4* out,
                                hipStream_t stream);
// The same walk, and per query how many inner nodes it visited and how many triangles it tested (acgpt_test.h pt_debug_nearest_visits).
hipError_t launch_nearest_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, float4* out,
                                 uint2* visits, hipStream_t stream);

}  // namespace ptd
