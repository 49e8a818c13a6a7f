// overlap.h — box-overlap queries on the scene's BVH: pt_query_overlap, pt_query_overlap_any (include/acgpt.h states the contract;
// tests/overlap_ref.py is the NumPy statement of the triangle-box test and the brute force).  Kernels in overlap.hip; they read the
// render kernels' headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

constexpr uint32_t kOverlapMaxPrims = 8u;      // PT_QUERY_OVERLAP_MAX

// The margin of the walk: with e the per-axis gap between the query box's centre c and a child box, the child is entered iff
//   e_k <= h_k + m_k  on all three axes,   m_k = scene_scale * kOverlapScene + (|c_k| + h_k) * kOverlapQuery,
// scene_scale = the largest |coordinate| of the scene box.  Both constants are derived in DESIGN.md section 27: the statement's
// p = v0 - c, p + e1, p + e2 and the corner sums the leaf box was built from differ from the exact corners by at most 3 u S + 2 u |c_k|
// (u = 2^-24), the fp16 decode adds 7 u S and a factor 1 + 3 u on the gap, the threshold's own sum rounds by u (h_k + m_k): 10 u S and
// 2 u |c_k| + 4 u h_k at worst, taken as 16 u S and 8 u (|c_k| + h_k).
constexpr float kOverlapScene = 0x1p-20f;
constexpr float kOverlapQuery = 0x1p-21f;

// scene_lo / scene_hi: the scene box the builder (or the last refit) recorded.  The product is taken in double and rounded up.
float overlap_scene_term(const float scene_lo[3], const float scene_hi[3]);

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  boxes: n records of two float4 {cx, cy, cz, hx |
// hy, hz, -, -}.  prims: n * max_prims words, box-major, or null with max_prims == 0; counts: n words or null; not both null.  All
// DEVICE, boxes 16-byte aligned, 1 <= n <= 2^31 - 1, max_prims <= kOverlapMaxPrims.  scene_term: overlap_scene_term of the scene.
hipError_t launch_query_overlap(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                uint32_t* prims, uint32_t* counts, hipStream_t stream);
// hit: n bytes, 1 where any triangle overlaps the box; a lane leaves the walk at its first accepted triangle.
hipError_t launch_query_overlap_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint8_t* hit,
                                    hipStream_t stream);
// The counting walk, and per box how many inner nodes it visited and how many triangles it tested (acgpt_test.h pt_debug_overlap_visits).
hipError_t launch_overlap_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t* counts,
                                 uint2* visits, hipStream_t stream);

}  // namespace ptd
