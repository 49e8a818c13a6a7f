// tritri.h — triangle-against-mesh intersection queries on the scene's BVH: pt_query_triangles, pt_query_triangles_any
// (include/acgpt.h states the contract; tests/tritri_ref.py is the NumPy statement of the triangle-triangle test and the brute force).
// Kernels in tritri.hip; they read the render kernels' headers and overlap.h's margin and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "overlap.h"

namespace ptd {

constexpr uint32_t kTrianglesMaxPrims = 8u;      // PT_QUERY_TRIANGLES_MAX

// The walk prunes a child box against the query triangle's bounding box [qlo, qhi] = [fmin3, fmax3] of its vertices, which is exact.
//   fp32 nodes (fmt 0):   entered iff lo_k <= qhi_k and hi_k >= qlo_k on all three axes: compares of stored numbers, no arithmetic
//                         and so no margin.
//   fp16 nodes (fmt 11):  the box goes through overlap.hip's decode as centre c = 0.5 qlo + 0.5 qhi and half extent h = 0.5 qhi - 0.5 qlo,
//                         entered iff the per-axis gap e_k <= h_k + m_k with overlap.h's m_k = scene_scale * kOverlapScene +
//                         (|c_k| + h_k) * kOverlapQuery.  DESIGN.md section 29 derives why section 27's two constants carry over: the
//                         statement's three box conditions compare the very corners the leaf box was built from, so the per-query
//                         part is the rounding of c and h alone, u |c_k| + 2 u h_k, below section 27's 3 u S + 2 u |c_k|.
// scene_term: overlap_scene_term of the scene (overlap.h).

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  tris: n records of three float4 {a0.xyz, - |
// a1.xyz, - | a2.xyz, -}.  prims: n * max_prims words, query-major, or null with max_prims == 0; counts: n words or null; not both
// null.  All DEVICE, tris 16-byte aligned, 1 <= n <= 2^31 - 1, max_prims <= kTrianglesMaxPrims.
hipError_t launch_query_triangles(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, uint32_t max_prims,
                                  uint32_t* prims, uint32_t* counts, hipStream_t stream);
// hit: n bytes, 1 where any scene triangle intersects the query triangle; a lane leaves the walk at its first accepted triangle.
hipError_t launch_query_triangles_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, uint8_t* hit,
                                      hipStream_t stream);
// The counting walk, and per query how many inner nodes it visited and how many triangles it tested (acgpt_test.h pt_debug_triangles_visits).
hipError_t launch_triangles_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, uint32_t* counts,
                                   uint2* visits, hipStream_t stream);

}  // namespace ptd
