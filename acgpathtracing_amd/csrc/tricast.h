// tricast.h — translating-triangle casts on the scene's BVH: pt_query_triangle_cast, pt_query_triangle_cast_any and the posed form
// pt_query_poses_cast (include/acgpt.h states the contract; tests/tricast_ref.py is the NumPy statement of the time of impact and
// the whole record).  Kernels in tricast.hip, the pair statement and the walk's policy in tricast_device.h; they read the render
// kernels' headers and the query kernels' shared headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// The two widenings of the walk (DESIGN.md section 37 has the derivation in full).  u = 2^-24, S = the largest |coordinate| of the
// scene box, mQ = the largest |coordinate| of the query triangle, M = S + mQ; cq and hq are the centre and half extent of the query's
// box, per axis.
//
// The box.  The walk clips the line cq + t d against each child box inflated on every axis by
//   hq + R,   R = M * kCastBoxAbs.
// Whatever feature gives a candidate at t, its guard has tied the contact c to both boxes: c lies in the scene triangle's box within
// eps and c - d t in the query's box within eps, where one of the two holds without an eps (features 0..2: c - d t is the query's own
// corner; 3..5: c is the scene triangle's own corner; 6..14: c = A + E (G / det) with G / det in [0, 1], so within 2 u S of the
// scene edge).  eps = 2^-16 (the leaf's largest |coordinate| + mQ) <= 2^-16 (1 + u) M.  c and c - d t are computed: d t rounds once
// (u |d t|, and |d t| <= |c| + mQ + eps <= 2 M), the sum or difference once (2 u M), and the stored w1 = fl(v0 + e1) sits within
// an ulp of S of the vertex the tree's boxes were built from: together under 8 u M = 2^-21 M.  So the exact point cq + t d of the line
// lies in the triangle's box, and with it in every box that holds the triangle, inflated by hq + eps + 2^-21 M.  Taken as
// hq + (2^-16 + 2^-17) M: 2^-17 M is left for that, for the rounding of cq and hq (an ulp of mQ each) and for the slab's own
// arithmetic (cq - centre, the fp16 decode's fma, two products with the 1-ulp reciprocal: under 16 u M = 2^-20 M), a factor 8.
// Feature 15 needs none of it: its three box conditions are exact, so at t = 0 the query's box meets the triangle's.
//
// The far cut.  A child is entered iff its slab interval meets [0, cut],
//   cut = min(tmax, best t) * kCastRelT.
// Unlike the swept sphere's, a candidate's t is the parameter of a point that lies INSIDE the inflated box with the slack above to
// spare, so the cut needs no absolute term: planes moved by the slab's rounding still hold the point, and what is left is the relative
// rounding of the two products per axis and of the cut itself, a few u of t.  The interval is closed, so a triangle with the same t and
// a lower index is still reached.  With d = 0 the reciprocals are +-1e30 (finite_rcp), so a product
// is huge or 0: the slab admits the boxes the query's box meets and, since 1e30 is not infinite, also boxes that miss it by less than
// cut / 1e30 on an axis (under tmax = +inf about 3e8 units).  That only admits more; the leaf decides.
constexpr float kCastBoxAbs = 0x1p-16f + 0x1p-17f;
constexpr float kCastRelT = 1.0f + 0x1p-16f;

// flags of launch_poses_cast (acgpt_test.h pt_debug_query_poses_cast; the product passes 0): poses.h kPoseNoEarly, kPosePoseMajor

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  casts: n records of four float4 {a0.xyz, tmax |
// a1.xyz, . | a2.xyz, . | d.xyz, .}; out: n records of two float4 (pt_triangle_cast_hit).  Both DEVICE, 16-byte aligned,
// 1 <= n <= 2^31 - 1.  scene_scale: scene_max_abs (query_launch.h) of the scene box.
hipError_t launch_query_triangle_cast(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                      hipStream_t stream);
// blocked: n bytes, 1 where some triangle has a time of impact within [0, tmax]; a lane leaves the walk at its first such triangle.
hipError_t launch_query_triangle_cast_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n,
                                          uint8_t* blocked, hipStream_t stream);
// The same walk and records, and per cast how many inner nodes it visited and how many triangles it tested (acgpt_test.h
// pt_debug_triangle_cast_visits).
hipError_t launch_triangle_cast_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                       uint2* visits, hipStream_t stream);

// mesh: T records of three float4 (DEVICE, the context's copy); poses: P records of three float4; motions: P float4 {d.xyz, tmax};
// keys: P 64-bit words of scratch, written here (all ones, then (bits of t) << 32 | mesh triangle by fetch_min); out: P records of two
// float4.  P * T <= 2^31 - 1.  Three steps on the stream: fill, phase 1 (one lane per posed triangle), phase 2 (one lane per pose).
hipError_t launch_poses_cast(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* mesh, uint32_t T, const float4* poses,
                             const float4* motions, uint32_t P, unsigned long long* keys, float4* out, uint32_t flags, hipStream_t stream);

}  // namespace ptd
