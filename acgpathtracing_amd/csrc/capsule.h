// capsule.h — swept-capsule casts on the scene's BVH: pt_query_capsule_cast, pt_query_capsule_cast_any (include/acgpt.h states the
// contract; tests/capsule_ref.py is the NumPy statement of the time of impact and the whole record).  Kernels in capsule.hip; they
// read the render kernels' headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// The widenings of the walk, derived as sweep.h derives the sphere's.  u = 2^-24, S = the largest |coordinate|
// of the scene box, per cast M = S + the largest |coordinate| of p0 and p1, which bounds every component of every m = p - P the leaf
// test forms, a = p1 - p0 (every component at most 2 M) and |d| = sqrt(dd).  At the time t the leaf accepts, the capsule's axis
// {p0 + t d, p1 + t d} passes the triangle within the radius and the leaf's own error; the walk follows the axis' midpoint
// c(t) = (p0 + p1) / 2 + t d.
//
// The box.  A child box is inflated on axis k by |a_k| / 2 + R,
//   R = r * kCapBoxRel + M * kCapBoxAbs:
// a point of the axis lies within |a_k| / 2 of the midpoint on axis k, so the midpoint's line meets the box inflated by |a_k| / 2 + rho
// whenever a point of the axis comes within rho of the box.  rho is the sphere's, r (1 + 2 u) + 28 u M for a vertex or an edge at p0
// or at p1 (sweep.h), with two changes.  The axis edge {P - a, a} can be as long as the capsule, not as a triangle's edge: its
// projections m - a (md / ee) and d - a (nd / ee) lose u |a| <= 2 u M each, as much again.  And the side face's and the face's
// t = (+-r |n| - s0) / dot(n, d) carries the rounding of dot(n, d), 3 u |n| |d|, which moves the point along d by t * 3 u |d| and so
// its height over the plane by at most 3 u times the distance travelled, itself at most 4 M for a point that ends over a triangle.
// Together under 64 u M = 2^-18 M; taken as 2^-15 M, which leaves room for the slab's own arithmetic (the midpoint, p - centre, the
// fp16 decode's fma, two products with the 1-ulp reciprocal: under 24 u M) and for a feature whose dp cancels: when d runs along a
// within an angle of 2^-8 the axis edges' dp = d - a (nd / ee) keeps 2^-8 |d| of d with an error of u |d|, and the time it gives is
// good to 2^-16 of itself where the sphere's edge was good to 2^-24.  There the end spheres at p0 and p1 meet the mesh first in
// exact arithmetic, and an axis edge that still wins does so within 2^-16 of the distance travelled: the factor 8 covers it.
//
// The far cut.  A child is entered iff its slab interval meets [0, cut],
//   cut = min(tmax, best t) * kCapRelT + (M * kCapLinT + sqrt(r * (r + M)) * kCapSqrtT) / |d|:
// sweep.h's, its two absolute terms doubled for the second set of roundings above (2^-16 M and 2^-7 sqrt(r (r + M))).  With d = 0 the
// cut is +inf and the slab admits exactly the boxes the inflated midpoint lies in.
//
// The plane.  The swept axis {p0 + s a + t d} lies in the plane through the midpoint with normal a x d.  For ANY vector w the points
// of the swept axis that can touch a box satisfy |dot(w, x - mid)| <= |dot(w, a)| / 2 + t |dot(w, d)|, and t |d| <= |x - mid| + |a| / 2
// <= sqrt(3) (2 M + r) <= D = 4 M + 2 r for an x within r of the scene box.  So with w the computed, normalised cross product (whatever its
// rounding made of it: when a and d are nearly parallel it points anywhere) a child is entered only if
//   |dot(w, centre - mid)| <= sum_k |w_k| h_k + R * kCapPlaneRel + |dot(w, a)| / 2 + D |dot(w, d)| / |d| + M * kCapPlaneAbs,
// h the box's half extent: the right-hand side's last three terms are formed once per cast from the computed w, so a w that is not
// perpendicular to the swept axis widens its own test.  kCapPlaneRel covers |w| = 1 +- 2^-20 (one v_rsq_f32), kCapPlaneAbs the
// rounding of the three dot products (under 32 u M) and of the two measured ones.  A cross product without usable length (d = 0,
// a = 0, a length whose square leaves fp32's range) gives w = 0, and the test admits everything.
constexpr float kCapBoxRel = 1.0f + 0x1p-20f;
constexpr float kCapBoxAbs = 0x1p-15f;
constexpr float kCapRelT = 1.0f + 0x1p-16f;
constexpr float kCapLinT = 0x1p-16f;
constexpr float kCapSqrtT = 0x1p-7f;
constexpr float kCapPlaneRel = 1.0f + 0x1p-10f;
constexpr float kCapPlaneAbs = 0x1p-16f;
// The product walks with the plane test (DESIGN.md section 39 has the measurement that decides it).
constexpr bool kCapsulePlane = true;

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  casts: n records of three float4 {p0.xyz,
// radius | p1.xyz, tmax | d.xyz, ignored}; out: n records of two float4 (pt_capsule_cast_hit).  Both DEVICE, 16-byte aligned,
// 1 <= n <= 2^31 - 1.  scene_scale: scene_max_abs (query_launch.h) of the scene box.
hipError_t launch_query_capsule_cast(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                     hipStream_t stream);
// blocked: n bytes, 1 where some triangle has a time of impact within [0, tmax]; a lane leaves the walk at its first such triangle.
hipError_t launch_query_capsule_cast_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n,
                                         uint8_t* blocked, hipStream_t stream);
// The same records, and per cast how many inner nodes it visited and how many triangles it tested (acgpt_test.h
// pt_debug_capsule_cast_visits).  plane: the product's walk (true) or the walk without the plane axis (false).
hipError_t launch_capsule_cast_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                      uint2* visits, bool plane, hipStream_t stream);

}  // namespace ptd
