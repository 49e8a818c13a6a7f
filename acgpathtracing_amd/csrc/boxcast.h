// boxcast.h — swept oriented-box casts on the scene's BVH: pt_query_box_cast, pt_query_box_cast_any (include/acgpt.h states the
// contract; tests/boxcast_ref.py is the NumPy statement of the time of impact and the whole record).  Kernels in boxcast.hip, the leaf
// test and the record in boxcast_device.h; they read oriented_device.h / overlap_device.h and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// The widenings of the walk, derived as capsule.h derives the capsule's.  u = 2^-24, S = the largest |coordinate|
// of the scene box, per cast C = the largest |coordinate| of the centre, hs = hx + hy + hz and
//   M = S + C + hs,
// which bounds every component of v0 - c, of every local coordinate the leaf forms (|L(p)| <= 1.001 sqrt 3 |p|_inf, so 2 M bounds
// those) and of a box corner.  At the time t the leaf accepts, the 13 entry times are all <= t and the 13 exit times all >= t as
// computed: the triangle, moved by -D t in the box's frame, meets the cube |q_j| <= h_j on every axis up to the rounding of the
// projections, of the two subtractions and of the division.  The walk follows the centre's line c + t d.
//
// The box.  A child box is inflated on world axis k by
//   H_k + M * kBoxCastAbs + hs * kBoxCastOrtho,          H_k = sum_j |A_kj| h_j:
// oriented.h's world-axis threshold.  Section 38 bounds what the static statement lets through by 22 u (S + C) and the walk's own
// arithmetic by 84 u (S + C) in all.  The swept statement adds, per axis, the rounding of the speed s (3.02 u |axis| |D|), of -r - hi
// and r - lo (u each) and of the quotient (u), which move the triangle's projection at time t by at most 6 u of (|lo| + |hi| + r +
// |s| t); |s| t is the travel projected on the axis, and a cast that ends on a triangle of the scene has travelled at most
// 2 sqrt 3 M, so the sum stays under 8 M |axis| and the term under 48 u M per unit of axis.  Together under 132 u M; taken as
// 2^-15 M = 512 u M, a factor 3.8 of room, which also covers the slab's arithmetic (c minus the node space's centre, the fp16 decode's
// fma, two products with the 1-ulp reciprocal: under 24 u M).  kBoxCastOrtho is oriented.h's kOBoxOrtho: axes orthonormal to 2^-10
// move every |p_k - c_k| by at most 1.75 * 2^-10 hs.
//
// The far cut.  The leaf compares its computed t with tmax and with the best t exactly, so a triangle that can still win has a
// computed t <= tb = min(tmax, best t), and at that t the centre lies in its leaf box inflated as above.  The slab's interval holds
// that t up to its own rounding (two products with a 1-ulp reciprocal, relative 4 u of t, and the absolute 24 u M above divided by
// |d_k| >= |d| / sqrt 3 on the axis that decides):
//   cut = tb * kBoxCastRelT + M * kBoxCastLinT / |d|,
// 2^-16 against 4 u = 2^-22 relative and 2^-16 M against 42 u M = 2^-18.6 M absolute.  With d = 0 the cut is +inf (clamped to
// FLT_MAX) and the slab admits exactly the boxes the inflated centre lies in: oriented.h's world axes.
//
// The extra axes (AXES; DESIGN.md section 40 has the measurement that decides).  In the statement's own local coordinates a triangle
// accepted at time t has a point p with a_j . (p - c) in t D_j +- (h_j + m), D_j = dot(a_j, d) as the statement computes it, whatever
// the axes' orthonormality (oriented.h, "box axes").  D_j carries 3.02 u |d| of rounding, taken as delta = |d| * kBoxCastDirRel, so
// for t in [0, cut] the projection lies in
//   [min(0, cut (D_j - delta)) - h_j - m,  max(0, cut (D_j + delta)) + h_j + m],        m = M * kBoxCastAbs,
// and a child box of centre b and half extent g is entered only if [a_j . (b - c) -+ sum_k |A_kj| g_k] meets that interval.
// On an axis w perpendicular to d the swept box does not grow: for ANY vector w a point p = c + t d + A^-T q of the swept box has
//   |dot(w, p - c)| <= sum_i h_i |dot(w, a_i)| + t |dot(w, d)| + 1.75 * 2^-10 * 3 hs |w|,       t |d| <= R = 2 M * sqrt 3 <= 4 M.
// With w_j the computed, normalised cross(a_j, d), whatever its rounding made of it, a child is entered only if
//   |dot(w_j, b - c)| <= sum_k |w_jk| g_k + [sum_i h_i |dot(w_j, a_i)| + 4 M |dot(w_j, d)| / |d|] * kBoxCastCrossRel + hs * kBoxCastCrossOrtho + m:
// the bracket is measured once per cast from the computed w_j, so a w_j that is not perpendicular to d widens its own test
// (capsule.h's construction).  kBoxCastCrossRel covers |w_j| = 1 +- 2^-20 (one v_rsq_f32) and the rounding of the measured dot
// products.  A cross product without usable length (d = 0, d along a_j) gives w_j = 0, and the test admits everything.
constexpr float kBoxCastAbs = 0x1p-15f;
constexpr float kBoxCastOrtho = 0x1p-9f;
constexpr float kBoxCastRelT = 1.0f + 0x1p-16f;
constexpr float kBoxCastLinT = 0x1p-16f;
constexpr float kBoxCastDirRel = 0x1p-20f;
constexpr float kBoxCastCrossRel = 1.0f + 0x1p-10f;
constexpr float kBoxCastCrossOrtho = 0x1p-7f;
// The product walks with the extra axes (DESIGN.md section 40 has the measurement that decides it).
constexpr bool kBoxCastAxes = true;

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  casts: n records of five float4 {m0 m1 m2 m3 |
// m4 m5 m6 m7 | m8 m9 m10 m11 | hx hy hz - | d.xyz tmax}; out: n records of three float4 (pt_box_cast_hit).  Both DEVICE, 16-byte
// aligned, 1 <= n <= 2^31 - 1.  scene_scale: scene_max_abs (query_launch.h) of the scene box.
hipError_t launch_query_box_toi(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                hipStream_t stream);
// blocked: n bytes, 1 where some triangle has a time of impact within [0, tmax]; a lane leaves the walk at its first such triangle.
hipError_t launch_query_box_toi_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n,
                                    uint8_t* blocked, hipStream_t stream);
// The same records, and per cast how many inner nodes it visited and how many triangles it tested (acgpt_test.h
// pt_debug_box_cast_visits).  axes: the walk with the six extra axes (true) or the slab alone (false).
hipError_t launch_box_toi_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                 uint2* visits, bool axes, hipStream_t stream);

}  // namespace ptd
