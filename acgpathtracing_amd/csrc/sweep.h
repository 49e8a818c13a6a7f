// sweep.h — swept-sphere casts on the scene's BVH: pt_query_sweep, pt_query_sweep_any (include/acgpt.h states the contract;
// tests/sweep_ref.py is the NumPy statement of the time of impact and the whole record).  Kernels in sweep.hip; they read the render
// kernels' headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// The two widenings of the walk (DESIGN.md section 28 has the derivation in full).  u = 2^-24, S = the largest |coordinate| of the scene
// box, and per sweep M = S + max(|o.x|, |o.y|, |o.z|), which bounds every component of m = o - P the leaf test forms, and |d| = sqrt(dd).
//
// The box.  A child box is inflated on every axis by
//   R = r * kSweepBoxRel + M * kSweepBoxAbs.
// A feature is a candidate when its computed residual (mp for a vertex, mq for an edge) has dot <= rr.  m carries u |m| per component,
// t0 three roundings of a dot product and one division, d * t0 and the sum one each: the computed residual differs from the exact one
// of the same line by at most 8 u |m| <= 14 u M for a vertex, twice that for an edge (two projections), and rr = r * r and the compare
// add 2 u r.  So an accepted line passes the feature, and with it the child box that holds it, within r (1 + 2 u) + 28 u M: taken as
// r (1 + 2^-20) and 2^-17 M, which leaves 2^-18 M for the slab's own arithmetic (o - centre, the fp16 decode's fma, two products with
// the 1-ulp reciprocal: under 16 u M).  An edge the line runs along within an angle of 2^-8 loses more (its dp cancels); there the box
// still holds by the same factor 4.
//
// The far cut.  A child is entered iff its slab interval meets [0, cut],
//   cut = min(tmax, best t) * kSweepRelT + (M * kSweepLinT + sqrt(r * (r + M)) * kSweepSqrtT) / |d|.
// The leaf's t = t0 - sqrt(q) can lie below the entry of the exact line into the inflated box: t0 |d| is off by at most 14 u M, and
// q dd = rr - dot(mp, mp) by at most 2 u r^2 + 2 r * 28 u M + (28 u M)^2, whose square root is at most 2^-9 sqrt(r (r + M)) + 28 u M
// (sqrt(x + e) - sqrt(x) <= sqrt(e)).  Taken as 2^-17 M and 2^-8 sqrt(r (r + M)), a factor 2 and more.  kSweepRelT covers the rounding
// of the cut itself and of the slab's products, a few u of t.  With d = 0 the cut is +inf: nothing is pruned by t, and the slab admits
// exactly the boxes the centre lies in.
constexpr float kSweepBoxRel = 1.0f + 0x1p-20f;
constexpr float kSweepBoxAbs = 0x1p-17f;
constexpr float kSweepRelT = 1.0f + 0x1p-16f;
constexpr float kSweepLinT = 0x1p-17f;
constexpr float kSweepSqrtT = 0x1p-8f;

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  sweeps: n records of two float4 {o.xyz, d.x |
// d.yz, radius, tmax}; out: n records of two float4 (pt_sweep_hit).  Both DEVICE, 16-byte aligned, 1 <= n <= 2^31 - 1.  scene_scale:
// S, query_launch.h's scene_max_abs of the scene box the builder (or the last refit) recorded.
hipError_t launch_query_sweep(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n, float4* out,
                              hipStream_t stream);
// blocked: n bytes, 1 where some triangle has a time of impact within [0, tmax]; a lane leaves the walk at its first such triangle.
hipError_t launch_query_sweep_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n,
                                  uint8_t* blocked, hipStream_t stream);
// The same walk and records, and per sweep how many inner nodes it visited and how many triangles it tested (acgpt_test.h
// pt_debug_sweep_visits).
hipError_t launch_sweep_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n, float4* out,
                               uint2* visits, hipStream_t stream);

}  // namespace ptd
