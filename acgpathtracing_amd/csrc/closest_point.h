// closest_point.h — the closest point of a triangle to a point, and the two lower bounds of the squared distance from a point to a
// child box.  One copy: pt_query_nearest's d2, weights and closest point are what pt_query_nearest_k, pt_query_within_any,
// pt_query_sweep (start overlap, the record's weights), pt_query_segments (features 0 and 1) and pt_query_triangle_distance (features
// 0 to 5) are defined by, bit for bit.  Evaluated as written (-ffp-contract=off); tests/nearest_ref.py mirrors closest_on_triangle
// operation for operation.  The box bounds are outside that contract (they only prune) and use explicit fused multiply-adds.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

struct ClosestPoint { float d2, v, w; f3 c; };

// Closest point of the triangle {v0, v0 + ab, v0 + ac} to q: Ericson, Real-Time Collision Detection 5.1.5, on the record's own edge
// vectors.  The regions are decided by compares on d1..d6 and va, vb, vc and applied as selects in reverse order of priority (vertex
// A, vertex B, edge AB, vertex C, edge AC, edge BC, face), so a wave's lanes run one instruction stream; the one division of the
// region that wins is selected before it is taken.  (v, w): the weights of v1 and v2.  A NaN anywhere ends in a NaN d2, which is no
// candidate.  A caller that needs d2 alone, or d2 and c, drops the rest and the compiler removes it.
__device__ __forceinline__ ClosestPoint closest_on_triangle(const f3& q, const f3& v0, const f3& ab, const f3& ac)
{
    const f3 ap = q - v0;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const f3 bp = ap - ab;
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const f3 cp = ap - ac;
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const bool at_a = d1 <= 0.0f && d2 <= 0.0f;
    const bool at_b = d3 >= 0.0f && d4 <= d3;
    const bool on_ab = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool at_c = d6 >= 0.0f && d5 <= d6;
    const bool on_ac = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool on_bc = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
    float num = 1.0f, den = (va + vb) + vc;
    if (on_bc) { num = e43; den = e43 + e56; }
    if (on_ac) { num = d2; den = d2 - d6; }
    if (on_ab) { num = d1; den = d1 - d3; }
    const float t = num / den;
    float v = vb * t, w = vc * t;
    if (on_bc) { v = 1.0f - t; w = t; }
    if (on_ac) { v = 0.0f; w = t; }
    if (at_c) { v = 0.0f; w = 1.0f; }
    if (on_ab) { v = t; w = 0.0f; }
    if (at_b) { v = 1.0f; w = 0.0f; }
    if (at_a) { v = 0.0f; w = 0.0f; }
    ClosestPoint r;
    r.v = v; r.w = w;
    r.c = mk((v0.x + ab.x * v) + ac.x * w, (v0.y + ab.y * v) + ac.y * w, (v0.z + ab.z * v) + ac.z * w);
    const f3 s = q - r.c;
    r.d2 = dot(s, s);
    return r;
}
// The same on a TriRecord's three words (bvh_walk.h says where v0, e1 and e2 sit in them).
__device__ __forceinline__ ClosestPoint closest_on_triangle(const f3& q, const float4& r0, const float4& r1, const float4& r2)
{
    return closest_on_triangle(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
}

// Lower bound of the squared distance from the point to one child box; a NaN for an empty child, which no threshold admits (+inf
// would pass under max_radius = +inf, where the threshold is +inf too).
//   FMT 11: qc = q - centre of HSpace, once per lane; per axis t = c * is - qc (c, h the fp16 centre and half extent: world = g * is +
//           centre), e = max(|t| - h * is, 0): two v_fma_mix_f32 and a max.  An empty child has h < 0.
//   FMT 0:  e = max(lo - q, q - hi, 0) from the fp32 planes.  An empty child has lo = +inf.
__device__ __forceinline__ float box_bound_hc(uint32_t px, uint32_t py, uint32_t pz, const f3& qc, const HSpace& hs)
{
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const float tx = __builtin_fmaf((float)hx.x, hs.isx, -qc.x), ty = __builtin_fmaf((float)hy.x, hs.isy, -qc.y), tz = __builtin_fmaf((float)hz.x, hs.isz, -qc.z);
    const float ex = fmaxf(__builtin_fmaf((float)hx.y, -hs.isx, fabsf(tx)), 0.0f);
    const float ey = fmaxf(__builtin_fmaf((float)hy.y, -hs.isy, fabsf(ty)), 0.0f);
    const float ez = fmaxf(__builtin_fmaf((float)hz.y, -hs.isz, fabsf(tz)), 0.0f);
    const float b = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    return (float)hx.y < 0.0f ? __builtin_nanf("") : b;
}
__device__ __forceinline__ float box_bound_f32(const f3& q, float lx, float ly, float lz, float hx, float hy, float hz)
{
    const float ex = fmaxf(fmaxf(lx - q.x, q.x - hx), 0.0f), ey = fmaxf(fmaxf(ly - q.y, q.y - hy), 0.0f), ez = fmaxf(fmaxf(lz - q.z, q.z - hz), 0.0f);
    const float b = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    return lx <= hx ? b : __builtin_nanf("");
}

}  // namespace ptd
