// segment_device.h — the device functions the segment query (segment.hip) and the triangle-distance query (tridist.hip) share: the
// closest point of a triangle to a point, the clamp and the segment-against-edge statement of include/acgpt.h's segment section.
// Evaluated as written (-ffp-contract=off); tests/segment_ref.py mirrors them operation for operation.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// nearest.hip's closest_on_triangle, operation for operation (pt_query_nearest's d2 and closest point): features 0 and 1.
__device__ __forceinline__ float seg_closest_on_triangle(const f3& q, const f3& v0, const f3& ab, const f3& ac, f3& c)
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
    c = mk((v0.x + ab.x * v) + ac.x * w, (v0.y + ab.y * v) + ac.y * w, (v0.z + ab.z * v) + ac.z * w);
    const f3 s = q - c;
    return dot(s, s);
}

// Selects, not fminf / fmaxf: a -0 stays a -0 and a NaN a NaN, as in the NumPy statement.
__device__ __forceinline__ float clamp01(float q)
{
    q = q < 0.0f ? 0.0f : q;
    return q > 1.0f ? 1.0f : q;
}

// The segment {p0, d} (a = dot(d, d)) against the edge {A, E}: Ericson, Real-Time Collision Detection 5.1.9.  The cases — a segment
// or an edge without length, parallel lines, the edge parameter leaving [0, 1] and the re-projection that follows — are compares
// applied as selects on numerators and denominators, so a wave's lanes run one instruction stream and an edge costs two divisions:
// s0 on the segment, then either t on the edge (tnom / e, inside [0, 1]) or the re-projected s (t clamped to an end).  Every
// denominator a select keeps is > 0.  s: the parameter on the segment, c: the point on the edge.
__device__ __forceinline__ float segment_edge(const f3& p0, const f3& d, float a, const f3& A, const f3& E, float& s, f3& c)
{
    const f3 r = p0 - A;
    const float e = dot(E, E), b = dot(d, E), cc = dot(d, r), f = dot(E, r);
    const bool a_ok = a > 0.0f, e_ok = e > 0.0f;
    const float den = a * e - b * b;
    const bool both = a_ok && e_ok && den > 0.0f;
    const bool only_a = a_ok && !e_ok;
    float num1 = only_a ? -cc : 0.0f, den1 = only_a ? a : 1.0f;
    if (both) { num1 = b * f - cc * e; den1 = den; }
    const float s0 = clamp01(num1 / den1);
    const float tnom = b * s0 + f;
    const bool lo = e_ok && tnom < 0.0f, hi = e_ok && tnom > e, out = lo || hi;
    float num2 = e_ok ? tnom : 0.0f, den2 = e_ok ? e : 1.0f;
    if (lo) num2 = -cc;
    if (hi) num2 = b - cc;
    if (out) den2 = a;
    if (out && !a_ok) { num2 = 0.0f; den2 = 1.0f; }
    const float q2 = clamp01(num2 / den2);
    s = out ? q2 : s0;
    const float t = lo ? 0.0f : (hi ? 1.0f : q2);
    const f3 ps = mk(p0.x + d.x * s, p0.y + d.y * s, p0.z + d.z * s);
    c = mk(A.x + E.x * t, A.y + E.y * t, A.z + E.z * t);
    const f3 w = ps - c;
    return dot(w, w);
}

}  // namespace ptd
