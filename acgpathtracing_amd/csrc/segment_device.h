// segment_device.h — the device functions the segment query (segment.hip) and the triangle-distance query (tridist.hip) share: the
// closest point of a triangle to a point (closest_point.h: pt_query_nearest's own, features 0 and 1), the clamp and the
// segment-against-edge statement of include/acgpt.h's segment section.
// Evaluated as written (-ffp-contract=off); tests/segment_ref.py mirrors them operation for operation.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "closest_point.h"

namespace ptd {

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
