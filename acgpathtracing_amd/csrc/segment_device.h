// segment_device.h — the device functions the segment query (segment.hip) and the triangle-distance query (tridist.hip) share: the
// closest point of a triangle to a point (closest_point.h: pt_query_nearest's own, features 0 and 1), the clamp and the
// segment-against-edge statement of include/acgpt.h's segment section; and the whole segment-to-triangle statement, which the
// capsule cast (capsule.hip) shares with segment.hip: its start-overlap test and its record.
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

struct SegPoint { float d2, s, feature; f3 c; };

// Take candidate k if its d2 is smaller (ties stay with the lower feature); a NaN is no candidate.  The empty statement and the
// barrier close one sub-test before the next starts: left to itself the compiler runs the five side by side and keeps their state
// live together (tritri.hip's fold).
template <bool FULL>
__device__ __forceinline__ void seg_take(SegPoint& best, float d2, float s, float feature, const f3& c)
{
    const bool take = d2 < best.d2 || (best.d2 != best.d2 && d2 == d2);
    best.d2 = take ? d2 : best.d2;
    if (FULL) {
        best.s = take ? s : best.s;
        best.feature = take ? feature : best.feature;
        best.c = mk(take ? c.x : best.c.x, take ? c.y : best.c.y, take ? c.z : best.c.z);
    }
    asm volatile("" : "+v"(best.d2));
    __builtin_amdgcn_sched_barrier(0);
}

// The statement of include/acgpt.h: six sub-tests in the order of their feature numbers.  FULL = false is the walk's: d2 alone, the
// same operations on the same inputs, so the same bits.
template <bool FULL>
__device__ __forceinline__ SegPoint segment_triangle(const f3& p0, const f3& p1, const f3& d, float a, const f3& v0, const f3& e1, const f3& e2)
{
    SegPoint best;
    f3 c;
    float s = 0.0f;
    const ClosestPoint c0 = closest_on_triangle(p0, v0, e1, e2);
    best.d2 = c0.d2; best.c = c0.c;
    best.s = 0.0f; best.feature = 0.0f;
    asm volatile("" : "+v"(best.d2));
    __builtin_amdgcn_sched_barrier(0);
    const ClosestPoint c1 = closest_on_triangle(p1, v0, e1, e2);
    seg_take<FULL>(best, c1.d2, 1.0f, 1.0f, c1.c);
    float d2 = segment_edge(p0, d, a, v0, e1, s, c);
    seg_take<FULL>(best, d2, s, 2.0f, c);
    d2 = segment_edge(p0, d, a, v0, e2, s, c);
    seg_take<FULL>(best, d2, s, 3.0f, c);
    d2 = segment_edge(p0, d, a, v0 + e1, e2 - e1, s, c);
    seg_take<FULL>(best, d2, s, 4.0f, c);
    // feature 5: a two-sided Moeller-Trumbore test of {p0, d} against the triangle in plain multiplies and adds (not tri_test, whose
    // fused operations NumPy cannot mirror)
    const f3 pv = cross(d, e2);
    float det = dot(e1, pv);
    const f3 tv = p0 - v0;
    float U = dot(tv, pv);
    const f3 qv = cross(tv, e1);
    float V = dot(d, qv), T = dot(e2, qv);
    if (det < 0.0f) { det = -det; U = -U; V = -V; T = -T; }
    const bool crosses = det > 0.0f && U >= 0.0f && V >= 0.0f && U + V <= det && T >= 0.0f && T <= det;
    best.d2 = crosses ? 0.0f : best.d2;
    if (FULL) {
        const float sx = T / det;
        best.s = crosses ? sx : best.s;
        best.feature = crosses ? 5.0f : best.feature;
        best.c = mk(crosses ? p0.x + d.x * sx : best.c.x, crosses ? p0.y + d.y * sx : best.c.y, crosses ? p0.z + d.z * sx : best.c.z);
    }
    return best;
}

}  // namespace ptd
