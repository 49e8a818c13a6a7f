// tricast_device.h — the device functions of the translating-triangle casts (tricast.hip): the query record CastQuery, which is
// cast_walk.h's per-query struct, the time of impact of one pair cast_pair and the record of a finished walk.  The walk is
// cast_walk.h's; this unit's own are the leaf statement cast_pair, the centre line of the query's box with each child box inflated by
// the box's half extent (tricast.h: by a little more), the cut of tricast.h, and no extra admission test.  The start-overlap test is
// tritri_device.h's tri_tri_intersect.  Include only from a unit built with -ffp-contract=off (the statement is evaluated as written,
// and tests/tricast_ref.py mirrors it operation for operation).
#pragma once
#include "tricast.h"
#include "cast_walk.h"
#include "tritri_device.h"

namespace ptd {

// What a lane keeps of its cast.  set() returns whether the cast can touch something: every coordinate of the triangle, of d and of
// the three edge vectors finite, tmax >= 0 and no NaN (include/acgpt.h: "a miss before any traversal"); a cast that cannot is zeroed.
// line() then fills the slab test's view of it (tricast.h): the centre line of the query's box and the inflation per axis.
struct CastQuery {
    static constexpr bool kAdmits = false, kTracksCut = false;
    f3 a0, a1, a2, d;
    float tmax;         // +inf is the largest finite t: a time of impact of +inf stands for "no candidate"
    f3 inv;             // finite 1-ulp reciprocals of d
    f3 qc;              // cq, the centre of the query's box, minus the centre of HSpace for FMT 11
    f3 infl;            // hq + R
    __device__ __forceinline__ bool set(const f3& a0_, const f3& a1_, const f3& a2_, const f3& d_, float tmax_, bool have)
    {
        const f3 f1 = a1_ - a0_, f2 = a2_ - a0_, g = a2_ - a1_;
        const bool ok = have && __builtin_isfinite(a0_.x) && __builtin_isfinite(a0_.y) && __builtin_isfinite(a0_.z) && __builtin_isfinite(a1_.x) &&
                        __builtin_isfinite(a1_.y) && __builtin_isfinite(a1_.z) && __builtin_isfinite(a2_.x) && __builtin_isfinite(a2_.y) && __builtin_isfinite(a2_.z) &&
                        __builtin_isfinite(d_.x) && __builtin_isfinite(d_.y) && __builtin_isfinite(d_.z) && __builtin_isfinite(f1.x) && __builtin_isfinite(f1.y) &&
                        __builtin_isfinite(f1.z) && __builtin_isfinite(f2.x) && __builtin_isfinite(f2.y) && __builtin_isfinite(f2.z) && __builtin_isfinite(g.x) &&
                        __builtin_isfinite(g.y) && __builtin_isfinite(g.z) && tmax_ >= 0.0f;      // false when tmax is a NaN
        a0 = ok ? a0_ : mk(0.0f); a1 = ok ? a1_ : mk(0.0f); a2 = ok ? a2_ : mk(0.0f); d = ok ? d_ : mk(0.0f);
        tmax = ok ? fminf(tmax_, FLT_MAX) : 0.0f;
        return ok;
    }
    template <int FMT>
    __device__ __forceinline__ void line(float scene_scale, const HSpace& hs)
    {
        const f3 lo = mk(fmin3(a0.x, a1.x, a2.x), fmin3(a0.y, a1.y, a2.y), fmin3(a0.z, a1.z, a2.z));
        const f3 hi = mk(fmax3(a0.x, a1.x, a2.x), fmax3(a0.y, a1.y, a2.y), fmax3(a0.z, a1.z, a2.z));
        const f3 cq = mk(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z);
        const float big = scene_scale + fmax3(fmaxf(fabsf(lo.x), fabsf(hi.x)), fmaxf(fabsf(lo.y), fabsf(hi.y)), fmaxf(fabsf(lo.z), fabsf(hi.z)));
        const float R = big * kCastBoxAbs;
        inv = mk(finite_rcp(d.x), finite_rcp(d.y), finite_rcp(d.z));
        infl = mk(fmaxf(hi.x - cq.x, cq.x - lo.x) + R, fmaxf(hi.y - cq.y, cq.y - lo.y) + R, fmaxf(hi.z - cq.z, cq.z - lo.z) + R);
        qc = FMT == 11 ? mk(cq.x - hs.cx, cq.y - hs.cy, cq.z - hs.cz) : cq;
    }
    // cast i of the array, or an inert one for a lane past n.  The eighth, twelfth and sixteenth float are loaded with their float4
    // and never used.
    template <int FMT>
    __device__ __forceinline__ bool load(const float4* __restrict__ casts, uint32_t i, uint32_t n, float scene_scale, const HSpace& hs)
    {
        float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, g2 = g0, g3 = g0;
        if (i < n) { g0 = casts[4ull * i]; g1 = casts[4ull * i + 1ull]; g2 = casts[4ull * i + 2ull]; g3 = casts[4ull * i + 3ull]; }
        const bool ok = set(mk(g0.x, g0.y, g0.z), mk(g1.x, g1.y, g1.z), mk(g2.x, g2.y, g2.z), mk(g3.x, g3.y, g3.z), g0.w, i < n);
        line<FMT>(scene_scale, hs);
        return ok;
    }
    // cut of tricast.h for tb = min(tmax, best t); at most FLT_MAX, so that a box the line never reaches (entry +inf) is not entered
    __device__ __forceinline__ float cut(float tb) const { return fminf(tb * kCastRelT, FLT_MAX); }
    __device__ __forceinline__ float toi(const float4& r0, const float4& r1, const float4& r2) const;      // cast_pair<false>'s t
};

struct CastPair { float t, feature; f3 c; };

// include/acgpt.h's ray(o, r; p, k1, k2): the crossing test of the line o + t r with the triangle {p, p + k1, p + k2}, without an
// upper end.  Every compare is false on a NaN.
__device__ __forceinline__ bool cast_ray(const f3& o, const f3& r, const f3& p, const f3& k1, const f3& k2, float& t)
{
    const f3 pv = cross(r, k2);
    float det = dot(k1, pv);
    const f3 tv = o - p;
    float U = dot(tv, pv);
    const f3 qv = cross(tv, k1);
    float V = dot(r, qv), T = dot(k2, qv);
    const bool neg = det < 0.0f;
    det = neg ? -det : det; U = neg ? -U : U; V = neg ? -V : V; T = neg ? -T : T;
    t = T / det + 0.0f;
    return (det > 0.0f) & (U >= 0.0f) & (V >= 0.0f) & (U + V <= det) & (T >= 0.0f);
}

// The query edge {P, D} moving along d against the scene edge {A, E}; c: the contact on the scene edge.
__device__ __forceinline__ bool cast_edges(const f3& P, const f3& D, const f3& A, const f3& E, const f3& d, float& t, f3& c)
{
    const f3 n = cross(D, E);
    float det = dot(d, n);
    const f3 w = A - P;
    float T = dot(w, n), S = dot(d, cross(w, E)), G = dot(d, cross(w, D));
    const bool neg = det < 0.0f;
    det = neg ? -det : det; T = neg ? -T : T; S = neg ? -S : S; G = neg ? -G : G;
    t = T / det + 0.0f;
    const float k = G / det;
    c = mk(A.x + E.x * k, A.y + E.y * k, A.z + E.z * k);
    return (det > 0.0f) & (S >= 0.0f) & (S <= det) & (G >= 0.0f) & (G <= det) & (T >= 0.0f);
}

__device__ __forceinline__ bool cast_inside(const f3& c, const f3& lo, const f3& hi, float eps)
{
    return (c.x >= lo.x - eps) & (c.x <= hi.x + eps) & (c.y >= lo.y - eps) & (c.y <= hi.y + eps) & (c.z >= lo.z - eps) & (c.z <= hi.z + eps);
}

// One feature's offer: taken when it is accepted, its guard holds and its t is below the pair's so far (ties stay with the lower
// feature).  The select is pinned as tritri_device.h's fold is, so that the lane masks of 16 features do not pile up in scalar
// registers and the next feature does not start early.
template <bool FULL>
__device__ __forceinline__ void cast_offer(CastPair& best, bool ok, float t, float feature, const f3& c)
{
    const bool take = ok & (t < best.t);
    best.t = take ? t : best.t;
    if (FULL) {
        best.feature = take ? feature : best.feature;
        best.c = mk(take ? c.x : best.c.x, take ? c.y : best.c.y, take ? c.z : best.c.z);
    }
    asm volatile("" : "+v"(best.t));
    __builtin_amdgcn_sched_barrier(0);
}

// The time of impact of the triangle {a0, a1, a2} translating along d with the scene triangle {v0, v0 + e1, v0 + e2}, +inf when there
// is none: include/acgpt.h's statement, the 16 features as selects on one instruction stream.  FULL: also the feature and the
// contact (the record's; the walk needs t alone).
template <bool FULL>
__device__ __forceinline__ CastPair cast_pair(const CastQuery& q, const f3& v0, const f3& e1, const f3& e2)
{
    const f3 f1 = q.a1 - q.a0, f2 = q.a2 - q.a0, g = q.a2 - q.a1;
    const f3 w1 = v0 + e1, w2 = v0 + e2, h = e2 - e1;
    const f3 qlo = mk(fmin3(q.a0.x, q.a1.x, q.a2.x), fmin3(q.a0.y, q.a1.y, q.a2.y), fmin3(q.a0.z, q.a1.z, q.a2.z));
    const f3 qhi = mk(fmax3(q.a0.x, q.a1.x, q.a2.x), fmax3(q.a0.y, q.a1.y, q.a2.y), fmax3(q.a0.z, q.a1.z, q.a2.z));
    const f3 slo = mk(fmin3(v0.x, w1.x, w2.x), fmin3(v0.y, w1.y, w2.y), fmin3(v0.z, w1.z, w2.z));
    const f3 shi = mk(fmax3(v0.x, w1.x, w2.x), fmax3(v0.y, w1.y, w2.y), fmax3(v0.z, w1.z, w2.z));
    const float big_s = fmax3(fmaxf(fabsf(slo.x), fabsf(shi.x)), fmaxf(fabsf(slo.y), fabsf(shi.y)), fmaxf(fabsf(slo.z), fabsf(shi.z)));
    const float big_q = fmax3(fmaxf(fabsf(qlo.x), fabsf(qhi.x)), fmaxf(fabsf(qlo.y), fabsf(qhi.y)), fmaxf(fabsf(qlo.z), fabsf(qhi.z)));
    const float eps = 0x1p-16f * (big_s + big_q);
    CastPair best;
    best.t = INFINITY; best.feature = 16.0f; best.c = mk(0.0f);
    const f3 nd = -q.d;
    float t;
    f3 c;
    bool acc;
    // 0, 1, 2: a corner of the query against the scene triangle
    acc = cast_ray(q.a0, q.d, v0, e1, e2, t); c = mk(q.a0.x + q.d.x * t, q.a0.y + q.d.y * t, q.a0.z + q.d.z * t);
    cast_offer<FULL>(best, acc & cast_inside(c, slo, shi, eps), t, 0.0f, c);
    acc = cast_ray(q.a1, q.d, v0, e1, e2, t); c = mk(q.a1.x + q.d.x * t, q.a1.y + q.d.y * t, q.a1.z + q.d.z * t);
    cast_offer<FULL>(best, acc & cast_inside(c, slo, shi, eps), t, 1.0f, c);
    acc = cast_ray(q.a2, q.d, v0, e1, e2, t); c = mk(q.a2.x + q.d.x * t, q.a2.y + q.d.y * t, q.a2.z + q.d.z * t);
    cast_offer<FULL>(best, acc & cast_inside(c, slo, shi, eps), t, 2.0f, c);
    // 3, 4, 5: a corner of the scene triangle against the query, which it meets coming along -d
    acc = cast_ray(v0, nd, q.a0, f1, f2, t); c = mk(v0.x - q.d.x * t, v0.y - q.d.y * t, v0.z - q.d.z * t);
    cast_offer<FULL>(best, acc & cast_inside(c, qlo, qhi, eps), t, 3.0f, v0);
    acc = cast_ray(w1, nd, q.a0, f1, f2, t); c = mk(w1.x - q.d.x * t, w1.y - q.d.y * t, w1.z - q.d.z * t);
    cast_offer<FULL>(best, acc & cast_inside(c, qlo, qhi, eps), t, 4.0f, w1);
    acc = cast_ray(w2, nd, q.a0, f1, f2, t); c = mk(w2.x - q.d.x * t, w2.y - q.d.y * t, w2.z - q.d.z * t);
    cast_offer<FULL>(best, acc & cast_inside(c, qlo, qhi, eps), t, 5.0f, w2);
    // 6 + 3 i + j: edge i of the query against edge j of the scene triangle
#define ACGPT_CAST_EDGE(K, P, D, A, E)                                                                                    \
    acc = cast_edges(P, D, A, E, q.d, t, c);                                                                              \
    cast_offer<FULL>(best, acc & cast_inside(mk(c.x - q.d.x * t, c.y - q.d.y * t, c.z - q.d.z * t), qlo, qhi, eps), t, K, c);
    ACGPT_CAST_EDGE(6.0f, q.a0, f1, v0, e1)
    ACGPT_CAST_EDGE(7.0f, q.a0, f1, v0, e2)
    ACGPT_CAST_EDGE(8.0f, q.a0, f1, w1, h)
    ACGPT_CAST_EDGE(9.0f, q.a0, f2, v0, e1)
    ACGPT_CAST_EDGE(10.0f, q.a0, f2, v0, e2)
    ACGPT_CAST_EDGE(11.0f, q.a0, f2, w1, h)
    ACGPT_CAST_EDGE(12.0f, q.a1, g, v0, e1)
    ACGPT_CAST_EDGE(13.0f, q.a1, g, v0, e2)
    ACGPT_CAST_EDGE(14.0f, q.a1, g, w1, h)
#undef ACGPT_CAST_EDGE
    // 15: the start overlap overrides the others
    const bool start = tri_tri_intersect(q.a0, f1, f2, qlo, qhi, v0, e1, e2);
    best.t = start ? 0.0f : best.t;
    if (FULL) {
        best.feature = start ? 15.0f : best.feature;
        best.c = mk(start ? 0.0f : best.c.x, start ? 0.0f : best.c.y, start ? 0.0f : best.c.z);
    }
    return best;
}

__device__ __forceinline__ float CastQuery::toi(const float4& r0, const float4& r1, const float4& r2) const
{
    return cast_pair<false>(*this, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x)).t;
}

// The walk of the per-triangle and the posed kernels.  tmax: the cast's own, or a smaller one that the posed kernel has seen in its
// pose's key.  The query is held by reference.
using TriCastWalk = CastWalk<false, const CastQuery&>;

// The record of a finished walk: the pair statement once more on the winner (the same statement on the same inputs gives the same
// bits, and the walk carries three registers for its best candidate), or the miss record.  query_triangle: the fourth word.
__device__ __forceinline__ void cast_record(const DeviceScene& sc, const CastQuery& q, bool found, const TriCastWalk& best, uint32_t query_triangle, float4& o0, float4& o1)
{
    o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, __uint_as_float(query_triangle));
    o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (found) {
        const TriRecord* tp = sc.tris + best.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
        const CastPair p = cast_pair<true>(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
        const float4 sr = sc.shade[best.slot];
        o0 = make_float4(p.t, __uint_as_float(best.prim), p.feature, __uint_as_float(query_triangle));
        o1 = make_float4(p.c.x, p.c.y, p.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
    }
}

}  // namespace ptd
