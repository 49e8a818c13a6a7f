// tricast_device.h — the device functions of the translating-triangle casts (tricast.hip): the query record CastQuery, the time of
// impact of one pair cast_pair, the slab test of the query box's centre line and the walk's policy CastWalk.  The start-overlap test
// is tritri_device.h's tri_tri_intersect.  Include only from a unit built with -ffp-contract=off (the statement is evaluated as
// written, and tests/tricast_ref.py mirrors it operation for operation).  The slab test is outside that contract (it only prunes) and
// uses explicit fused multiply-adds.
#pragma once
#include "tricast.h"
#include "bvh_walk.h"
#include "tritri_device.h"

#include <cfloat>

namespace ptd {

// What a lane keeps of its cast.  set() returns whether the cast can touch something: every coordinate of the triangle, of d and of
// the three edge vectors finite, tmax >= 0 and no NaN (include/acgpt.h: "a miss before any traversal"); a cast that cannot is zeroed.
struct CastQuery {
    f3 a0, a1, a2, d;
    float tmax;         // +inf is the largest finite t: a time of impact of +inf stands for "no candidate"
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
    // cast i of the array, or an inert one for a lane past n.  The eighth, twelfth and sixteenth float are loaded with their float4
    // and never used.
    __device__ __forceinline__ bool load(const float4* __restrict__ casts, uint32_t i, uint32_t n)
    {
        float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, g2 = g0, g3 = g0;
        if (i < n) { g0 = casts[4ull * i]; g1 = casts[4ull * i + 1ull]; g2 = casts[4ull * i + 2ull]; g3 = casts[4ull * i + 3ull]; }
        return set(mk(g0.x, g0.y, g0.z), mk(g1.x, g1.y, g1.z), mk(g2.x, g2.y, g2.z), mk(g3.x, g3.y, g3.z), g0.w, i < n);
    }
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

// The slab test's view of the cast (tricast.h): the query box's centre line and the inflation per axis.
struct CastSlab {
    f3 inv;             // finite 1-ulp reciprocals of d
    f3 o;               // cq (FMT 0), cq - centre of HSpace (FMT 11)
    f3 infl;            // hq + R
};

template <int FMT>
__device__ __forceinline__ CastSlab cast_slab_setup(const CastQuery& q, float scene_scale, const HSpace& hs)
{
    const f3 lo = mk(fmin3(q.a0.x, q.a1.x, q.a2.x), fmin3(q.a0.y, q.a1.y, q.a2.y), fmin3(q.a0.z, q.a1.z, q.a2.z));
    const f3 hi = mk(fmax3(q.a0.x, q.a1.x, q.a2.x), fmax3(q.a0.y, q.a1.y, q.a2.y), fmax3(q.a0.z, q.a1.z, q.a2.z));
    const f3 cq = mk(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z);
    const float big = scene_scale + fmax3(fmaxf(fabsf(lo.x), fabsf(hi.x)), fmaxf(fabsf(lo.y), fabsf(hi.y)), fmaxf(fabsf(lo.z), fabsf(hi.z)));
    const float R = big * kCastBoxAbs;
    CastSlab s;
    s.inv = mk(finite_rcp(q.d.x), finite_rcp(q.d.y), finite_rcp(q.d.z));
    s.infl = mk(fmaxf(hi.x - cq.x, cq.x - lo.x) + R, fmaxf(hi.y - cq.y, cq.y - lo.y) + R, fmaxf(hi.z - cq.z, cq.z - lo.z) + R);
    s.o = FMT == 11 ? mk(cq.x - hs.cx, cq.y - hs.cy, cq.z - hs.cz) : cq;
    return s;
}

// Entry and exit of the centre line in one child box inflated by s.infl, clipped to [0, cut]; tn = NaN for an empty child, which no
// compare admits (an inflated empty box would be hit).  c: the box centre minus cq, e: the inflated half extent, per axis, in world
// units; the products with +-1e30 for a zero direction component give +-inf or 0, never a NaN.
__device__ __forceinline__ void cast_slab(const f3& c, const f3& e, const f3& inv, float cut, bool empty, float& tn, float& tf)
{
    const float x0 = (c.x - e.x) * inv.x, x1 = (c.x + e.x) * inv.x;
    const float y0 = (c.y - e.y) * inv.y, y1 = (c.y + e.y) * inv.y;
    const float z0 = (c.z - e.z) * inv.z, z1 = (c.z + e.z) * inv.z;
    tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
    tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), cut));
    if (empty) tn = __builtin_nanf("");
}
__device__ __forceinline__ void cast_slab_hc(uint32_t px, uint32_t py, uint32_t pz, const CastSlab& s, const HSpace& hs, float cut, float& tn, float& tf)
{
    // world = g * is + centre: c = centre_g * is - o, e = half_g * is + infl, one v_fma_mix_f32 each
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const f3 c = mk(__builtin_fmaf((float)hx.x, hs.isx, -s.o.x), __builtin_fmaf((float)hy.x, hs.isy, -s.o.y), __builtin_fmaf((float)hz.x, hs.isz, -s.o.z));
    const f3 e = mk(__builtin_fmaf((float)hx.y, hs.isx, s.infl.x), __builtin_fmaf((float)hy.y, hs.isy, s.infl.y), __builtin_fmaf((float)hz.y, hs.isz, s.infl.z));
    cast_slab(c, e, s.inv, cut, (float)hx.y < 0.0f, tn, tf);
}
__device__ __forceinline__ void cast_slab_f32(float lx, float ly, float lz, float hx, float hy, float hz, const CastSlab& s, float cut, float& tn, float& tf)
{
    // the half extent from the rounded centre m, so that [m - e, m + e] holds [lo, hi] to an ulp of the extent
    const f3 m = mk(0.5f * lx + 0.5f * hx, 0.5f * ly + 0.5f * hy, 0.5f * lz + 0.5f * hz);
    const f3 c = m - s.o;
    const f3 e = mk(fmaxf(hx - m.x, m.x - lx) + s.infl.x, fmaxf(hy - m.y, m.y - ly) + s.infl.y, fmaxf(hz - m.z, m.z - lz) + s.infl.z);
    cast_slab(c, e, s.inv, cut, !(lx <= hx), tn, tf);
}

// cut of tricast.h for tb = min(tmax, best t); at most FLT_MAX, so that a box the line never reaches (entry +inf) is not entered
__device__ __forceinline__ float cast_cut(float tb) { return fminf(tb * kCastRelT, FLT_MAX); }

// One cast per lane through the two-child BVH (bvh_walk.h: the stack depth, the one-word entries).  The boxes only prune: the winner
// is decided by the leaf test, t <= tmax, smallest t, ties to the lowest triangle index, whatever order the walk reaches the triangles
// in.  tmax: the cast's own, or a smaller one that the posed kernel has seen in its pose's key.  ANY: leave at the first triangle with
// t <= tmax (slot >= 0 says so).
template <bool ANY>
struct CastWalk {
    const CastQuery& q;
    CastSlab s;
    float tmax, cut;
    float t; int slot; uint32_t prim;      // the best candidate so far
    __device__ __forceinline__ CastWalk(const CastQuery& q_, const CastSlab& s_, float tmax_) : q(q_), s(s_), tmax(tmax_), cut(cast_cut(tmax_)), t(INFINITY), slot(-1), prim(0xFFFFFFFFu) {}
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        cast_slab_hc(qa.x, qa.y, qa.z, s, hs, cut, n0, f0);
        cast_slab_hc(qb.x, qb.y, qb.z, s, hs, cut, n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        cast_slab_f32(a.x, a.y, a.z, a.w, b.x, b.y, s, cut, n0, f0);
        cast_slab_f32(b.z, b.w, c.x, c.y, c.z, c.w, s, cut, n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ bool leaf(int slot_, const float4& r0, const float4& r1, const float4& r2)
    {
        const float t_ = cast_pair<false>(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x)).t;
        const uint32_t prim_ = __float_as_uint(r2.y);
        if (ANY) {
            if (t_ <= tmax) { slot = slot_; return true; }
        } else if (t_ <= tmax && (t_ < t || (t_ == t && prim_ < prim))) {
            t = t_; slot = slot_; prim = prim_;
            cut = cast_cut(t_);
        }
        return false;
    }
};

// The record of a finished walk: the pair statement once more on the winner (the same statement on the same inputs gives the same
// bits, and the walk carries three registers for its best candidate), or the miss record.  query_triangle: the fourth word.
__device__ __forceinline__ void cast_record(const DeviceScene& sc, const CastQuery& q, bool ok, const CastWalk<false>& best, uint32_t query_triangle, float4& o0, float4& o1)
{
    o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, __uint_as_float(query_triangle));
    o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (ok && best.slot >= 0) {
        const TriRecord* tp = sc.tris + best.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
        const CastPair p = cast_pair<true>(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
        const float4 sr = sc.shade[best.slot];
        o0 = make_float4(p.t, __uint_as_float(best.prim), p.feature, __uint_as_float(query_triangle));
        o1 = make_float4(p.c.x, p.c.y, p.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
    }
}

}  // namespace ptd
