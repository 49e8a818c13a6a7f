// tridist_device.h — the device functions the triangle-distance query (tridist.hip) shares with the posed-mesh queries (poses.hip):
// the triangle-to-triangle statement, the box bounds, the walk's policy TriDistWalk, and the three parts of a lane's work around the
// walk, for a kernel that forms its query triangle in registers: the query from its vertices (tri_dist_query), the bounds' view of it
// (tri_dist_bounds) and the record of the winner (tri_dist_record).  The statement, the bounds and the policy were moved here from
// tridist.hip as they were.  The three parts are k_query_triangle_distance's own statements, operation for operation;
// that kernel keeps its text in tridist.hip, because built from these functions its walk is the same instructions but the compiler
// orders some thirty instructions before and after it differently, and the existing code objects stay as they are (DESIGN.md
// section 36).
// Include only from a unit built with -ffp-contract=off: the statement is evaluated as written, and tests/tridist_ref.py mirrors it
// operation for operation.  The box bounds are outside that contract (they only prune) and use explicit fused multiply-adds.
#pragma once
#include "tridist.h"
#include "bvh_walk.h"
#include "segment_device.h"

namespace ptd {

// What a lane keeps of its query triangle: the vertices as given and the three edge vectors, one subtraction per component.
struct TriDistQuery { f3 a0, a1, a2, f1, f2, g; };

struct TriPair { float d2, feature; f3 q, c; };

// Take candidate k if its d2 is smaller (ties stay with the lower feature); a NaN is no candidate.  The empty statement and the
// barrier close one sub-test before the next starts (segment.hip's seg_take): fifteen sub-tests' state is never live together.
template <bool FULL>
__device__ __forceinline__ void tri_take(TriPair& best, float d2, float feature, const f3& q, const f3& c)
{
    const bool take = d2 < best.d2 || (best.d2 != best.d2 && d2 == d2);
    best.d2 = take ? d2 : best.d2;
    if (FULL) {
        best.feature = take ? feature : best.feature;
        best.q = mk(take ? q.x : best.q.x, take ? q.y : best.q.y, take ? q.z : best.q.z);
        best.c = mk(take ? c.x : best.c.x, take ? c.y : best.c.y, take ? c.z : best.c.z);
    }
    asm volatile("" : "+v"(best.d2));
    __builtin_amdgcn_sched_barrier(0);
}

// The segment section's crossing test of {p0, d} against {v0, e1, e2}: a two-sided Moeller-Trumbore test in plain multiplies and adds.
// T / det is the parameter on the segment of an accepted crossing.
__device__ __forceinline__ bool segment_crosses(const f3& p0, const f3& d, const f3& v0, const f3& e1, const f3& e2, float& T, float& det)
{
    const f3 pv = cross(d, e2);
    det = dot(e1, pv);
    const f3 tv = p0 - v0;
    float U = dot(tv, pv);
    const f3 qv = cross(tv, e1);
    float V = dot(d, qv);
    T = dot(e2, qv);
    if (det < 0.0f) { det = -det; U = -U; V = -V; T = -T; }
    return det > 0.0f && U >= 0.0f && V >= 0.0f && U + V <= det && T >= 0.0f && T <= det;
}

// An accepted crossing sets d2 = 0 exactly; of several the lowest feature number keeps the record (crossed: one was accepted before).
template <bool FULL>
__device__ __forceinline__ void tri_cross(TriPair& best, bool& crossed, float feature, const f3& p0, const f3& d, const f3& v0, const f3& e1, const f3& e2)
{
    float T, det;
    const bool acc = segment_crosses(p0, d, v0, e1, e2, T, det);
    best.d2 = acc ? 0.0f : best.d2;
    if (FULL) {
        const bool first = acc && !crossed;
        const float sx = T / det;
        const f3 x = mk(p0.x + d.x * sx, p0.y + d.y * sx, p0.z + d.z * sx);
        best.feature = first ? feature : best.feature;
        best.q = mk(first ? x.x : best.q.x, first ? x.y : best.q.y, first ? x.z : best.q.z);
        best.c = mk(first ? x.x : best.c.x, first ? x.y : best.c.y, first ? x.z : best.c.z);
        crossed = crossed || acc;
    }
    asm volatile("" : "+v"(best.d2));
    __builtin_amdgcn_sched_barrier(0);
}

// The statement of include/acgpt.h: twenty-one sub-tests in the order of their feature numbers.  FULL = false is the walk's: d2 alone,
// the same operations on the same inputs, so the same bits.  The three query edges are loops that are not unrolled: the edge is
// picked by selects on a wave-uniform counter, and one copy of three edge tests is what the registers hold.
template <bool FULL>
__device__ __forceinline__ TriPair triangle_triangle(const TriDistQuery& t, const f3& v0, const f3& e1, const f3& e2)
{
    TriPair best;
    f3 c;
    float s = 0.0f;
    // features 0, 1, 2: the query's vertices against the scene triangle
    ClosestPoint cp = closest_on_triangle(t.a0, v0, e1, e2);
    best.d2 = cp.d2; best.c = cp.c;
    best.q = t.a0; best.feature = 0.0f;
    asm volatile("" : "+v"(best.d2));
    __builtin_amdgcn_sched_barrier(0);
    cp = closest_on_triangle(t.a1, v0, e1, e2);
    tri_take<FULL>(best, cp.d2, 1.0f, t.a1, cp.c);
    cp = closest_on_triangle(t.a2, v0, e1, e2);
    tri_take<FULL>(best, cp.d2, 2.0f, t.a2, cp.c);
    // features 3, 4, 5: the scene triangle's vertices against the query
    const f3 w1 = v0 + e1, w2 = v0 + e2, h = e2 - e1;
    cp = closest_on_triangle(v0, t.a0, t.f1, t.f2);
    tri_take<FULL>(best, cp.d2, 3.0f, cp.c, v0);
    cp = closest_on_triangle(w1, t.a0, t.f1, t.f2);
    tri_take<FULL>(best, cp.d2, 4.0f, cp.c, w1);
    cp = closest_on_triangle(w2, t.a0, t.f1, t.f2);
    tri_take<FULL>(best, cp.d2, 5.0f, cp.c, w2);
    float d2;
    // features 6 + 3 i + j: query edge i against scene edge j, the segment query's own edge order on both sides
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        const f3 P = i == 2 ? t.a1 : t.a0;
        const f3 D = i == 0 ? t.f1 : (i == 1 ? t.f2 : t.g);
        const float a = dot(D, D);
        const float base = 6.0f + 3.0f * (float)i;
        d2 = segment_edge(P, D, a, v0, e1, s, c);
        tri_take<FULL>(best, d2, base, mk(P.x + D.x * s, P.y + D.y * s, P.z + D.z * s), c);
        d2 = segment_edge(P, D, a, v0, e2, s, c);
        tri_take<FULL>(best, d2, base + 1.0f, mk(P.x + D.x * s, P.y + D.y * s, P.z + D.z * s), c);
        d2 = segment_edge(P, D, a, w1, h, s, c);
        tri_take<FULL>(best, d2, base + 2.0f, mk(P.x + D.x * s, P.y + D.y * s, P.z + D.z * s), c);
    }
    // features 15, 16, 17: a query edge crosses the scene triangle; 18, 19, 20: a scene edge crosses the query triangle
    bool crossed = false;
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        const f3 P = i == 2 ? t.a1 : t.a0;
        const f3 D = i == 0 ? t.f1 : (i == 1 ? t.f2 : t.g);
        tri_cross<FULL>(best, crossed, 15.0f + (float)i, P, D, v0, e1, e2);
    }
#pragma unroll 1
    for (int j = 0; j < 3; j++) {
        const f3 A = j == 2 ? w1 : v0;
        const f3 E = j == 0 ? e1 : (j == 1 ? e2 : h);
        tri_cross<FULL>(best, crossed, 18.0f + (float)j, A, E, t.a0, t.f1, t.f2);
    }
    return best;
}

// What a lane keeps of its query for the box bounds: the midpoint m of the triangle's own box (relative to HSpace's centre for FMT 11)
// and its half extent hd; the unit normal n = normalize(cross(f1, f2)) and the interval [pc - pw, pc + pw] that the three vertices,
// taken relative to m, project onto along the COMPUTED n.  In exact arithmetic the interval is the point n . (a0 - m); as computed it
// has the width the normal's rounding gives it (a sliver's normal is a poor one), and the bound holds for whatever unit vector n came
// out as.  A normal without usable length (a degenerate query, a squared length outside 1e-30 .. 1e30) is 0 and contributes 0.
struct TriBound { f3 m, hd, n; float pc, pw; };

// Lower bound of the squared distance from the query triangle to a box with centre offset t = c - m and half extent h: the larger of
//   (a) segment_box_bound's first term with the triangle's midpoint and half extent — the box against the triangle's box;
//   (b) the separation along n, |t . n - pc| - pw - sum_k h_k |n_k|, clamped at 0 and squared: a projection onto a unit vector cannot
//       lengthen a distance.  Without it a large diagonal triangle enters every box of its own bounding box.
__device__ __forceinline__ float triangle_box_bound(const f3& t, const f3& h, const TriBound& tb)
{
    const float ex = fmaxf(fabsf(t.x) - h.x - tb.hd.x, 0.0f), ey = fmaxf(fabsf(t.y) - h.y - tb.hd.y, 0.0f), ez = fmaxf(fabsf(t.z) - h.z - tb.hd.z, 0.0f);
    const float ba = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    const float along = __builtin_fmaf(t.x, tb.n.x, __builtin_fmaf(t.y, tb.n.y, __builtin_fmaf(t.z, tb.n.z, -tb.pc)));
    const float reach = __builtin_fmaf(h.x, fabsf(tb.n.x), __builtin_fmaf(h.y, fabsf(tb.n.y), __builtin_fmaf(h.z, fabsf(tb.n.z), tb.pw)));
    const float sm = fmaxf(fabsf(along) - reach, 0.0f);
    return fmaxf(ba, sm * sm);
}
// The decodes are segment.hip's seg_bound_hc / seg_bound_f32.  A NaN for an empty child, which no threshold admits.
__device__ __forceinline__ float tri_bound_hc(uint32_t px, uint32_t py, uint32_t pz, const TriBound& tb, const HSpace& hs)
{
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const f3 t = mk(__builtin_fmaf((float)hx.x, hs.isx, -tb.m.x), __builtin_fmaf((float)hy.x, hs.isy, -tb.m.y), __builtin_fmaf((float)hz.x, hs.isz, -tb.m.z));
    const f3 h = mk((float)hx.y * hs.isx, (float)hy.y * hs.isy, (float)hz.y * hs.isz);
    const float b = triangle_box_bound(t, h, tb);
    return (float)hx.y < 0.0f ? __builtin_nanf("") : b;
}
__device__ __forceinline__ float tri_bound_f32(const TriBound& tb, float lx, float ly, float lz, float hx, float hy, float hz)
{
    const f3 t = mk(__builtin_fmaf(0.5f, lx + hx, -tb.m.x), __builtin_fmaf(0.5f, ly + hy, -tb.m.y), __builtin_fmaf(0.5f, lz + hz, -tb.m.z));
    const f3 h = mk(0.5f * (hx - lx), 0.5f * (hy - ly), 0.5f * (hz - lz));
    const float b = triangle_box_bound(t, h, tb);
    return lx <= hx ? b : __builtin_nanf("");
}

// One query per lane through the two-child BVH (bvh_walk.h): segment.hip's walk with the triangle's bound and statement.  A child is
// entered iff its bound is at most thr and it is not empty; of two such children the nearer is entered and the other pushed.  The
// boxes only prune: the winner is decided by the statement, d2 <= r2, smallest d2, ties to the lowest triangle index, whatever order
// the walk reaches the triangles in.
struct TriDistWalk {
    TriDistQuery t;
    TriBound tb;
    float r2, abs_term, thr;
    float d2; int slot; uint32_t prim;      // the best candidate so far
    __device__ __forceinline__ TriDistWalk(const TriDistQuery& t_, const TriBound& tb_, float r2_, float abs_term_)
        : t(t_), tb(tb_), r2(r2_), abs_term(abs_term_), thr(r2_ * kNearRel + abs_term_), d2(INFINITY), slot(-1), prim(0xFFFFFFFFu) {}
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        admit_by_bound(tri_bound_hc(qa.x, qa.y, qa.z, tb, hs), tri_bound_hc(qb.x, qb.y, qb.z, tb, hs), thr, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& na, const float4& nb, const float4& nc, bool& h0, bool& h1, bool& first0) const
    {
        admit_by_bound(tri_bound_f32(tb, na.x, na.y, na.z, na.w, nb.x, nb.y), tri_bound_f32(tb, nb.z, nb.w, nc.x, nc.y, nc.z, nc.w), thr, h0, h1, first0);
    }
    __device__ __forceinline__ bool leaf(int slot_, const float4& r0, const float4& r1, const float4& r2_)
    {
        const TriPair p = triangle_triangle<false>(t, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
        const uint32_t prim_ = __float_as_uint(r2_.y);
        if (p.d2 <= r2 && (p.d2 < d2 || (p.d2 == d2 && prim_ < prim))) {
            d2 = p.d2; slot = slot_; prim = prim_;
            thr = p.d2 * kNearRel + abs_term;
        }
        return false;
    }
};

// The query of the three vertices and max_radius.  True: the query can find something — every coordinate and every component of the
// three edge vectors finite, max_radius >= 0 and no NaN (include/acgpt.h: "a miss before any traversal"); otherwise t is all zeros.
__device__ __forceinline__ bool tri_dist_query(TriDistQuery& t, const f3& a0, const f3& a1, const f3& a2, float max_radius)
{
    t.a0 = a0;
    t.a1 = a1;
    t.a2 = a2;
    t.f1 = t.a1 - t.a0;
    t.f2 = t.a2 - t.a0;
    t.g = t.a2 - t.a1;
    const bool ok = __builtin_isfinite(a0.x) && __builtin_isfinite(a0.y) && __builtin_isfinite(a0.z) && __builtin_isfinite(a1.x) && __builtin_isfinite(a1.y) &&
                    __builtin_isfinite(a1.z) && __builtin_isfinite(a2.x) && __builtin_isfinite(a2.y) && __builtin_isfinite(a2.z) && __builtin_isfinite(t.f1.x) &&
                    __builtin_isfinite(t.f1.y) && __builtin_isfinite(t.f1.z) && __builtin_isfinite(t.f2.x) && __builtin_isfinite(t.f2.y) && __builtin_isfinite(t.f2.z) &&
                    __builtin_isfinite(t.g.x) && __builtin_isfinite(t.g.y) && __builtin_isfinite(t.g.z) && max_radius >= 0.0f;   // false when max_radius is a NaN
    if (!ok) t.a0 = t.a1 = t.a2 = t.f1 = t.f2 = t.g = mk(0.0f);
    return ok;
}

// The bounds' view of the query (tb) and the lane's absolute term (tridist.h), which is returned.  COUNT: the test hook's
// instantiation, which takes the flag that switches bound (b) off.
template <int FMT, bool COUNT>
__device__ __forceinline__ float tri_dist_bounds(const DeviceScene& sc, const TriDistQuery& t, float abs_term, uint32_t flags, TriBound& tb)
{
    const f3 lo = mk(fminf(fminf(t.a0.x, t.a1.x), t.a2.x), fminf(fminf(t.a0.y, t.a1.y), t.a2.y), fminf(fminf(t.a0.z, t.a1.z), t.a2.z));
    const f3 hi = mk(fmaxf(fmaxf(t.a0.x, t.a1.x), t.a2.x), fmaxf(fmaxf(t.a0.y, t.a1.y), t.a2.y), fmaxf(fmaxf(t.a0.z, t.a1.z), t.a2.z));
    tb.hd = mk(0.5f * (hi.x - lo.x), 0.5f * (hi.y - lo.y), 0.5f * (hi.z - lo.z));      // hi - lo is a difference of two vertices: finite
    tb.m = lo + tb.hd;
    const f3 cr = cross(t.f1, t.f2);
    const float l2 = __builtin_fmaf(cr.x, cr.x, __builtin_fmaf(cr.y, cr.y, cr.z * cr.z));
    const bool usable = l2 > 1e-30f && l2 < 1e30f && !(COUNT && (flags & kTriDistNoPlane));      // false for a NaN
    const float inv = usable ? __builtin_amdgcn_rsqf(l2) : 0.0f;
    tb.n = mk(usable ? cr.x * inv : 0.0f, usable ? cr.y * inv : 0.0f, usable ? cr.z * inv : 0.0f);
    const float p0 = dot(tb.n, t.a0 - tb.m), p1 = dot(tb.n, t.a1 - tb.m), p2 = dot(tb.n, t.a2 - tb.m);
    const float pmin = fminf(fminf(p0, p1), p2), pmax = fmaxf(fmaxf(p0, p1), p2);
    tb.pw = 0.5f * (pmax - pmin);
    tb.pc = pmin + tb.pw;
    if (FMT == 11) tb.m = mk(tb.m.x - sc.hspace.cx, tb.m.y - sc.hspace.cy, tb.m.z - sc.hspace.cz);
    const float qs = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(hi.x))), fmaxf(fabsf(hi.y), fabsf(hi.z)));
    return segment_abs_term(abs_term, qs);
}

// The record of a lane after its walk: the miss record, or the winner's.  The winner's triangle once more: the same statement on the
// same inputs gives the same bits, and the walk carries three registers for its best candidate instead of ten.
__device__ __forceinline__ void tri_dist_record(const DeviceScene& sc, const TriDistQuery& t, bool ok, const TriDistWalk& best, float4& o0, float4& o1, float4& o2)
{
    o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, __uint_as_float(0xFFFFFFFFu));
    o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o2 = o1;
    if (ok && best.slot >= 0) {
        const TriRecord* tp = sc.tris + best.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
        const TriPair p = triangle_triangle<true>(t, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
        const float4 sr = sc.shade[best.slot];
        o0 = make_float4(sqrtf(p.d2), __uint_as_float(best.prim), p.feature, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
        o1 = make_float4(p.q.x, p.q.y, p.q.z, 0.0f);
        o2 = make_float4(p.c.x, p.c.y, p.c.z, 0.0f);
    }
}

}  // namespace ptd
