// tridist.hip — the kernels behind pt_query_triangle_distance (include/acgpt.h).
//
//   k_query_triangle_distance<FMT, COUNT>   one query triangle per lane from a device array: the closest scene triangle within
//                                           max_radius, then the record (distance, triangle, feature, material, the point on the query
//                                           triangle, the point on the scene triangle).  COUNT also writes how many inner nodes the
//                                           lane visited and how many triangles it tested, and takes the flag that switches bound (b)
//                                           off (the test hook's instantiation).
//
// The shape is segment.hip's: FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes; the walk is ordered by a lower
// bound of the squared distance from the query triangle to each child box, and the leaves run the triangle-to-triangle statement.
// 256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h (stack_entries * 64 words per wave).  A query is
// three 16-byte loads and a record three 16-byte stores per lane.  Lanes past n and lanes whose query is a miss before any traversal
// stay in the wave, inactive.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the statement is evaluated as written, and tests/tridist_ref.py mirrors it operation for operation.
// The box bounds are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "tridist.h"
#include "bvh_walk.h"
#include "tridist_device.h"

namespace ptd {

// TriDistQuery, triangle_triangle, the box bounds and the walk's policy TriDistWalk: tridist_device.h, which poses.hip shares.  The
// kernel below keeps its own text around the walk; tridist_device.h says why.

template <int FMT, bool COUNT>
__global__ void __launch_bounds__(256)
k_query_triangle_distance(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ tris, uint32_t n, float4* __restrict__ out,
                          uint2* __restrict__ visits_out, uint32_t flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    // query i of the array, or an inert one for a lane past n.  ok: the lane has a query and the query can find something — every
    // coordinate and every component of the three edge vectors finite, max_radius >= 0 and no NaN (include/acgpt.h: "a miss before
    // any traversal").  The eighth and twelfth float are loaded with their float4 and never used.
    TriDistQuery t;
    t.a0 = t.a1 = t.a2 = t.f1 = t.f2 = t.g = mk(0.0f);
    float r2 = 0.0f;
    bool ok = false;
    if (i < n) {
        const float4 g0 = tris[3ull * i], g1 = tris[3ull * i + 1ull], g2 = tris[3ull * i + 2ull];
        t.a0 = mk(g0.x, g0.y, g0.z);
        t.a1 = mk(g1.x, g1.y, g1.z);
        t.a2 = mk(g2.x, g2.y, g2.z);
        t.f1 = t.a1 - t.a0;
        t.f2 = t.a2 - t.a0;
        t.g = t.a2 - t.a1;
        r2 = g0.w * g0.w;
        ok = __builtin_isfinite(g0.x) && __builtin_isfinite(g0.y) && __builtin_isfinite(g0.z) && __builtin_isfinite(g1.x) && __builtin_isfinite(g1.y) &&
             __builtin_isfinite(g1.z) && __builtin_isfinite(g2.x) && __builtin_isfinite(g2.y) && __builtin_isfinite(g2.z) && __builtin_isfinite(t.f1.x) &&
             __builtin_isfinite(t.f1.y) && __builtin_isfinite(t.f1.z) && __builtin_isfinite(t.f2.x) && __builtin_isfinite(t.f2.y) && __builtin_isfinite(t.f2.z) &&
             __builtin_isfinite(t.g.x) && __builtin_isfinite(t.g.y) && __builtin_isfinite(t.g.z) && g0.w >= 0.0f;   // false when max_radius is a NaN
        if (!ok) t.a0 = t.a1 = t.a2 = t.f1 = t.f2 = t.g = mk(0.0f);
    }
    // the bounds' view of the query and the lane's absolute term (tridist.h)
    TriBound tb;
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
    const float lane_abs = segment_abs_term(abs_term, qs);
    TriDistWalk best(t, tb, r2, lane_abs);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, COUNT>(sc, st, ok, best, visits);
    if (i >= n) return;
    float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, __uint_as_float(0xFFFFFFFFu)), o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o2 = o1;
    if (ok && best.slot >= 0) {
        // the winner's triangle once more: the same statement on the same inputs gives the same bits, and the walk carries three
        // registers for its best candidate instead of ten
        const TriRecord* tp = sc.tris + best.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
        const TriPair p = triangle_triangle<true>(t, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
        const float4 sr = sc.shade[best.slot];
        o0 = make_float4(sqrtf(p.d2), __uint_as_float(best.prim), p.feature, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
        o1 = make_float4(p.q.x, p.q.y, p.q.z, 0.0f);
        o2 = make_float4(p.c.x, p.c.y, p.c.z, 0.0f);
    }
    out[3ull * i] = o0;
    out[3ull * i + 1ull] = o1;
    out[3ull * i + 2ull] = o2;
    if (COUNT) visits_out[i] = visits;
}

hipError_t launch_query_triangle_distance(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* tris, uint32_t n, float4* out,
                                          hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_triangle_distance<11, false>, stack_entries, n, stream, sc, stack_entries, abs_term, tris, n, out, (uint2*)nullptr, 0u);
    return launch_lane_stack(k_query_triangle_distance<0, false>, stack_entries, n, stream, sc, stack_entries, abs_term, tris, n, out, (uint2*)nullptr, 0u);
}

hipError_t launch_triangle_distance_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* tris, uint32_t n, float4* out,
                                           uint2* visits, uint32_t flags, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_triangle_distance<11, true>, stack_entries, n, stream, sc, stack_entries, abs_term, tris, n, out, visits, flags);
    return launch_lane_stack(k_query_triangle_distance<0, true>, stack_entries, n, stream, sc, stack_entries, abs_term, tris, n, out, visits, flags);
}

}  // namespace ptd
