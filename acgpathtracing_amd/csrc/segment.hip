// segment.hip — the kernels behind pt_query_segments (include/acgpt.h).
//
//   k_query_segments<FMT, COUNT>   one segment per lane from a device array: the closest triangle within max_radius, then the record
//                                  (distance, triangle, parameter on the segment, feature, point on the triangle, material).  COUNT also
//                                  writes how many inner nodes the lane visited and how many triangles it tested, and takes the flag
//                                  that switches bound (b) off (the test hook's instantiation).
//
// The shape is nearest.hip's: FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes; the walk is ordered by a lower
// bound of the squared distance from the segment to each child box, and the leaves run the segment-to-triangle statement.  256-lane
// workgroups over a one-dimensional grid, the lane stack of query_launch.h (stack_entries * 64 words per wave).  A segment is two
// 16-byte loads and a record two 16-byte stores per lane.  Lanes past n and lanes whose segment is a miss before any traversal stay in
// the wave, inactive.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the statement is evaluated as written, and tests/segment_ref.py mirrors it operation for operation.
// The box bounds are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "segment.h"
#include "bvh_walk.h"
#include "segment_device.h"      // closest_on_triangle (closest_point.h), clamp01, segment_edge: shared with tridist.hip; segment_triangle: with capsule.hip

namespace ptd {

// What a lane keeps of its segment for the box bounds: the midpoint (relative to HSpace's centre for FMT 11), the half extent of the
// segment's own box, and the three axes n_i = normalize(d x axis_i) — n_x = (0, d.z, -d.y) / |.|, n_y = (-d.z, 0, d.x) / |.|,
// n_z = (d.y, -d.x, 0) / |.|, two components each.  An axis whose cross product has no usable length (a segment along a coordinate
// axis, a point, a length whose square leaves fp32's range) has both components 0 and contributes 0.
struct SegBound { f3 m, hd; float xy, xz, yx, yz, zx, zy; };

__device__ __forceinline__ void axis_pair(float u, float v, float& nu, float& nv)
{
    const float l2 = __builtin_fmaf(u, u, v * v);
    const float inv = (l2 > 1e-30f && l2 < 1e30f) ? __builtin_amdgcn_rsqf(l2) : 0.0f;
    nu = u * inv; nv = v * inv;
}

// Lower bound of the squared distance from the segment to a box with centre offset t = c - m and half extent h: the larger of
//   (a) the point bound of nearest.hip from the midpoint with h enlarged per axis by |d| / 2 — the box against the segment's box;
//   (b) per axis n_i the separation |t . n_i| - sum_j h_j |n_i,j|, clamped at 0 and squared: n_i is perpendicular to d, so the segment
//       projects onto a point, and a projection onto a unit vector cannot lengthen a distance.
__device__ __forceinline__ float segment_box_bound(const f3& t, const f3& h, const SegBound& sb)
{
    const float ex = fmaxf(fabsf(t.x) - h.x - sb.hd.x, 0.0f), ey = fmaxf(fabsf(t.y) - h.y - sb.hd.y, 0.0f), ez = fmaxf(fabsf(t.z) - h.z - sb.hd.z, 0.0f);
    const float ba = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    const float sx = fabsf(__builtin_fmaf(t.y, sb.xy, t.z * sb.xz)) - __builtin_fmaf(h.y, fabsf(sb.xy), h.z * fabsf(sb.xz));
    const float sy = fabsf(__builtin_fmaf(t.x, sb.yx, t.z * sb.yz)) - __builtin_fmaf(h.x, fabsf(sb.yx), h.z * fabsf(sb.yz));
    const float sz = fabsf(__builtin_fmaf(t.x, sb.zx, t.y * sb.zy)) - __builtin_fmaf(h.x, fabsf(sb.zx), h.y * fabsf(sb.zy));
    const float sm = fmaxf(fmaxf(sx, sy), fmaxf(sz, 0.0f));
    return fmaxf(ba, sm * sm);
}
//   FMT 11: per axis t = c * is - (m - centre), h * is (c, h the fp16 centre and half extent: world = g * is + centre): v_fma_mix_f32
//           decodes.  An empty child has h < 0.
//   FMT 0:  t = (lo + hi) / 2 - m, h = (hi - lo) / 2 from the fp32 planes.  An empty child has lo = +inf.
// A NaN for an empty child, which no threshold admits.
__device__ __forceinline__ float seg_bound_hc(uint32_t px, uint32_t py, uint32_t pz, const SegBound& sb, const HSpace& hs)
{
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const f3 t = mk(__builtin_fmaf((float)hx.x, hs.isx, -sb.m.x), __builtin_fmaf((float)hy.x, hs.isy, -sb.m.y), __builtin_fmaf((float)hz.x, hs.isz, -sb.m.z));
    const f3 h = mk((float)hx.y * hs.isx, (float)hy.y * hs.isy, (float)hz.y * hs.isz);
    const float b = segment_box_bound(t, h, sb);
    return (float)hx.y < 0.0f ? __builtin_nanf("") : b;
}
__device__ __forceinline__ float seg_bound_f32(const SegBound& sb, float lx, float ly, float lz, float hx, float hy, float hz)
{
    const f3 t = mk(__builtin_fmaf(0.5f, lx + hx, -sb.m.x), __builtin_fmaf(0.5f, ly + hy, -sb.m.y), __builtin_fmaf(0.5f, lz + hz, -sb.m.z));
    const f3 h = mk(0.5f * (hx - lx), 0.5f * (hy - ly), 0.5f * (hz - lz));
    const float b = segment_box_bound(t, h, sb);
    return lx <= hx ? b : __builtin_nanf("");
}

// One segment per lane through the two-child BVH (bvh_walk.h): nearest.hip's walk with the segment's bound and statement.  thr is
// min(best d2, r2) widened (segment.h): a child is entered iff its bound is at most thr and it is not empty; of two such children the
// nearer is entered and the other pushed.  The boxes only prune: the winner is decided by the statement, d2 <= r2, smallest d2, ties to
// the lowest triangle index, whatever order the walk reaches the triangles in.
struct SegmentWalk {
    f3 p0, p1, d;
    float a;
    SegBound sb;
    float r2, abs_term, thr;
    float d2; int slot; uint32_t prim;      // the best candidate so far
    __device__ __forceinline__ SegmentWalk(const f3& p0_, const f3& p1_, const f3& d_, float a_, const SegBound& sb_, float r2_, float abs_term_)
        : p0(p0_), p1(p1_), d(d_), a(a_), sb(sb_), r2(r2_), abs_term(abs_term_), thr(r2_ * kNearRel + abs_term_), d2(INFINITY), slot(-1), prim(0xFFFFFFFFu) {}
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        admit_by_bound(seg_bound_hc(qa.x, qa.y, qa.z, sb, hs), seg_bound_hc(qb.x, qb.y, qb.z, sb, hs), thr, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& na, const float4& nb, const float4& nc, bool& h0, bool& h1, bool& first0) const
    {
        admit_by_bound(seg_bound_f32(sb, na.x, na.y, na.z, na.w, nb.x, nb.y), seg_bound_f32(sb, nb.z, nb.w, nc.x, nc.y, nc.z, nc.w), thr, h0, h1, first0);
    }
    __device__ __forceinline__ bool leaf(int slot_, const float4& r0, const float4& r1, const float4& r2_)
    {
        const SegPoint p = segment_triangle<false>(p0, p1, d, a, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
        const uint32_t prim_ = __float_as_uint(r2_.y);
        if (p.d2 <= r2 && (p.d2 < d2 || (p.d2 == d2 && prim_ < prim))) {
            d2 = p.d2; slot = slot_; prim = prim_;
            thr = p.d2 * kNearRel + abs_term;
        }
        return false;
    }
};

template <int FMT, bool COUNT>
__global__ void __launch_bounds__(256)
k_query_segments(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ segments, uint32_t n, float4* __restrict__ out,
                 uint2* __restrict__ visits_out, uint32_t flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    // segment i of the array, or an inert one for a lane past n.  ok: the lane has a segment and the segment can find something —
    // every coordinate and every component of d finite, max_radius >= 0 and no NaN (include/acgpt.h: "a miss before any traversal").
    // The eighth float is loaded with its float4 and never used.
    f3 p0 = mk(0.0f), p1 = mk(0.0f), d = mk(0.0f);
    float r2 = 0.0f;
    bool ok = false;
    if (i < n) {
        const float4 g0 = segments[2ull * i], g1 = segments[2ull * i + 1ull];
        p0 = mk(g0.x, g0.y, g0.z);
        p1 = mk(g1.x, g1.y, g1.z);
        d = p1 - p0;
        r2 = g0.w * g0.w;
        ok = __builtin_isfinite(g0.x) && __builtin_isfinite(g0.y) && __builtin_isfinite(g0.z) && __builtin_isfinite(g1.x) && __builtin_isfinite(g1.y) &&
             __builtin_isfinite(g1.z) && __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z) && g0.w >= 0.0f;   // false when max_radius is a NaN
        if (!ok) { p0 = mk(0.0f); p1 = mk(0.0f); d = mk(0.0f); }
    }
    const float a = dot(d, d);
    // the bounds' view of the segment and the lane's absolute term (segment.h)
    SegBound sb;
    sb.m = mk(__builtin_fmaf(0.5f, d.x, p0.x), __builtin_fmaf(0.5f, d.y, p0.y), __builtin_fmaf(0.5f, d.z, p0.z));
    if (FMT == 11) sb.m = mk(sb.m.x - sc.hspace.cx, sb.m.y - sc.hspace.cy, sb.m.z - sc.hspace.cz);
    sb.hd = mk(0.5f * fabsf(d.x), 0.5f * fabsf(d.y), 0.5f * fabsf(d.z));
    axis_pair(d.z, -d.y, sb.xy, sb.xz);
    axis_pair(-d.z, d.x, sb.yx, sb.yz);
    axis_pair(d.y, -d.x, sb.zx, sb.zy);
    if (COUNT && (flags & kSegmentNoAxes)) { sb.xy = sb.xz = sb.yx = sb.yz = sb.zx = sb.zy = 0.0f; }
    const float qs = fmaxf(fmaxf(fmaxf(fabsf(p0.x), fabsf(p0.y)), fmaxf(fabsf(p0.z), fabsf(p1.x))), fmaxf(fabsf(p1.y), fabsf(p1.z)));
    const float lane_abs = segment_abs_term(abs_term, qs);
    SegmentWalk best(p0, p1, d, a, sb, r2, lane_abs);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, COUNT>(sc, st, ok, best, visits);
    if (i >= n) return;
    float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (ok && best.slot >= 0) {
        // the winner's triangle once more: the same statement on the same inputs gives the same bits, and the walk carries three
        // registers for its best candidate instead of nine
        const TriRecord* tp = sc.tris + best.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
        const SegPoint p = segment_triangle<true>(p0, p1, d, a, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
        const float4 sr = sc.shade[best.slot];
        o0 = make_float4(sqrtf(p.d2), __uint_as_float(best.prim), p.s, p.feature);
        o1 = make_float4(p.c.x, p.c.y, p.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
    }
    out[2ull * i] = o0;
    out[2ull * i + 1ull] = o1;
    if (COUNT) visits_out[i] = visits;
}

hipError_t launch_query_segments(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* segments, uint32_t n, float4* out,
                                 hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_segments<11, false>, stack_entries, n, stream, sc, stack_entries, abs_term, segments, n, out, (uint2*)nullptr, 0u);
    return launch_lane_stack(k_query_segments<0, false>, stack_entries, n, stream, sc, stack_entries, abs_term, segments, n, out, (uint2*)nullptr, 0u);
}

hipError_t launch_segments_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* segments, uint32_t n, float4* out,
                                  uint2* visits, uint32_t flags, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_segments<11, true>, stack_entries, n, stream, sc, stack_entries, abs_term, segments, n, out, visits, flags);
    return launch_lane_stack(k_query_segments<0, true>, stack_entries, n, stream, sc, stack_entries, abs_term, segments, n, out, visits, flags);
}

}  // namespace ptd
