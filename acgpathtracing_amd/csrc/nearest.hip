// nearest.hip — the kernels behind pt_query_nearest (include/acgpt.h).
//
//   k_query_nearest<FMT, COUNT>   one point per lane from a device array: the closest triangle within max_radius, then the record
//                                 (distance, triangle, weights of v1 and v2, closest point, material).  COUNT also writes how many
//                                 inner nodes the lane visited and how many triangles it tested (the test hook's instantiation).
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk is ordered by a
// lower bound of the squared distance from the point to each child box instead of a ray's slab interval, and the leaves run a
// point-to-triangle test.  256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h (stack_entries * 64
// words per wave).  A point is one 16-byte load and a record two 16-byte stores per lane.  Lanes past n and lanes whose point is a
// miss before any traversal stay in the wave, inactive.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the triangle test is evaluated as written, and tests/nearest_ref.py mirrors it operation for
// operation.  The box bounds are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "nearest.h"
#include "bvh_walk.h"
#include "closest_point.h"      // closest_on_triangle, box_bound_hc / box_bound_f32

namespace ptd {

// One point per lane through the two-child BVH (bvh_walk.h: the stack depth, the one-word entries).  thr is min(best d2, r2) widened
// (nearest.h): a child is entered iff its bound is at most thr and it is not empty; of two such children the nearer is entered and
// the other pushed.  The boxes only prune: the winner is decided by the triangle test, d2 <= r2, smallest d2, ties to the lowest
// triangle index, whatever order the walk reaches the triangles in.
struct NearestWalk {
    f3 q, qc;
    float r2, abs_term, thr;
    float d2; int slot; uint32_t prim;      // the best candidate so far
    __device__ __forceinline__ NearestWalk(const DeviceScene& sc, const f3& q_, float r2_, float abs_term_)
        : q(q_), qc(mk(q_.x - sc.hspace.cx, q_.y - sc.hspace.cy, q_.z - sc.hspace.cz)), r2(r2_), abs_term(abs_term_), thr(r2_ * kNearRel + abs_term_),
          d2(INFINITY), slot(-1), prim(0xFFFFFFFFu) {}
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        admit_by_bound(box_bound_hc(qa.x, qa.y, qa.z, qc, hs), box_bound_hc(qb.x, qb.y, qb.z, qc, hs), thr, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        admit_by_bound(box_bound_f32(q, a.x, a.y, a.z, a.w, b.x, b.y), box_bound_f32(q, b.z, b.w, c.x, c.y, c.z, c.w), thr, h0, h1, first0);
    }
    __device__ __forceinline__ bool leaf(int slot_, const float4& r0, const float4& r1, const float4& r2_)
    {
        const ClosestPoint p = closest_on_triangle(q, r0, r1, r2_);
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
k_query_nearest(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ points, uint32_t n, float4* __restrict__ out,
                uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    // point i of the array, or an inert one for a lane past n.  ok: the lane has a point and the point can find something — every
    // coordinate finite, max_radius >= 0 and no NaN (include/acgpt.h: "a miss before any traversal")
    f3 q = mk(0.0f);
    float r2 = 0.0f;
    bool ok = false;
    if (i < n) {
        const float4 p = points[i];
        q = mk(p.x, p.y, p.z);
        r2 = p.w * p.w;
        ok = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z) && p.w >= 0.0f;      // false when max_radius is a NaN
    }
    NearestWalk best(sc, q, r2, abs_term);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, COUNT>(sc, st, ok, best, visits);
    if (i >= n) return;
    float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (ok && best.slot >= 0) {
        // the winner's triangle once more: the same function on the same inputs gives the same bits, and the walk carries three
        // registers for its best candidate instead of eight
        const TriRecord* tp = sc.tris + best.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
        const ClosestPoint p = closest_on_triangle(q, r0, r1, r2_);
        const float4 sr = sc.shade[best.slot];
        o0 = make_float4(sqrtf(p.d2), __uint_as_float(best.prim), p.v, p.w);
        o1 = make_float4(p.c.x, p.c.y, p.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
    }
    out[2ull * i] = o0;
    out[2ull * i + 1ull] = o1;
    if (COUNT) visits_out[i] = visits;
}

float nearest_abs_term(const float scene_lo[3], const float scene_hi[3])
{
    const double s = (double)scene_max_abs(scene_lo, scene_hi);
    return round_up_to_float(s * s * (double)kNearAbs);
}

hipError_t launch_query_nearest(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, float4* out,
                                hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_nearest<11, false>, stack_entries, n, stream, sc, stack_entries, abs_term, points, n, out, (uint2*)nullptr);
    return launch_lane_stack(k_query_nearest<0, false>, stack_entries, n, stream, sc, stack_entries, abs_term, points, n, out, (uint2*)nullptr);
}

hipError_t launch_nearest_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, float4* out,
                                 uint2* visits, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_nearest<11, true>, stack_entries, n, stream, sc, stack_entries, abs_term, points, n, out, visits);
    return launch_lane_stack(k_query_nearest<0, true>, stack_entries, n, stream, sc, stack_entries, abs_term, points, n, out, visits);
}

}  // namespace ptd
