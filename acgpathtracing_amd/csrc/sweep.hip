// sweep.hip — the kernels behind pt_query_sweep and pt_query_sweep_any (include/acgpt.h).
//
//   k_query_sweep<FMT, COUNT>   one swept sphere per lane from a device array: the triangle with the smallest time of impact within
//                               [0, tmax], then the record (t, triangle, weights of v1 and v2 and the closest point at the centre of
//                               impact, material).  COUNT also writes how many inner nodes the lane visited and how many triangles it
//                               tested (the test hook's instantiation).
//   k_query_sweep_any<FMT>      one byte per sweep; a lane leaves the walk at its first triangle with a time of impact within [0, tmax].
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk, the any-hit
// kernel and the record kernel's frame are cast_walk.h's.  This unit's own: the leaf statement sweep_triangle; the line of the
// sphere's centre, each child box inflated by the radius (sweep.h: R, a little more), the cut of sweep.h; no extra admission test;
// the record.  A sweep is one 32-byte load and a record two 16-byte stores per lane.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the time of impact is evaluated as written, and tests/sweep_ref.py mirrors it operation for operation.
#include "sweep.h"
#include "cast_walk.h"
#include "closest_point.h"      // closest_on_triangle: the start-overlap test and the record's (u, v, c) are defined as pt_query_nearest's results
#include "sweep_device.h"       // sweep_vertex, sweep_edge, sweep_face: shared with capsule.hip

namespace ptd {

// The time of impact of the sphere {o + t d, r} with the triangle {v0, v0 + e1, v0 + e2}: 0 on a start overlap, else the smallest
// candidate of the eight features, +inf when there is none.
__device__ __forceinline__ float sweep_triangle(const f3& o, const f3& d, float dd, float r, float rr, const f3& v0, const f3& e1, const f3& e2)
{
    float t = INFINITY;
    const f3 m0 = o - v0;
    const f3 p1 = v0 + e1, p2 = v0 + e2;
    const f3 m1 = o - p1, m2 = o - p2;
    sweep_vertex(m0, d, dd, rr, t);
    sweep_vertex(m1, d, dd, rr, t);
    sweep_vertex(m2, d, dd, rr, t);
    sweep_edge(m0, e1, d, rr, t);
    sweep_edge(m0, e2, d, rr, t);
    sweep_edge(m1, e2 - e1, d, rr, t);
    sweep_face(m0, e1, e2, d, r, t);
    const ClosestPoint p = closest_on_triangle(o, v0, e1, e2);
    if (p.d2 <= rr) t = 0.0f;
    return t;
}

// What a lane keeps of its sweep: cast_walk.h's per-query struct.
struct SweepRay {
    static constexpr bool kAdmits = false, kTracksCut = false;
    f3 o, d;
    float dd, r, rr, tmax;
    f3 inv;             // finite 1-ulp reciprocals of d
    f3 qc;              // o, minus the centre of HSpace for FMT 11
    f3 infl;            // R of sweep.h on every axis
    float abs_t;        // the absolute term of the far cut, in units of t

    template <int FMT>
    __device__ __forceinline__ void setup(const f3& o_, const f3& d_, float r_, float tmax_, float scene_scale, const HSpace& hs)
    {
        o = o_; d = d_; r = r_; tmax = tmax_;
        dd = dot(d, d);
        rr = r * r;
        inv = mk(finite_rcp(d.x), finite_rcp(d.y), finite_rcp(d.z));
        qc = FMT == 11 ? mk(o.x - hs.cx, o.y - hs.cy, o.z - hs.cz) : o;
        const float big = scene_scale + fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
        infl = mk(__builtin_fmaf(r, kSweepBoxRel, big * kSweepBoxAbs));
        const float len = sqrtf(dd);
        abs_t = len > 0.0f ? __builtin_fmaf(big, kSweepLinT, sqrtf(r * (r + big)) * kSweepSqrtT) / len : INFINITY;
    }
    // sweep i of the array, or an inert one for a lane past n.  Returns whether the lane has a sweep that can touch something: o and
    // d finite, radius finite and >= 0, tmax >= 0 and no NaN (include/acgpt.h: "a miss before any traversal")
    template <int FMT>
    __device__ __forceinline__ bool load(const float4* __restrict__ sweeps, uint32_t i, uint32_t n, float scene_scale, const HSpace& hs)
    {
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n) { a = sweeps[2ull * i]; b = sweeps[2ull * i + 1ull]; }
        const bool ok = i < n && __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) && __builtin_isfinite(a.w) &&
                        __builtin_isfinite(b.x) && __builtin_isfinite(b.y) && __builtin_isfinite(b.z) && b.z >= 0.0f && b.w >= 0.0f;
        // tmax = +inf is the largest finite t: a time of impact of +inf stands for "no candidate"
        setup<FMT>(mk(a.x, a.y, a.z), mk(a.w, b.x, b.y), ok ? b.z : 0.0f, ok ? fminf(b.w, FLT_MAX) : 0.0f, scene_scale, hs);
        return ok;
    }
    // cut of sweep.h for tb = min(tmax, best t); at most FLT_MAX, so that a box the line never reaches (entry +inf) is not entered
    __device__ __forceinline__ float cut(float tb) const { return fminf(__builtin_fmaf(tb, kSweepRelT, abs_t), FLT_MAX); }
    __device__ __forceinline__ float toi(const float4& r0, const float4& r1, const float4& r2) const
    {
        return sweep_triangle(o, d, dd, r, rr, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
    }
};

template <int FMT, bool COUNT>
__global__ void __launch_bounds__(256)
k_query_sweep(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ sweeps, uint32_t n, float4* __restrict__ out,
              uint2* __restrict__ visits_out)
{
    cast_record_body<FMT, COUNT, SweepRay, SweepRay>(sc, stack_entries, scene_scale, sweeps, n, visits_out, [&](uint32_t i, const SweepRay& s, bool found, const auto& best) {
        float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
        if (found) {
            // closest_on_triangle once, on the winner at the centre of impact: the walk carries three registers for its best candidate
            const TriRecord* tp = sc.tris + best.slot;
            const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
            const f3 centre = mk(s.o.x + s.d.x * best.t, s.o.y + s.d.y * best.t, s.o.z + s.d.z * best.t);
            const ClosestPoint p = closest_on_triangle(centre, r0, r1, r2);
            const float4 sr = sc.shade[best.slot];
            o0 = make_float4(best.t, __uint_as_float(best.prim), p.v, p.w);
            o1 = make_float4(p.c.x, p.c.y, p.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
        }
        out[2ull * i] = o0;
        out[2ull * i + 1ull] = o1;
    });
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_sweep_any(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ sweeps, uint32_t n, uint8_t* __restrict__ blocked)
{
    cast_any_body<FMT, SweepRay, SweepRay>(sc, stack_entries, scene_scale, sweeps, n, blocked);
}

hipError_t launch_query_sweep(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n, float4* out,
                              hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) { return launch_cast(k_query_sweep<decltype(F)::value, false>, sc, stack_entries, scene_scale, sweeps, n, stream, out, (uint2*)nullptr); });
}

hipError_t launch_query_sweep_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n,
                                  uint8_t* blocked, hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) { return launch_cast(k_query_sweep_any<decltype(F)::value>, sc, stack_entries, scene_scale, sweeps, n, stream, blocked); });
}

hipError_t launch_sweep_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n, float4* out,
                               uint2* visits, hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) { return launch_cast(k_query_sweep<decltype(F)::value, true>, sc, stack_entries, scene_scale, sweeps, n, stream, out, visits); });
}

}  // namespace ptd
