// sweep.hip — the kernels behind pt_query_sweep and pt_query_sweep_any (include/acgpt.h).
//
//   k_query_sweep<FMT, COUNT>   one swept sphere per lane from a device array: the triangle with the smallest time of impact within
//                               [0, tmax], then the record (t, triangle, weights of v1 and v2 and the closest point at the centre of
//                               impact, material).  COUNT also writes how many inner nodes the lane visited and how many triangles it
//                               tested (the test hook's instantiation).
//   k_query_sweep_any<FMT>      one byte per sweep; a lane leaves the walk at its first triangle with a time of impact within [0, tmax].
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk is a slab test of
// the centre line against each child box inflated by the radius (sweep.h: by a little more), clipped to [0, min(tmax, best t)] widened
// (sweep.h), nearer child first.  256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h (stack_entries * 64
// words per wave).  A sweep is one 32-byte load and a record two 16-byte stores per lane.  Lanes past n and lanes whose sweep is a
// miss before any traversal stay in the wave, inactive.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the time of impact is evaluated as written, and tests/sweep_ref.py mirrors it operation for operation.
// The box test is outside that contract (it only prunes) and uses explicit fused multiply-adds.
#include "sweep.h"
#include "bvh_walk.h"
#include "closest_point.h"      // closest_on_triangle: the start-overlap test and the record's (u, v, c) are defined as pt_query_nearest's results
#include "sweep_device.h"       // sweep_vertex, sweep_edge, sweep_face: shared with capsule.hip

#include <cfloat>

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

// What a lane keeps of its sweep for the walk.
struct SweepRay {
    f3 o, d;
    float dd, r, rr, tmax;
    f3 inv;             // finite 1-ulp reciprocals of d
    f3 qc;              // o - centre of HSpace (FMT 11)
    float infl;         // R of sweep.h
    float abs_t;        // the absolute term of the far cut, in units of t
};

__device__ __forceinline__ SweepRay sweep_setup(const f3& o, const f3& d, float r, float tmax, float scene_scale, const HSpace& hs)
{
    SweepRay s;
    s.o = o; s.d = d; s.r = r; s.tmax = tmax;
    s.dd = dot(d, d);
    s.rr = r * r;
    s.inv = mk(finite_rcp(d.x), finite_rcp(d.y), finite_rcp(d.z));
    s.qc = mk(o.x - hs.cx, o.y - hs.cy, o.z - hs.cz);
    const float big = scene_scale + fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    s.infl = __builtin_fmaf(r, kSweepBoxRel, big * kSweepBoxAbs);
    const float len = sqrtf(s.dd);
    s.abs_t = len > 0.0f ? __builtin_fmaf(big, kSweepLinT, sqrtf(r * (r + big)) * kSweepSqrtT) / len : INFINITY;
    return s;
}
// cut of sweep.h for tb = min(tmax, best t); at most FLT_MAX, so that a box the line never reaches (entry +inf) is not entered
__device__ __forceinline__ float sweep_cut(const SweepRay& s, float tb) { return fminf(__builtin_fmaf(tb, kSweepRelT, s.abs_t), FLT_MAX); }

// Entry and exit of the centre line in one child box inflated by s.infl, clipped to [0, cut]; tn = NaN for an empty child, which no
// compare admits (an inflated empty box would be hit).  c: the box centre minus o, e: the inflated half extent, per axis, in world
// units; the products with +-1e30 for a zero direction component give +-inf or 0, never a NaN.
__device__ __forceinline__ void sweep_slab(const f3& c, const f3& e, const f3& inv, float cut, bool empty, float& tn, float& tf)
{
    const float x0 = (c.x - e.x) * inv.x, x1 = (c.x + e.x) * inv.x;
    const float y0 = (c.y - e.y) * inv.y, y1 = (c.y + e.y) * inv.y;
    const float z0 = (c.z - e.z) * inv.z, z1 = (c.z + e.z) * inv.z;
    tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
    tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), cut));
    if (empty) tn = __builtin_nanf("");
}
__device__ __forceinline__ void sweep_slab_hc(uint32_t px, uint32_t py, uint32_t pz, const SweepRay& s, const HSpace& hs, float cut, float& tn, float& tf)
{
    // world = g * is + centre: c = centre_g * is - qc, e = half_g * is + R, one v_fma_mix_f32 each
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const f3 c = mk(__builtin_fmaf((float)hx.x, hs.isx, -s.qc.x), __builtin_fmaf((float)hy.x, hs.isy, -s.qc.y), __builtin_fmaf((float)hz.x, hs.isz, -s.qc.z));
    const f3 e = mk(__builtin_fmaf((float)hx.y, hs.isx, s.infl), __builtin_fmaf((float)hy.y, hs.isy, s.infl), __builtin_fmaf((float)hz.y, hs.isz, s.infl));
    sweep_slab(c, e, s.inv, cut, (float)hx.y < 0.0f, tn, tf);
}
__device__ __forceinline__ void sweep_slab_f32(float lx, float ly, float lz, float hx, float hy, float hz, const SweepRay& s, float cut, float& tn, float& tf)
{
    // the half extent from the rounded centre m, so that [m - e, m + e] holds [lo, hi] to an ulp of the extent
    const f3 m = mk(0.5f * lx + 0.5f * hx, 0.5f * ly + 0.5f * hy, 0.5f * lz + 0.5f * hz);
    const f3 c = m - s.o;
    const f3 e = mk(fmaxf(hx - m.x, m.x - lx) + s.infl, fmaxf(hy - m.y, m.y - ly) + s.infl, fmaxf(hz - m.z, m.z - lz) + s.infl);
    sweep_slab(c, e, s.inv, cut, !(lx <= hx), tn, tf);
}

// One sweep per lane through the two-child BVH (bvh_walk.h: the stack depth, the one-word entries).  The boxes only prune: the winner
// is decided by the leaf test, t <= tmax, smallest t, ties to the lowest triangle index, whatever order the walk reaches the triangles
// in.  ANY: leave at the first triangle with t <= tmax (slot >= 0 says so).
template <bool ANY>
struct SweepWalk {
    SweepRay s;
    float cut;
    float t; int slot; uint32_t prim;      // the best candidate so far
    __device__ __forceinline__ explicit SweepWalk(const SweepRay& s_) : s(s_), cut(sweep_cut(s_, s_.tmax)), t(INFINITY), slot(-1), prim(0xFFFFFFFFu) {}
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        sweep_slab_hc(qa.x, qa.y, qa.z, s, hs, cut, n0, f0);
        sweep_slab_hc(qb.x, qb.y, qb.z, s, hs, cut, n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        sweep_slab_f32(a.x, a.y, a.z, a.w, b.x, b.y, s, cut, n0, f0);
        sweep_slab_f32(b.z, b.w, c.x, c.y, c.z, c.w, s, cut, n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ bool leaf(int slot_, const float4& r0, const float4& r1, const float4& r2)
    {
        const float t_ = sweep_triangle(s.o, s.d, s.dd, s.r, s.rr, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
        const uint32_t prim_ = __float_as_uint(r2.y);
        if (ANY) {
            if (t_ <= s.tmax) { slot = slot_; return true; }
        } else if (t_ <= s.tmax && (t_ < t || (t_ == t && prim_ < prim))) {
            t = t_; slot = slot_; prim = prim_;
            cut = sweep_cut(s, t_);
        }
        return false;
    }
};

// sweep i of the array, or an inert one for a lane past n.  Returns whether the lane has a sweep that can touch something: o and d
// finite, radius finite and >= 0, tmax >= 0 and no NaN (include/acgpt.h: "a miss before any traversal")
__device__ __forceinline__ bool sweep_load(const float4* __restrict__ sweeps, uint32_t i, uint32_t n, float scene_scale, const HSpace& hs, SweepRay& s)
{
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < n) { a = sweeps[2ull * i]; b = sweeps[2ull * i + 1ull]; }
    const bool ok = i < n && __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) && __builtin_isfinite(a.w) &&
                    __builtin_isfinite(b.x) && __builtin_isfinite(b.y) && __builtin_isfinite(b.z) && b.z >= 0.0f && b.w >= 0.0f;
    // tmax = +inf is the largest finite t: a time of impact of +inf stands for "no candidate"
    s = sweep_setup(mk(a.x, a.y, a.z), mk(a.w, b.x, b.y), ok ? b.z : 0.0f, ok ? fminf(b.w, FLT_MAX) : 0.0f, scene_scale, hs);
    return ok;
}

template <int FMT, bool COUNT>
__global__ void __launch_bounds__(256)
k_query_sweep(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ sweeps, uint32_t n, float4* __restrict__ out,
              uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    SweepRay s;
    const bool ok = sweep_load(sweeps, i, n, scene_scale, sc.hspace, s);
    SweepWalk<false> best(s);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, COUNT>(sc, st, ok, best, visits);
    if (i >= n) return;
    float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (ok && best.slot >= 0) {
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
    if (COUNT) visits_out[i] = visits;
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_sweep_any(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ sweeps, uint32_t n, uint8_t* __restrict__ blocked)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    SweepRay s;
    const bool ok = sweep_load(sweeps, i, n, scene_scale, sc.hspace, s);
    SweepWalk<true> best(s);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, best, visits);
    if (i >= n) return;
    blocked[i] = (ok && best.slot >= 0) ? (uint8_t)1 : (uint8_t)0;
}

float sweep_scene_scale(const float scene_lo[3], const float scene_hi[3]) { return scene_max_abs(scene_lo, scene_hi); }

hipError_t launch_query_sweep(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n, float4* out,
                              hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_sweep<11, false>, stack_entries, n, stream, sc, stack_entries, scene_scale, sweeps, n, out, (uint2*)nullptr);
    return launch_lane_stack(k_query_sweep<0, false>, stack_entries, n, stream, sc, stack_entries, scene_scale, sweeps, n, out, (uint2*)nullptr);
}

hipError_t launch_query_sweep_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n,
                                  uint8_t* blocked, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_sweep_any<11>, stack_entries, n, stream, sc, stack_entries, scene_scale, sweeps, n, blocked);
    return launch_lane_stack(k_query_sweep_any<0>, stack_entries, n, stream, sc, stack_entries, scene_scale, sweeps, n, blocked);
}

hipError_t launch_sweep_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* sweeps, uint32_t n, float4* out,
                               uint2* visits, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_sweep<11, true>, stack_entries, n, stream, sc, stack_entries, scene_scale, sweeps, n, out, visits);
    return launch_lane_stack(k_query_sweep<0, true>, stack_entries, n, stream, sc, stack_entries, scene_scale, sweeps, n, out, visits);
}

}  // namespace ptd
