// cast_walk.h — the one time-of-impact walk of the cast kernels: sweep.hip, capsule.hip, boxcast.hip and
// tricast.hip (through tricast_device.h) move a shape along a line and ask for the first triangle it meets.  They share everything but
// the shape: the slab test of the shape's centre line against a child box inflated by the shape's extent, the decode of both node
// formats into that test, the policy bvh_walk.h asks for, the any-hit kernel and the frame of the record kernel.  A unit keeps its
// time-of-impact statement, its inflation and cut constants, its extra admission test and its record.
//
// The pruning contract, in one place.  A child is entered iff it is not empty, the centre line meets its inflated box within
// [0, cut] and the unit's extra test (if it has one) does not separate it; cut = Q::cut(min(tmax, best t)) widens the bound so that
// a triangle whose computed time of impact is at most the bound is never behind a pruned box (the derivations are the units': sweep.h,
// capsule.h, boxcast.h, tricast.h).  The boxes only prune: the winner is decided by the leaf rule, t <= tmax, smallest t, ties to the
// lowest triangle index, whatever order the walk reaches the triangles in.
//
// The per-query struct Q of a unit supplies only what differs:
//   f3 qc, inv, infl               the centre of the shape minus the centre of HSpace for FMT 11 (the load is told FMT), the finite
//                                  1-ulp reciprocals of d, the inflation of a child box per world axis
//   float tmax                     the cast's own; the walk takes its tmax as an argument (k_cast_pose walks with a smaller one)
//   float cut(float tb) const      the widened bound for tb = min(tmax, best t), at most FLT_MAX
//   float toi(r0, r1, r2) const    the time of impact with one TriRecord, +inf when there is none
//   static constexpr bool kAdmits  true: bool admit(const f3& c, const f3& g, bool keep) const is a second admission test on the
//                                  child's centre minus qc and its half extent (the capsule's plane, the box's six axes).  keep: the
//                                  child is not empty; the result is keep and the test.  How the two are combined is the unit's
//                                  choice and only a matter of generated code: `keep && test` branches round the test for an empty
//                                  child (the capsule: one register fewer), `keep & test` masks it (the box: no branch)
//   static constexpr bool kTracksCut   true: void cut_moved(float cut) is run whenever the cut is set (the box's swept intervals);
//                                  such a Q is held by value
//   template <int FMT> bool load(casts, i, n, scene_scale, hs)   cast i of the array or an inert one for a lane past n; false: a miss
//                                  before any traversal (the shared kernel bodies alone use it)
// CastWalk<ANY, H> holds H, which is Q or const Q&: whichever keeps the kernel's registers (section 42).
//
// The box arithmetic is outside the bit-exact contract of the units' statements (it only prunes) but is written with explicit fused
// multiply-adds under -ffp-contract=off, so the source fixes its bits and the visit counts with them
// (tests/test_gpu_cast_walk_parity.py).
#pragma once
#include "bvh_walk.h"

#include <cfloat>
#include <type_traits>

namespace ptd {

// Entry and exit of the centre line in one child box, clipped to [0, cut].  c: the box centre minus the shape's centre, e: the
// inflated half extent, per axis, in world units; the products with +-1e30 for a zero direction component give +-inf or 0, never a
// NaN.
__device__ __forceinline__ void cast_line_slab(const f3& c, const f3& e, const f3& inv, float cut, float& tn, float& tf)
{
    const float x0 = (c.x - e.x) * inv.x, x1 = (c.x + e.x) * inv.x;
    const float y0 = (c.y - e.y) * inv.y, y1 = (c.y + e.y) * inv.y;
    const float z0 = (c.z - e.z) * inv.z, z1 = (c.z + e.z) * inv.z;
    tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
    tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), cut));
}

// One child as the tests see it: c the centre minus qc, g the half extent, e = g + infl, in world units.
//
// An empty child is flagged, and its extents are not guarded.  In the fp16 form it is a negative half word and everything stays
// finite.  In the fp32 form lo = +inf and hi = -inf make m, c, g and e NaN or inf; that is harmless because nothing computed from them
// is used: the walk overwrites tn with a NaN, tf is only ever compared with that tn, and a unit's admit() returns false when it is
// handed keep = false.  No compare admits a NaN, and the arithmetic cannot trap.  (boxcast.hip once selected g = 0 for an empty child; its c
// was a NaN all the same, and its axis tests were already masked by the flag.)
struct CastChild { f3 c, g, e; bool empty; };

__device__ __forceinline__ CastChild cast_child_hc(uint32_t px, uint32_t py, uint32_t pz, const f3& qc, const f3& infl, const HSpace& hs)
{
    // world = g * is + centre: c = centre_g * is - qc, g = half_g * is, e = half_g * is + infl, one v_fma_mix_f32 each
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    CastChild b;
    b.c = mk(__builtin_fmaf((float)hx.x, hs.isx, -qc.x), __builtin_fmaf((float)hy.x, hs.isy, -qc.y), __builtin_fmaf((float)hz.x, hs.isz, -qc.z));
    b.g = mk((float)hx.y * hs.isx, (float)hy.y * hs.isy, (float)hz.y * hs.isz);
    b.e = mk(__builtin_fmaf((float)hx.y, hs.isx, infl.x), __builtin_fmaf((float)hy.y, hs.isy, infl.y), __builtin_fmaf((float)hz.y, hs.isz, infl.z));
    b.empty = (float)hx.y < 0.0f;
    return b;
}
__device__ __forceinline__ CastChild cast_child_f32(float lx, float ly, float lz, float hx, float hy, float hz, const f3& qc, const f3& infl)
{
    // the half extent from the rounded centre m, so that [m - g, m + g] holds [lo, hi] to an ulp of the extent
    const f3 m = mk(0.5f * lx + 0.5f * hx, 0.5f * ly + 0.5f * hy, 0.5f * lz + 0.5f * hz);
    CastChild b;
    b.c = m - qc;
    b.g = mk(fmaxf(hx - m.x, m.x - lx), fmaxf(hy - m.y, m.y - ly), fmaxf(hz - m.z, m.z - lz));
    b.e = b.g + infl;
    b.empty = !(lx <= hx);
    return b;
}

// The policy of bvh_walk.h for a cast (its header: the stack depth, the one-word entries).  ANY: leave at the first triangle with
// t <= tmax (slot >= 0 says so).
template <bool ANY, class H>
struct CastWalk {
    using Q = std::remove_cv_t<std::remove_reference_t<H>>;
    H q;
    float tmax, cut;
    float t; int slot; uint32_t prim;      // the best candidate so far
    __device__ __forceinline__ CastWalk(H q_, float tmax_) : q(q_), tmax(tmax_), t(INFINITY), slot(-1), prim(0xFFFFFFFFu) { set_cut(tmax_); }
    __device__ __forceinline__ void set_cut(float tb)
    {
        cut = q.cut(tb);
        if constexpr (Q::kTracksCut) q.cut_moved(cut);
    }
    // tn = NaN for an empty child or one the unit's own test separates, which no compare admits (an inflated empty box would be hit)
    __device__ __forceinline__ void child(const CastChild& b, float& tn, float& tf) const
    {
        cast_line_slab(b.c, b.e, q.inv, cut, tn, tf);
        bool keep = !b.empty;
        if constexpr (Q::kAdmits) keep = q.admit(b.c, b.g, keep);
        if (!keep) tn = __builtin_nanf("");
    }
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        child(cast_child_hc(qa.x, qa.y, qa.z, q.qc, q.infl, hs), n0, f0);
        child(cast_child_hc(qb.x, qb.y, qb.z, q.qc, q.infl, hs), n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        child(cast_child_f32(a.x, a.y, a.z, a.w, b.x, b.y, q.qc, q.infl), n0, f0);
        child(cast_child_f32(b.z, b.w, c.x, c.y, c.z, c.w, q.qc, q.infl), n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ bool leaf(int slot_, const float4& r0, const float4& r1, const float4& r2)
    {
        const float t_ = q.toi(r0, r1, r2);
        const uint32_t prim_ = __float_as_uint(r2.y);
        if (ANY) {
            if (t_ <= tmax) { slot = slot_; return true; }
        } else if (t_ <= tmax && (t_ < t || (t_ == t && prim_ < prim))) {
            t = t_; slot = slot_; prim = prim_;
            set_cut(t_);
        }
        return false;
    }
};

// The body of a unit's any-hit kernel: one byte per cast.  256-lane workgroups over a one-dimensional grid, the lane stack of
// query_launch.h; lanes past n and lanes whose cast is a miss before any traversal stay in the wave, inactive.
template <int FMT, class Q, class H>
__device__ __forceinline__ void cast_any_body(const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n,
                                              uint8_t* __restrict__ blocked)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    Q q;
    const bool ok = q.template load<FMT>(casts, i, n, scene_scale, sc.hspace);
    CastWalk<true, H> best(q, q.tmax);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, best, visits);
    if (i >= n) return;
    blocked[i] = (ok && best.slot >= 0) ? (uint8_t)1 : (uint8_t)0;
}

// The frame of a unit's record kernel.  write(i, q, found, best) stores record i: the unit's record of the winner (best.t, best.prim,
// best.slot) when found, its miss record otherwise.  COUNT also writes how many inner nodes the lane visited and how many triangles it
// tested.
template <int FMT, bool COUNT, class Q, class H, class W>
__device__ __forceinline__ void cast_record_body(const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n,
                                                 uint2* __restrict__ visits_out, W write)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    Q q;
    const bool ok = q.template load<FMT>(casts, i, n, scene_scale, sc.hspace);
    CastWalk<false, H> best(q, q.tmax);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, COUNT>(sc, st, ok, best, visits);
    if (i >= n) return;
    write(i, q, ok && best.slot >= 0, best);
    if (COUNT) visits_out[i] = visits;
}

// The launch the units' kernels share: (scene, stack, scale, casts, n) and then the kernel's own outputs.
template <typename K, typename... A>
static hipError_t launch_cast(K kernel, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, hipStream_t stream, A... outputs)
{
    return launch_lane_stack(kernel, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, outputs...);
}

}  // namespace ptd
