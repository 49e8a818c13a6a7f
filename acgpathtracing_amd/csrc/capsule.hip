// capsule.hip — the kernels behind pt_query_capsule_cast and pt_query_capsule_cast_any (include/acgpt.h).
//
//   k_query_capsule<FMT, COUNT, PLANE>   one swept capsule per lane from a device array: the triangle with the smallest time of impact
//                                        within [0, tmax], then the record (t, triangle, parameter on the axis, feature and closest
//                                        point of the axis at impact, material).  COUNT also writes how many inner nodes the lane
//                                        visited and how many triangles it tested (the test hook's instantiations); PLANE = false is
//                                        the walk without the plane axis, the other arm of its measurement.
//   k_query_capsule_any<FMT>             one byte per cast; a lane leaves the walk at its first triangle with a time of impact within
//                                        [0, tmax].
// (The names leave out "cast": tests/test_tricast_host.py counts the kernels whose name contains it.)
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk is sweep.hip's
// slab test with the line of the axis' midpoint against each child box inflated per axis by half the axis and the radius (capsule.h:
// by a little more), clipped to [0, min(tmax, best t)] widened, and the separation of the box from the plane of the swept axis
// (capsule.h), nearer child first.  256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h (stack_entries *
// 64 words per wave).  A cast is three 16-byte loads and a record two 16-byte stores per lane.  Lanes past n and lanes whose cast is a
// miss before any traversal stay in the wave, inactive.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the time of impact is evaluated as written, and tests/capsule_ref.py mirrors it operation for
// operation.  The box tests are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "capsule.h"
#include "bvh_walk.h"
#include "sweep_device.h"        // sweep_vertex, sweep_edge, sweep_face: pt_query_sweep's three feature forms
#include "segment_device.h"      // segment_triangle: the start-overlap test and the record's (s, feature, c) are pt_query_segments' results

#include <cfloat>

namespace ptd {

// Closes one sub-test before the next starts (segment_device.h's seg_take): the twenty-two are never live together.  What two of
// them share (it depends on E and d alone) is still computed once.
__device__ __forceinline__ void cap_close(float& t)
{
    asm volatile("" : "+v"(t));
    __builtin_amdgcn_sched_barrier(0);
}

// The face form of include/acgpt.h on the parallelogram {A - a + u E + v a}: m = p1 - A, E in the place of e1 and a in the place of
// e2, and the candidate rule of a parallelogram.
__device__ __forceinline__ void capsule_side_face(const f3& m, const f3& E, const f3& a, const f3& d, float r, float& t)
{
    const f3 n = cross(E, a);
    const float nn = dot(n, n), s0 = dot(n, m);
    const float sr = s0 >= 0.0f ? r : -r;
    const float tf = (sr * sqrtf(nn) - s0) / dot(n, d);
    const f3 w = mk(m.x + d.x * tf, m.y + d.y * tf, m.z + d.z * tf);
    const float u = dot(cross(w, a), n) / nn, v = dot(cross(E, w), n) / nn;
    if (tf >= 0.0f && u >= 0.0f && u <= 1.0f && v >= 0.0f && v <= 1.0f && tf < t) t = tf;
}

// The time of impact of the capsule {p0 + t d, p1 + t d, r} with the triangle {v0, v0 + e1, v0 + e2}: 0 on a start overlap, else the
// smallest candidate of the twenty-one features of the prism triangle + (-[0, a]) offset by r, +inf when there is none.  a = p1 - p0,
// aa = dot(a, a); p1 is the record's, not p0 + a.
__device__ __forceinline__ float capsule_triangle(const f3& p0, const f3& p1, const f3& a, float aa, const f3& d, float dd, float r, float rr, const f3& v0,
                                                  const f3& e1, const f3& e2)
{
    float t = INFINITY;
    const f3 q1 = v0 + e1, q2 = v0 + e2;
    const f3 e3 = e2 - e1;
    {
        const f3 m0 = p0 - v0, m1 = p0 - q1, m2 = p0 - q2;
        sweep_vertex(m0, d, dd, rr, t); cap_close(t);
        sweep_vertex(m1, d, dd, rr, t); cap_close(t);
        sweep_vertex(m2, d, dd, rr, t); cap_close(t);
        sweep_edge(m0, e1, d, rr, t); cap_close(t);
        sweep_edge(m0, e2, d, rr, t); cap_close(t);
        sweep_edge(m1, e3, d, rr, t); cap_close(t);
        sweep_face(m0, e1, e2, d, r, t); cap_close(t);
    }
    {
        const f3 m0 = p1 - v0, m1 = p1 - q1, m2 = p1 - q2;
        sweep_vertex(m0, d, dd, rr, t); cap_close(t);
        sweep_vertex(m1, d, dd, rr, t); cap_close(t);
        sweep_vertex(m2, d, dd, rr, t); cap_close(t);
        sweep_edge(m0, e1, d, rr, t); cap_close(t);
        sweep_edge(m0, e2, d, rr, t); cap_close(t);
        sweep_edge(m1, e3, d, rr, t); cap_close(t);
        sweep_face(m0, e1, e2, d, r, t); cap_close(t);
        // the three axis edges {P - a, a} and the three side faces {A - a, E, a}
        sweep_edge(m0, a, d, rr, t); cap_close(t);
        sweep_edge(m1, a, d, rr, t); cap_close(t);
        sweep_edge(m2, a, d, rr, t); cap_close(t);
        capsule_side_face(m0, e1, a, d, r, t); cap_close(t);
        capsule_side_face(m0, e2, a, d, r, t); cap_close(t);
        capsule_side_face(m1, e3, a, d, r, t); cap_close(t);
    }
    const SegPoint p = segment_triangle<false>(p0, p1, a, aa, v0, e1, e2);
    if (p.d2 <= rr) t = 0.0f;
    return t;
}

// What a lane keeps of its cast for the walk.
struct CapsuleRay {
    f3 p0, p1, a, d;
    float aa, dd, r, rr, tmax;
    f3 inv;             // finite 1-ulp reciprocals of d
    f3 qc;              // the axis' midpoint, minus the centre of HSpace for FMT 11
    f3 infl;            // |a_k| / 2 + R of capsule.h
    float abs_t;        // the absolute term of the far cut, in units of t
    f3 w;               // the unit normal of the swept axis' plane, or 0
    float plane_r;      // the right-hand side of the plane test less the box's own extent
};

template <int FMT>
__device__ __forceinline__ CapsuleRay capsule_setup(const f3& p0, const f3& p1, const f3& d, float r, float tmax, float scene_scale, const HSpace& hs)
{
    CapsuleRay s;
    s.p0 = p0; s.p1 = p1; s.d = d; s.r = r; s.tmax = tmax;
    s.a = p1 - p0;
    s.aa = dot(s.a, s.a);
    s.dd = dot(d, d);
    s.rr = r * r;
    s.inv = mk(finite_rcp(d.x), finite_rcp(d.y), finite_rcp(d.z));
    s.qc = mk(__builtin_fmaf(0.5f, s.a.x, p0.x), __builtin_fmaf(0.5f, s.a.y, p0.y), __builtin_fmaf(0.5f, s.a.z, p0.z));
    if (FMT == 11) s.qc = mk(s.qc.x - hs.cx, s.qc.y - hs.cy, s.qc.z - hs.cz);
    const float big = scene_scale + fmaxf(fmaxf(fmaxf(fabsf(p0.x), fabsf(p0.y)), fmaxf(fabsf(p0.z), fabsf(p1.x))), fmaxf(fabsf(p1.y), fabsf(p1.z)));
    const float R = __builtin_fmaf(r, kCapBoxRel, big * kCapBoxAbs);
    s.infl = mk(__builtin_fmaf(0.5f, fabsf(s.a.x), R), __builtin_fmaf(0.5f, fabsf(s.a.y), R), __builtin_fmaf(0.5f, fabsf(s.a.z), R));
    const float len = sqrtf(s.dd);
    s.abs_t = len > 0.0f ? __builtin_fmaf(big, kCapLinT, sqrtf(r * (r + big)) * kCapSqrtT) / len : INFINITY;
    // the plane of the swept axis: w = normalize(a x d) as computed, and what the computed w lets through (capsule.h)
    const f3 n = cross(s.a, d);
    const float l2 = dot(n, n);
    const float il = (l2 > 1e-30f && l2 < 1e30f && len > 0.0f) ? __builtin_amdgcn_rsqf(l2) : 0.0f;
    s.w = mk(n.x * il, n.y * il, n.z * il);
    const float wa = fabsf(dot(s.w, s.a)), wd = fabsf(dot(s.w, d));
    const float reach = __builtin_fmaf(4.0f, big, 2.0f * r);      // D of capsule.h
    const float tilt = len > 0.0f ? reach * wd / len : 0.0f;
    s.plane_r = __builtin_fmaf(R, kCapPlaneRel, __builtin_fmaf(0.5f, wa, __builtin_fmaf(big, kCapPlaneAbs, tilt)));
    return s;
}
// cut of capsule.h for tb = min(tmax, best t); at most FLT_MAX, so that a box the line never reaches (entry +inf) is not entered
__device__ __forceinline__ float capsule_cut(const CapsuleRay& s, float tb) { return fminf(__builtin_fmaf(tb, kCapRelT, s.abs_t), FLT_MAX); }

// One child: entry and exit of the midpoint's line in the box inflated by s.infl, clipped to [0, cut], and (PLANE) whether the box
// reaches the plane of the swept axis; tn = NaN for an empty child or a box off the plane, which no compare admits.  c: the box
// centre minus the midpoint, h: the box's half extent, per axis, in world units; the products with +-1e30 for a zero direction
// component give +-inf or 0, never a NaN.
template <bool PLANE>
__device__ __forceinline__ void capsule_child(const f3& c, const f3& h, const f3& e, const CapsuleRay& s, float cut, bool empty, float& tn, float& tf)
{
    const float x0 = (c.x - e.x) * s.inv.x, x1 = (c.x + e.x) * s.inv.x;
    const float y0 = (c.y - e.y) * s.inv.y, y1 = (c.y + e.y) * s.inv.y;
    const float z0 = (c.z - e.z) * s.inv.z, z1 = (c.z + e.z) * s.inv.z;
    tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
    tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), cut));
    bool off = empty;
    if (PLANE) {
        const float pd = fabsf(__builtin_fmaf(s.w.x, c.x, __builtin_fmaf(s.w.y, c.y, s.w.z * c.z)));
        const float pe = __builtin_fmaf(fabsf(s.w.x), h.x, __builtin_fmaf(fabsf(s.w.y), h.y, fabsf(s.w.z) * h.z));
        off = off || !(pd - pe <= s.plane_r);
    }
    if (off) tn = __builtin_nanf("");
}
template <bool PLANE>
__device__ __forceinline__ void capsule_child_hc(uint32_t px, uint32_t py, uint32_t pz, const CapsuleRay& s, const HSpace& hs, float cut, float& tn, float& tf)
{
    // world = g * is + centre: c = centre_g * is - qc, h = half_g * is, e = half_g * is + infl, one v_fma_mix_f32 each
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const f3 c = mk(__builtin_fmaf((float)hx.x, hs.isx, -s.qc.x), __builtin_fmaf((float)hy.x, hs.isy, -s.qc.y), __builtin_fmaf((float)hz.x, hs.isz, -s.qc.z));
    const f3 h = mk((float)hx.y * hs.isx, (float)hy.y * hs.isy, (float)hz.y * hs.isz);
    const f3 e = mk(__builtin_fmaf((float)hx.y, hs.isx, s.infl.x), __builtin_fmaf((float)hy.y, hs.isy, s.infl.y), __builtin_fmaf((float)hz.y, hs.isz, s.infl.z));
    capsule_child<PLANE>(c, h, e, s, cut, (float)hx.y < 0.0f, tn, tf);
}
template <bool PLANE>
__device__ __forceinline__ void capsule_child_f32(float lx, float ly, float lz, float hx, float hy, float hz, const CapsuleRay& s, float cut, float& tn, float& tf)
{
    // the half extent from the rounded centre m, so that [m - h, m + h] holds [lo, hi] to an ulp of the extent
    const f3 m = mk(0.5f * lx + 0.5f * hx, 0.5f * ly + 0.5f * hy, 0.5f * lz + 0.5f * hz);
    const f3 c = m - s.qc;
    const f3 h = mk(fmaxf(hx - m.x, m.x - lx), fmaxf(hy - m.y, m.y - ly), fmaxf(hz - m.z, m.z - lz));
    capsule_child<PLANE>(c, h, h + s.infl, s, cut, !(lx <= hx), tn, tf);
}

// One cast per lane through the two-child BVH (bvh_walk.h: the stack depth, the one-word entries).  The boxes only prune: the winner
// is decided by the leaf test, t <= tmax, smallest t, ties to the lowest triangle index, whatever order the walk reaches the triangles
// in.  ANY: leave at the first triangle with t <= tmax (slot >= 0 says so).
template <bool ANY, bool PLANE>
struct CapsuleWalk {
    CapsuleRay s;
    float cut;
    float t; int slot; uint32_t prim;      // the best candidate so far
    __device__ __forceinline__ explicit CapsuleWalk(const CapsuleRay& s_) : s(s_), cut(capsule_cut(s_, s_.tmax)), t(INFINITY), slot(-1), prim(0xFFFFFFFFu) {}
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        capsule_child_hc<PLANE>(qa.x, qa.y, qa.z, s, hs, cut, n0, f0);
        capsule_child_hc<PLANE>(qb.x, qb.y, qb.z, s, hs, cut, n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        capsule_child_f32<PLANE>(a.x, a.y, a.z, a.w, b.x, b.y, s, cut, n0, f0);
        capsule_child_f32<PLANE>(b.z, b.w, c.x, c.y, c.z, c.w, s, cut, n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ bool leaf(int slot_, const float4& r0, const float4& r1, const float4& r2)
    {
        const float t_ = capsule_triangle(s.p0, s.p1, s.a, s.aa, s.d, s.dd, s.r, s.rr, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
        const uint32_t prim_ = __float_as_uint(r2.y);
        if (ANY) {
            if (t_ <= s.tmax) { slot = slot_; return true; }
        } else if (t_ <= s.tmax && (t_ < t || (t_ == t && prim_ < prim))) {
            t = t_; slot = slot_; prim = prim_;
            cut = capsule_cut(s, t_);
        }
        return false;
    }
};

// cast i of the array, or an inert one for a lane past n.  Returns whether the lane has a cast that can touch something: p0, p1,
// p1 - p0 and d finite, radius finite and >= 0, tmax >= 0 and no NaN (include/acgpt.h: "a miss before any traversal").  The twelfth
// float is loaded with its float4 and never used.
template <int FMT>
__device__ __forceinline__ bool capsule_load(const float4* __restrict__ casts, uint32_t i, uint32_t n, float scene_scale, const HSpace& hs, CapsuleRay& s)
{
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, g2 = g0;
    if (i < n) { g0 = casts[3ull * i]; g1 = casts[3ull * i + 1ull]; g2 = casts[3ull * i + 2ull]; }
    const float ax = g1.x - g0.x, ay = g1.y - g0.y, az = g1.z - g0.z;
    const bool ok = i < n && __builtin_isfinite(g0.x) && __builtin_isfinite(g0.y) && __builtin_isfinite(g0.z) && __builtin_isfinite(g0.w) &&
                    __builtin_isfinite(g1.x) && __builtin_isfinite(g1.y) && __builtin_isfinite(g1.z) && __builtin_isfinite(ax) && __builtin_isfinite(ay) &&
                    __builtin_isfinite(az) && __builtin_isfinite(g2.x) && __builtin_isfinite(g2.y) && __builtin_isfinite(g2.z) && g0.w >= 0.0f && g1.w >= 0.0f;
    if (!ok) { g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); g1 = g0; g2 = g0; }
    // tmax = +inf is the largest finite t: a time of impact of +inf stands for "no candidate"
    s = capsule_setup<FMT>(mk(g0.x, g0.y, g0.z), mk(g1.x, g1.y, g1.z), mk(g2.x, g2.y, g2.z), g0.w, fminf(g1.w, FLT_MAX), scene_scale, hs);
    return ok;
}

template <int FMT, bool COUNT, bool PLANE>
__global__ void __launch_bounds__(256)
k_query_capsule(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, float4* __restrict__ out,
                     uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    CapsuleRay s;
    const bool ok = capsule_load<FMT>(casts, i, n, scene_scale, sc.hspace, s);
    CapsuleWalk<false, PLANE> best(s);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, COUNT>(sc, st, ok, best, visits);
    if (i >= n) return;
    float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (ok && best.slot >= 0) {
        // segment_triangle once, on the winner with the axis at impact: the walk carries three registers for its best candidate
        const TriRecord* tp = sc.tris + best.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
        const f3 q0 = mk(s.p0.x + s.d.x * best.t, s.p0.y + s.d.y * best.t, s.p0.z + s.d.z * best.t);
        const f3 q1 = mk(s.p1.x + s.d.x * best.t, s.p1.y + s.d.y * best.t, s.p1.z + s.d.z * best.t);
        const f3 dq = q1 - q0;
        const SegPoint p = segment_triangle<true>(q0, q1, dq, dot(dq, dq), mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
        const float4 sr = sc.shade[best.slot];
        o0 = make_float4(best.t, __uint_as_float(best.prim), p.s, p.feature);
        o1 = make_float4(p.c.x, p.c.y, p.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
    }
    out[2ull * i] = o0;
    out[2ull * i + 1ull] = o1;
    if (COUNT) visits_out[i] = visits;
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_capsule_any(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, uint8_t* __restrict__ blocked)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    CapsuleRay s;
    const bool ok = capsule_load<FMT>(casts, i, n, scene_scale, sc.hspace, s);
    CapsuleWalk<true, kCapsulePlane> best(s);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, best, visits);
    if (i >= n) return;
    blocked[i] = (ok && best.slot >= 0) ? (uint8_t)1 : (uint8_t)0;
}

hipError_t launch_query_capsule_cast(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                     hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_capsule<11, false, kCapsulePlane>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, (uint2*)nullptr);
    return launch_lane_stack(k_query_capsule<0, false, kCapsulePlane>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, (uint2*)nullptr);
}

hipError_t launch_query_capsule_cast_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n,
                                         uint8_t* blocked, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_capsule_any<11>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, blocked);
    return launch_lane_stack(k_query_capsule_any<0>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, blocked);
}

hipError_t launch_capsule_cast_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                      uint2* visits, bool plane, hipStream_t stream)
{
    if (fmt == 11) {
        if (plane) return launch_lane_stack(k_query_capsule<11, true, true>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, visits);
        return launch_lane_stack(k_query_capsule<11, true, false>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, visits);
    }
    if (plane) return launch_lane_stack(k_query_capsule<0, true, true>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, visits);
    return launch_lane_stack(k_query_capsule<0, true, false>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, visits);
}

}  // namespace ptd
