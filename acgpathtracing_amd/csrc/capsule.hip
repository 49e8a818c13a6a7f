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
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk, the any-hit
// kernel and the record kernel's frame are cast_walk.h's.  This unit's own: the leaf statement capsule_triangle; the line of the
// axis' midpoint, each child box inflated per axis by half the axis and the radius (capsule.h: by a little more), the cut of
// capsule.h; the extra admission test, the separation of the box from the plane of the swept axis (capsule.h, PLANE); the record.
// A cast is three 16-byte loads and a record two 16-byte stores per lane.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the time of impact is evaluated as written, and tests/capsule_ref.py mirrors it operation for
// operation.
#include "capsule.h"
#include "cast_walk.h"
#include "sweep_device.h"        // sweep_vertex, sweep_edge, sweep_face: pt_query_sweep's three feature forms
#include "segment_device.h"      // segment_triangle: the start-overlap test and the record's (s, feature, c) are pt_query_segments' results

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

// What a lane keeps of its cast: cast_walk.h's per-query struct.  PLANE: the plane axis is tested.
template <bool PLANE>
struct CapsuleRay {
    static constexpr bool kAdmits = PLANE, kTracksCut = false;
    f3 p0, p1, a, d;
    float aa, dd, r, rr, tmax;
    f3 inv;             // finite 1-ulp reciprocals of d
    f3 qc;              // the axis' midpoint, minus the centre of HSpace for FMT 11
    f3 infl;            // |a_k| / 2 + R of capsule.h
    float abs_t;        // the absolute term of the far cut, in units of t
    f3 w;               // the unit normal of the swept axis' plane, or 0
    float plane_r;      // the right-hand side of the plane test less the box's own extent

    template <int FMT>
    __device__ __forceinline__ void setup(const f3& p0_, const f3& p1_, const f3& d_, float r_, float tmax_, float scene_scale, const HSpace& hs)
    {
        p0 = p0_; p1 = p1_; d = d_; r = r_; tmax = tmax_;
        a = p1 - p0;
        aa = dot(a, a);
        dd = dot(d, d);
        rr = r * r;
        inv = mk(finite_rcp(d.x), finite_rcp(d.y), finite_rcp(d.z));
        qc = mk(__builtin_fmaf(0.5f, a.x, p0.x), __builtin_fmaf(0.5f, a.y, p0.y), __builtin_fmaf(0.5f, a.z, p0.z));
        if (FMT == 11) qc = mk(qc.x - hs.cx, qc.y - hs.cy, qc.z - hs.cz);
        const float big = scene_scale + fmaxf(fmaxf(fmaxf(fabsf(p0.x), fabsf(p0.y)), fmaxf(fabsf(p0.z), fabsf(p1.x))), fmaxf(fabsf(p1.y), fabsf(p1.z)));
        const float R = __builtin_fmaf(r, kCapBoxRel, big * kCapBoxAbs);
        infl = mk(__builtin_fmaf(0.5f, fabsf(a.x), R), __builtin_fmaf(0.5f, fabsf(a.y), R), __builtin_fmaf(0.5f, fabsf(a.z), R));
        const float len = sqrtf(dd);
        abs_t = len > 0.0f ? __builtin_fmaf(big, kCapLinT, sqrtf(r * (r + big)) * kCapSqrtT) / len : INFINITY;
        // the plane of the swept axis: w = normalize(a x d) as computed, and what the computed w lets through (capsule.h)
        const f3 n = cross(a, d);
        const float l2 = dot(n, n);
        const float il = (l2 > 1e-30f && l2 < 1e30f && len > 0.0f) ? __builtin_amdgcn_rsqf(l2) : 0.0f;
        w = mk(n.x * il, n.y * il, n.z * il);
        const float wa = fabsf(dot(w, a)), wd = fabsf(dot(w, d));
        const float reach = __builtin_fmaf(4.0f, big, 2.0f * r);      // D of capsule.h
        const float tilt = len > 0.0f ? reach * wd / len : 0.0f;
        plane_r = __builtin_fmaf(R, kCapPlaneRel, __builtin_fmaf(0.5f, wa, __builtin_fmaf(big, kCapPlaneAbs, tilt)));
    }
    // cast i of the array, or an inert one for a lane past n.  Returns whether the lane has a cast that can touch something: p0, p1,
    // p1 - p0 and d finite, radius finite and >= 0, tmax >= 0 and no NaN (include/acgpt.h: "a miss before any traversal").  The
    // twelfth float is loaded with its float4 and never used.
    template <int FMT>
    __device__ __forceinline__ bool load(const float4* __restrict__ casts, uint32_t i, uint32_t n, float scene_scale, const HSpace& hs)
    {
        float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, g2 = g0;
        if (i < n) { g0 = casts[3ull * i]; g1 = casts[3ull * i + 1ull]; g2 = casts[3ull * i + 2ull]; }
        const float ax = g1.x - g0.x, ay = g1.y - g0.y, az = g1.z - g0.z;
        const bool ok = i < n && __builtin_isfinite(g0.x) && __builtin_isfinite(g0.y) && __builtin_isfinite(g0.z) && __builtin_isfinite(g0.w) &&
                        __builtin_isfinite(g1.x) && __builtin_isfinite(g1.y) && __builtin_isfinite(g1.z) && __builtin_isfinite(ax) && __builtin_isfinite(ay) &&
                        __builtin_isfinite(az) && __builtin_isfinite(g2.x) && __builtin_isfinite(g2.y) && __builtin_isfinite(g2.z) && g0.w >= 0.0f && g1.w >= 0.0f;
        if (!ok) { g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); g1 = g0; g2 = g0; }
        // tmax = +inf is the largest finite t: a time of impact of +inf stands for "no candidate"
        setup<FMT>(mk(g0.x, g0.y, g0.z), mk(g1.x, g1.y, g1.z), mk(g2.x, g2.y, g2.z), g0.w, fminf(g1.w, FLT_MAX), scene_scale, hs);
        return ok;
    }
    // cut of capsule.h for tb = min(tmax, best t); at most FLT_MAX, so that a box the line never reaches (entry +inf) is not entered
    __device__ __forceinline__ float cut(float tb) const { return fminf(__builtin_fmaf(tb, kCapRelT, abs_t), FLT_MAX); }
    __device__ __forceinline__ float toi(const float4& r0, const float4& r1, const float4& r2) const
    {
        return capsule_triangle(p0, p1, a, aa, d, dd, r, rr, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
    }
    // whether the box {c, g} reaches the plane of the swept axis.  c: the box centre minus the midpoint, g: its half extent
    __device__ __forceinline__ bool admit(const f3& c, const f3& g, bool keep) const
    {
        const float pd = fabsf(__builtin_fmaf(w.x, c.x, __builtin_fmaf(w.y, c.y, w.z * c.z)));
        const float pe = __builtin_fmaf(fabsf(w.x), g.x, __builtin_fmaf(fabsf(w.y), g.y, fabsf(w.z) * g.z));
        return keep && pd - pe <= plane_r;
    }
};

template <int FMT, bool COUNT, bool PLANE>
__global__ void __launch_bounds__(256)
k_query_capsule(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, float4* __restrict__ out,
                     uint2* __restrict__ visits_out)
{
    using Ray = CapsuleRay<PLANE>;
    cast_record_body<FMT, COUNT, Ray, Ray>(sc, stack_entries, scene_scale, casts, n, visits_out, [&](uint32_t i, const Ray& s, bool found, const auto& best) {
        float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
        if (found) {
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
    });
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_capsule_any(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, uint8_t* __restrict__ blocked)
{
    cast_any_body<FMT, CapsuleRay<kCapsulePlane>, CapsuleRay<kCapsulePlane>>(sc, stack_entries, scene_scale, casts, n, blocked);
}

hipError_t launch_query_capsule_cast(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                     hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) {
        return launch_cast(k_query_capsule<decltype(F)::value, false, kCapsulePlane>, sc, stack_entries, scene_scale, casts, n, stream, out, (uint2*)nullptr);
    });
}

hipError_t launch_query_capsule_cast_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n,
                                         uint8_t* blocked, hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) { return launch_cast(k_query_capsule_any<decltype(F)::value>, sc, stack_entries, scene_scale, casts, n, stream, blocked); });
}

hipError_t launch_capsule_cast_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                      uint2* visits, bool plane, hipStream_t stream)
{
    return dispatch_format(fmt, plane, [&](auto F, auto P) {
        return launch_cast(k_query_capsule<decltype(F)::value, true, decltype(P)::value>, sc, stack_entries, scene_scale, casts, n, stream, out, visits);
    });
}

}  // namespace ptd
