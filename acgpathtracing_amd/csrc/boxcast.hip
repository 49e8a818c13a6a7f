// boxcast.hip — the kernels behind pt_query_box_cast and pt_query_box_cast_any (include/acgpt.h).
//
//   k_query_obox_toi<FMT, COUNT, AXES>   one swept oriented box per lane from a device array: the triangle with the smallest time of
//                                        impact within [0, tmax], then the record (t, triangle, winning axis, material, normal, point).
//                                        COUNT also writes how many inner nodes the lane visited and how many triangles it tested (the
//                                        test hook's instantiations); AXES = false is the walk on the slab alone, the other arm of its
//                                        measurement.
//   k_query_obox_toi_any<FMT>            one byte per cast; a lane leaves the walk at its first triangle with a time of impact within
//                                        [0, tmax].
// (The names leave out "cast": tests/test_tricast_host.py counts the kernels whose name contains it.)
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk, the any-hit
// kernel and the record kernel's frame are cast_walk.h's.  This unit's own: the leaf statement obox_triangle (boxcast_device.h); the
// line of the box's centre, each child box inflated per world axis by the box's world half extent (boxcast.h: by a little more), the
// cut of boxcast.h; the extra admission test (AXES): the three box axes against the swept interval, which follows the cut, and the
// three axes cross(box axis, d), on which the swept box does not grow (boxcast.h); the record.  A cast is five 16-byte loads and a
// record three 16-byte stores per lane.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the time of impact is evaluated as written, and tests/boxcast_ref.py mirrors it operation for
// operation.
#include "boxcast.h"
#include "cast_walk.h"
#include "boxcast_device.h"

namespace ptd {

__device__ __forceinline__ float fdot(const f3& a, const f3& b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ float fdot_abs(const f3& a, const f3& b) { return __builtin_fmaf(fabsf(a.z), b.z, __builtin_fmaf(fabsf(a.y), b.y, fabsf(a.x) * b.x)); }

// What a lane keeps of its cast: cast_walk.h's per-query struct.  AXES: the six extra axes are tested.
template <bool AXES>
struct OBoxRay {
    static constexpr bool kAdmits = AXES, kTracksCut = AXES;
    OBoxQuery q;        // c, h and the axes u, v, w (neither q.qc nor the thresholds of the static walk are used)
    f3 d, nD;           // the direction, and -L(d): the triangle's velocity in the box's frame
    float tmax;
    f3 inv;             // finite 1-ulp reciprocals of d
    f3 qc;              // c, minus the centre of HSpace for FMT 11
    f3 infl;            // the inflation of a child box per world axis (boxcast.h)
    float abs_t;        // the absolute term of the far cut, in units of t
    // AXES
    f3 hb;              // h_j + m
    f3 dlo, dhi;        // D_j - delta, D_j + delta
    f3 w0, w1, w2;      // the unit normals cross(a_j, d), or 0
    f3 wthr;            // the right-hand sides of their tests less the child box's own extent
    f3 slo, shi;        // the swept intervals on the box axes for the walk's present cut

    __device__ __forceinline__ void cross_axis(const f3& a, float len, float reach, float m, float ortho, f3& w, float& thr) const
    {
        const f3 n = cross(a, d);
        const float l2 = dot(n, n);
        const float il = (l2 > 1e-30f && l2 < 1e30f && len > 0.0f) ? __builtin_amdgcn_rsqf(l2) : 0.0f;
        w = mk(n.x * il, n.y * il, n.z * il);
        const float rb = __builtin_fmaf(q.h.z, fabsf(fdot(w, q.w)), __builtin_fmaf(q.h.y, fabsf(fdot(w, q.v)), q.h.x * fabsf(fdot(w, q.u))));
        const float tilt = len > 0.0f ? reach * fabsf(fdot(w, d)) / len : 0.0f;
        thr = __builtin_fmaf(rb + tilt, kBoxCastCrossRel, ortho + m);
    }
    // q loaded, d and tmax as the record gives them (zeros for an inert lane)
    template <int FMT>
    __device__ __forceinline__ void setup(const f3& d_, float tmax_, float scene_scale, const HSpace& hs)
    {
        d = d_; tmax = tmax_;
        const f3 D = q.local(d);
        nD = mk(-D.x, -D.y, -D.z);
        inv = mk(finite_rcp(d.x), finite_rcp(d.y), finite_rcp(d.z));
        qc = q.c;
        if (FMT == 11) qc = mk(q.c.x - hs.cx, q.c.y - hs.cy, q.c.z - hs.cz);
        const float hsum = (q.h.x + q.h.y) + q.h.z;
        const float M = scene_scale + fmax3(fabsf(q.c.x), fabsf(q.c.y), fabsf(q.c.z)) + hsum;
        const float m = M * kBoxCastAbs;
        const float mw = __builtin_fmaf(hsum, kBoxCastOrtho, m);
        // H_k = sum_j |A_kj| h_j: row k of the 3 x 3 part is (u_k, v_k, w_k)
        infl = mk(__builtin_fmaf(fabsf(q.w.x), q.h.z, __builtin_fmaf(fabsf(q.v.x), q.h.y, __builtin_fmaf(fabsf(q.u.x), q.h.x, mw))),
                  __builtin_fmaf(fabsf(q.w.y), q.h.z, __builtin_fmaf(fabsf(q.v.y), q.h.y, __builtin_fmaf(fabsf(q.u.y), q.h.x, mw))),
                  __builtin_fmaf(fabsf(q.w.z), q.h.z, __builtin_fmaf(fabsf(q.v.z), q.h.y, __builtin_fmaf(fabsf(q.u.z), q.h.x, mw))));
        const float len = sqrtf(dot(d, d));
        abs_t = len > 0.0f ? M * kBoxCastLinT / len : INFINITY;
        if (AXES) {
            hb = mk(q.h.x + m, q.h.y + m, q.h.z + m);
            const float delta = len * kBoxCastDirRel;
            dlo = mk(D.x - delta, D.y - delta, D.z - delta);
            dhi = mk(D.x + delta, D.y + delta, D.z + delta);
            const float reach = 4.0f * M, ortho = hsum * kBoxCastCrossOrtho;
            cross_axis(q.u, len, reach, m, ortho, w0, wthr.x);
            cross_axis(q.v, len, reach, m, ortho, w1, wthr.y);
            cross_axis(q.w, len, reach, m, ortho, w2, wthr.z);
        }
    }
    // cast i of the array, or an inert one for a lane past n.  Returns whether the lane has a cast that can touch something: the first
    // sixteen floats by OBoxQuery::load's rule, d finite, tmax >= 0 and no NaN (include/acgpt.h: "a miss before any traversal").  A
    // cast is five float4 and OBoxQuery::load reads base[4 i ..]: with base = casts + i that is casts[5 i ..], the cast's first four.
    template <int FMT>
    __device__ __forceinline__ bool load(const float4* __restrict__ casts, uint32_t i, uint32_t n, float scene_scale, const HSpace& hs)
    {
        bool ok = q.load(casts + i, i, n);
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n) g = casts[5ull * i + 4ull];
        ok = ok && __builtin_isfinite(g.x) && __builtin_isfinite(g.y) && __builtin_isfinite(g.z) && g.w >= 0.0f;
        if (!ok) {
            g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            q.c = mk(0.0f); q.h = mk(0.0f); q.u = mk(0.0f); q.v = mk(0.0f); q.w = mk(0.0f);
        }
        // tmax = +inf is the largest finite t: a time of impact of +inf stands for "no candidate"
        setup<FMT>(mk(g.x, g.y, g.z), fminf(g.w, FLT_MAX), scene_scale, hs);
        return ok;
    }
    // cut of boxcast.h for tb = min(tmax, best t); at most FLT_MAX, so that a box the line never reaches (entry +inf) is not entered
    __device__ __forceinline__ float cut(float tb) const { return fminf(__builtin_fmaf(tb, kBoxCastRelT, abs_t), FLT_MAX); }
    // AXES: the swept intervals on the three box axes for this cut
    __device__ __forceinline__ void cut_moved(float bound)
    {
        slo = mk(fminf(bound * dlo.x, 0.0f) - hb.x, fminf(bound * dlo.y, 0.0f) - hb.y, fminf(bound * dlo.z, 0.0f) - hb.z);
        shi = mk(fmaxf(bound * dhi.x, 0.0f) + hb.x, fmaxf(bound * dhi.y, 0.0f) + hb.y, fmaxf(bound * dhi.z, 0.0f) + hb.z);
    }
    __device__ __forceinline__ float toi(const float4& r0, const float4& r1, const float4& r2) const
    {
        OBoxClip clip;
        return obox_triangle(q.h, q.local(mk(r0.x, r0.y, r0.z) - q.c), q.local(mk(r0.w, r1.x, r1.y)), q.local(mk(r1.z, r1.w, r2.x)), nD, clip);
    }
    // AXES: whether the box {c, g} reaches the swept box on the three box axes and on the three cross axes.  c: the box centre minus
    // the cast's centre, g: its half extent
    __device__ __forceinline__ bool admit(const f3& c, const f3& g, bool keep) const
    {
        const float pu = fdot(q.u, c), ru = fdot_abs(q.u, g);
        const float pv = fdot(q.v, c), rv = fdot_abs(q.v, g);
        const float pw = fdot(q.w, c), rw = fdot_abs(q.w, g);
        return keep & (pu + ru >= slo.x) & (pu - ru <= shi.x) & (pv + rv >= slo.y) & (pv - rv <= shi.y) & (pw + rw >= slo.z) & (pw - rw <= shi.z) &
               (fabsf(fdot(w0, c)) - fdot_abs(w0, g) <= wthr.x) & (fabsf(fdot(w1, c)) - fdot_abs(w1, g) <= wthr.y) & (fabsf(fdot(w2, c)) - fdot_abs(w2, g) <= wthr.z);
    }
};

template <int FMT, bool COUNT, bool AXES>
__global__ void __launch_bounds__(256)
k_query_obox_toi(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, float4* __restrict__ out,
                 uint2* __restrict__ visits_out)
{
    using Ray = OBoxRay<AXES>;
    cast_record_body<FMT, COUNT, Ray, Ray>(sc, stack_entries, scene_scale, casts, n, visits_out, [&](uint32_t i, const Ray& s, bool found, const auto& best) {
        float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, __uint_as_float(0xFFFFFFFFu)), o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o2 = o1;
        if (found) {
            // the leaf test once more, on the winner: the walk carries three registers for its best candidate
            const TriRecord* tp = sc.tris + best.slot;
            const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
            const f3 v0 = mk(r0.x, r0.y, r0.z), e1 = mk(r0.w, r1.x, r1.y), e2 = mk(r1.z, r1.w, r2.x);
            const f3 P0 = s.q.local(v0 - s.q.c), E1 = s.q.local(e1), E2 = s.q.local(e2);
            OBoxClip clip;
            const float t = obox_triangle(s.q.h, P0, E1, E2, s.nD, clip);
            const float4 sr = sc.shade[best.slot];
            o0 = make_float4(t, __uint_as_float(best.prim), (float)clip.ax, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
            if (clip.ax != 13) {
                f3 nn, pp;
                obox_contact(s.q, s.d, v0, e1, e2, P0, E1, E2, s.nD, clip, t, nn, pp);
                o1 = make_float4(nn.x, nn.y, nn.z, 0.0f);
                o2 = make_float4(pp.x, pp.y, pp.z, 0.0f);
            }
        }
        out[3ull * i] = o0;
        out[3ull * i + 1ull] = o1;
        out[3ull * i + 2ull] = o2;
    });
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_obox_toi_any(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, uint8_t* __restrict__ blocked)
{
    cast_any_body<FMT, OBoxRay<kBoxCastAxes>, OBoxRay<kBoxCastAxes>>(sc, stack_entries, scene_scale, casts, n, blocked);
}

hipError_t launch_query_box_toi(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) {
        return launch_cast(k_query_obox_toi<decltype(F)::value, false, kBoxCastAxes>, sc, stack_entries, scene_scale, casts, n, stream, out, (uint2*)nullptr);
    });
}

hipError_t launch_query_box_toi_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n,
                                    uint8_t* blocked, hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) { return launch_cast(k_query_obox_toi_any<decltype(F)::value>, sc, stack_entries, scene_scale, casts, n, stream, blocked); });
}

hipError_t launch_box_toi_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                 uint2* visits, bool axes, hipStream_t stream)
{
    return dispatch_format(fmt, axes, [&](auto F, auto A) {
        return launch_cast(k_query_obox_toi<decltype(F)::value, true, decltype(A)::value>, sc, stack_entries, scene_scale, casts, n, stream, out, visits);
    });
}

}  // namespace ptd
