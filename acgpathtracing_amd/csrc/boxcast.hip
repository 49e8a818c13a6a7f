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
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk is capsule.hip's
// slab test with the line of the box's centre against each child box inflated per world axis by the box's world half extent
// (boxcast.h: by a little more), clipped to [0, min(tmax, best t)] widened; AXES adds the three box axes against the swept interval
// and the three axes cross(box axis, d), on which the swept box does not grow (boxcast.h), nearer child first.  256-lane workgroups
// over a one-dimensional grid, the lane stack of query_launch.h.  A cast is five 16-byte loads and a record three 16-byte stores per
// lane.  Lanes past n and lanes whose cast is a miss before any traversal stay in the wave, inactive.  No atomics: two calls give the
// same bits.
// Built with -ffp-contract=off: the time of impact is evaluated as written, and tests/boxcast_ref.py mirrors it operation for
// operation.  The box tests are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "boxcast.h"
#include "bvh_walk.h"
#include "boxcast_device.h"

#include <cfloat>

namespace ptd {

__device__ __forceinline__ float fdot(const f3& a, const f3& b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ float fdot_abs(const f3& a, const f3& b) { return __builtin_fmaf(fabsf(a.z), b.z, __builtin_fmaf(fabsf(a.y), b.y, fabsf(a.x) * b.x)); }

// What a lane keeps of its cast for the walk.
template <bool AXES>
struct OBoxRay {
    OBoxQuery q;        // c, h and the axes u, v, w; q.qc = c in the fp16 nodes' space (the thresholds of the static walk are not used)
    f3 d, nD;           // the direction, and -L(d): the triangle's velocity in the box's frame
    float tmax;
    f3 inv;             // finite 1-ulp reciprocals of d
    f3 infl;            // the inflation of a child box per world axis (boxcast.h)
    float abs_t;        // the absolute term of the far cut, in units of t
    // AXES
    f3 hb;              // h_j + m
    f3 dlo, dhi;        // D_j - delta, D_j + delta
    f3 w0, w1, w2;      // the unit normals cross(a_j, d), or 0
    f3 wthr;            // the right-hand sides of their tests less the child box's own extent
};

template <bool AXES>
__device__ __forceinline__ void obox_cross_axis(const OBoxRay<AXES>& s, const f3& a, float len, float reach, float m, float ortho, f3& w, float& thr)
{
    const f3 n = cross(a, s.d);
    const float l2 = dot(n, n);
    const float il = (l2 > 1e-30f && l2 < 1e30f && len > 0.0f) ? __builtin_amdgcn_rsqf(l2) : 0.0f;
    w = mk(n.x * il, n.y * il, n.z * il);
    const float rb = __builtin_fmaf(s.q.h.z, fabsf(fdot(w, s.q.w)), __builtin_fmaf(s.q.h.y, fabsf(fdot(w, s.q.v)), s.q.h.x * fabsf(fdot(w, s.q.u))));
    const float tilt = len > 0.0f ? reach * fabsf(fdot(w, s.d)) / len : 0.0f;
    thr = __builtin_fmaf(rb + tilt, kBoxCastCrossRel, ortho + m);
}

// q loaded, d and tmax as the record gives them (zeros for an inert lane)
template <int FMT, bool AXES>
__device__ __forceinline__ void obox_setup(OBoxRay<AXES>& s, const f3& d, float tmax, float scene_scale, const HSpace& hs)
{
    const OBoxQuery& q = s.q;
    s.d = d; s.tmax = tmax;
    const f3 D = q.local(d);
    s.nD = mk(-D.x, -D.y, -D.z);
    s.inv = mk(finite_rcp(d.x), finite_rcp(d.y), finite_rcp(d.z));
    s.q.qc = q.c;
    if (FMT == 11) s.q.qc = mk(q.c.x - hs.cx, q.c.y - hs.cy, q.c.z - hs.cz);
    const float hsum = (q.h.x + q.h.y) + q.h.z;
    const float M = scene_scale + fmax3(fabsf(q.c.x), fabsf(q.c.y), fabsf(q.c.z)) + hsum;
    const float m = M * kBoxCastAbs;
    const float mw = __builtin_fmaf(hsum, kBoxCastOrtho, m);
    // H_k = sum_j |A_kj| h_j: row k of the 3 x 3 part is (u_k, v_k, w_k)
    s.infl = mk(__builtin_fmaf(fabsf(q.w.x), q.h.z, __builtin_fmaf(fabsf(q.v.x), q.h.y, __builtin_fmaf(fabsf(q.u.x), q.h.x, mw))),
                __builtin_fmaf(fabsf(q.w.y), q.h.z, __builtin_fmaf(fabsf(q.v.y), q.h.y, __builtin_fmaf(fabsf(q.u.y), q.h.x, mw))),
                __builtin_fmaf(fabsf(q.w.z), q.h.z, __builtin_fmaf(fabsf(q.v.z), q.h.y, __builtin_fmaf(fabsf(q.u.z), q.h.x, mw))));
    const float len = sqrtf(dot(d, d));
    s.abs_t = len > 0.0f ? M * kBoxCastLinT / len : INFINITY;
    if (AXES) {
        s.hb = mk(q.h.x + m, q.h.y + m, q.h.z + m);
        const float delta = len * kBoxCastDirRel;
        s.dlo = mk(D.x - delta, D.y - delta, D.z - delta);
        s.dhi = mk(D.x + delta, D.y + delta, D.z + delta);
        const float reach = 4.0f * M, ortho = hsum * kBoxCastCrossOrtho;
        obox_cross_axis(s, q.u, len, reach, m, ortho, s.w0, s.wthr.x);
        obox_cross_axis(s, q.v, len, reach, m, ortho, s.w1, s.wthr.y);
        obox_cross_axis(s, q.w, len, reach, m, ortho, s.w2, s.wthr.z);
    }
}
// cut of boxcast.h for tb = min(tmax, best t); at most FLT_MAX, so that a box the line never reaches (entry +inf) is not entered
template <bool AXES>
__device__ __forceinline__ float obox_cut(const OBoxRay<AXES>& s, float tb) { return fminf(__builtin_fmaf(tb, kBoxCastRelT, s.abs_t), FLT_MAX); }

// One child: entry and exit of the centre's line in the box inflated by s.infl, clipped to [0, cut], and (AXES) whether the box
// reaches the swept box on the three box axes (slo, shi: the swept intervals for this cut) and on the three cross axes; tn = NaN for
// an empty child or a separated box, which no compare admits.  c: the box centre minus the cast's centre, g: the box's half extent,
// e = g + infl, per axis, in world units; the products with +-1e30 for a zero direction component give +-inf or 0, never a NaN.
template <bool AXES>
__device__ __forceinline__ void obox_child(const f3& c, const f3& g, const f3& e, const OBoxRay<AXES>& s, float cut, const f3& slo, const f3& shi, bool empty, float& tn,
                                           float& tf)
{
    const float x0 = (c.x - e.x) * s.inv.x, x1 = (c.x + e.x) * s.inv.x;
    const float y0 = (c.y - e.y) * s.inv.y, y1 = (c.y + e.y) * s.inv.y;
    const float z0 = (c.z - e.z) * s.inv.z, z1 = (c.z + e.z) * s.inv.z;
    tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
    tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), cut));
    bool keep = !empty;
    if (AXES) {
        const float pu = fdot(s.q.u, c), ru = fdot_abs(s.q.u, g);
        const float pv = fdot(s.q.v, c), rv = fdot_abs(s.q.v, g);
        const float pw = fdot(s.q.w, c), rw = fdot_abs(s.q.w, g);
        keep &= (pu + ru >= slo.x) & (pu - ru <= shi.x) & (pv + rv >= slo.y) & (pv - rv <= shi.y) & (pw + rw >= slo.z) & (pw - rw <= shi.z);
        keep &= (fabsf(fdot(s.w0, c)) - fdot_abs(s.w0, g) <= s.wthr.x) & (fabsf(fdot(s.w1, c)) - fdot_abs(s.w1, g) <= s.wthr.y) &
                (fabsf(fdot(s.w2, c)) - fdot_abs(s.w2, g) <= s.wthr.z);
    }
    if (!keep) tn = __builtin_nanf("");
}
template <bool AXES>
__device__ __forceinline__ void obox_child_hc(uint32_t px, uint32_t py, uint32_t pz, const OBoxRay<AXES>& s, const HSpace& hs, float cut, const f3& slo, const f3& shi,
                                              float& tn, float& tf)
{
    // world = g * is + centre: c = centre_g * is - qc, g = half_g * is, e = half_g * is + infl, one v_fma_mix_f32 each
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const f3 c = mk(__builtin_fmaf((float)hx.x, hs.isx, -s.q.qc.x), __builtin_fmaf((float)hy.x, hs.isy, -s.q.qc.y), __builtin_fmaf((float)hz.x, hs.isz, -s.q.qc.z));
    const f3 g = mk((float)hx.y * hs.isx, (float)hy.y * hs.isy, (float)hz.y * hs.isz);
    const f3 e = mk(__builtin_fmaf((float)hx.y, hs.isx, s.infl.x), __builtin_fmaf((float)hy.y, hs.isy, s.infl.y), __builtin_fmaf((float)hz.y, hs.isz, s.infl.z));
    obox_child<AXES>(c, g, e, s, cut, slo, shi, (float)hx.y < 0.0f, tn, tf);
}
template <bool AXES>
__device__ __forceinline__ void obox_child_f32(float lx, float ly, float lz, float hx, float hy, float hz, const OBoxRay<AXES>& s, float cut, const f3& slo, const f3& shi,
                                               float& tn, float& tf)
{
    // the half extent from the rounded centre m, so that [m - g, m + g] holds [lo, hi] to an ulp of the extent
    const f3 m = mk(0.5f * lx + 0.5f * hx, 0.5f * ly + 0.5f * hy, 0.5f * lz + 0.5f * hz);
    const f3 c = m - s.q.qc;
    const bool empty = !(lx <= hx);
    // an empty child has lo = +inf: its extents are kept out of the arithmetic
    const f3 g = empty ? mk(0.0f) : mk(fmaxf(hx - m.x, m.x - lx), fmaxf(hy - m.y, m.y - ly), fmaxf(hz - m.z, m.z - lz));
    obox_child<AXES>(c, g, g + s.infl, s, cut, slo, shi, empty, tn, tf);
}

// One cast per lane through the two-child BVH (bvh_walk.h: the stack depth, the one-word entries).  The boxes only prune: the winner
// is decided by the leaf test, t <= tmax, smallest t, ties to the lowest triangle index, whatever order the walk reaches the triangles
// in.  ANY: leave at the first triangle with t <= tmax (slot >= 0 says so).
template <bool ANY, bool AXES>
struct OBoxWalk {
    OBoxRay<AXES> s;
    float cut;
    f3 slo, shi;                            // AXES: the swept intervals on the box axes for this cut
    float t; int slot; uint32_t prim;      // the best candidate so far
    __device__ __forceinline__ explicit OBoxWalk(const OBoxRay<AXES>& s_) : s(s_), t(INFINITY), slot(-1), prim(0xFFFFFFFFu) { set_cut(s_.tmax); }
    __device__ __forceinline__ void set_cut(float tb)
    {
        cut = obox_cut(s, tb);
        if (AXES) {
            slo = mk(fminf(cut * s.dlo.x, 0.0f) - s.hb.x, fminf(cut * s.dlo.y, 0.0f) - s.hb.y, fminf(cut * s.dlo.z, 0.0f) - s.hb.z);
            shi = mk(fmaxf(cut * s.dhi.x, 0.0f) + s.hb.x, fmaxf(cut * s.dhi.y, 0.0f) + s.hb.y, fmaxf(cut * s.dhi.z, 0.0f) + s.hb.z);
        } else {
            slo = mk(0.0f); shi = mk(0.0f);
        }
    }
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        obox_child_hc<AXES>(qa.x, qa.y, qa.z, s, hs, cut, slo, shi, n0, f0);
        obox_child_hc<AXES>(qb.x, qb.y, qb.z, s, hs, cut, slo, shi, n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        float n0, f0, n1, f1;
        obox_child_f32<AXES>(a.x, a.y, a.z, a.w, b.x, b.y, s, cut, slo, shi, n0, f0);
        obox_child_f32<AXES>(b.z, b.w, c.x, c.y, c.z, c.w, s, cut, slo, shi, n1, f1);
        admit_by_interval(n0, f0, n1, f1, h0, h1, first0);
    }
    __device__ __forceinline__ bool leaf(int slot_, const float4& r0, const float4& r1, const float4& r2)
    {
        OBoxClip clip;
        const float t_ = obox_triangle(s.q.h, s.q.local(mk(r0.x, r0.y, r0.z) - s.q.c), s.q.local(mk(r0.w, r1.x, r1.y)), s.q.local(mk(r1.z, r1.w, r2.x)), s.nD, clip);
        const uint32_t prim_ = __float_as_uint(r2.y);
        if (ANY) {
            if (t_ <= s.tmax) { slot = slot_; return true; }
        } else if (t_ <= s.tmax && (t_ < t || (t_ == t && prim_ < prim))) {
            t = t_; slot = slot_; prim = prim_;
            set_cut(t_);
        }
        return false;
    }
};

// cast i of the array, or an inert one for a lane past n.  Returns whether the lane has a cast that can touch something: the first
// sixteen floats by OBoxQuery::load's rule, d finite, tmax >= 0 and no NaN (include/acgpt.h: "a miss before any traversal").  A cast
// is five float4 and OBoxQuery::load reads base[4 i ..]: with base = casts + i that is casts[5 i ..], the cast's first four.
template <int FMT, bool AXES>
__device__ __forceinline__ bool obox_load(const float4* __restrict__ casts, uint32_t i, uint32_t n, float scene_scale, const HSpace& hs, OBoxRay<AXES>& s)
{
    bool ok = s.q.load(casts + i, i, n);
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < n) g = casts[5ull * i + 4ull];
    ok = ok && __builtin_isfinite(g.x) && __builtin_isfinite(g.y) && __builtin_isfinite(g.z) && g.w >= 0.0f;
    if (!ok) {
        g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s.q.c = mk(0.0f); s.q.h = mk(0.0f); s.q.u = mk(0.0f); s.q.v = mk(0.0f); s.q.w = mk(0.0f);
    }
    // tmax = +inf is the largest finite t: a time of impact of +inf stands for "no candidate"
    obox_setup<FMT>(s, mk(g.x, g.y, g.z), fminf(g.w, FLT_MAX), scene_scale, hs);
    return ok;
}

template <int FMT, bool COUNT, bool AXES>
__global__ void __launch_bounds__(256)
k_query_obox_toi(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, float4* __restrict__ out,
                 uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    OBoxRay<AXES> s;
    const bool ok = obox_load<FMT>(casts, i, n, scene_scale, sc.hspace, s);
    OBoxWalk<false, AXES> best(s);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, COUNT>(sc, st, ok, best, visits);
    if (i >= n) return;
    float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, __uint_as_float(0xFFFFFFFFu)), o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o2 = o1;
    if (ok && best.slot >= 0) {
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
    if (COUNT) visits_out[i] = visits;
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_obox_toi_any(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, uint8_t* __restrict__ blocked)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    OBoxRay<kBoxCastAxes> s;
    const bool ok = obox_load<FMT>(casts, i, n, scene_scale, sc.hspace, s);
    OBoxWalk<true, kBoxCastAxes> best(s);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, best, visits);
    if (i >= n) return;
    blocked[i] = (ok && best.slot >= 0) ? (uint8_t)1 : (uint8_t)0;
}

hipError_t launch_query_box_toi(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_obox_toi<11, false, kBoxCastAxes>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, (uint2*)nullptr);
    return launch_lane_stack(k_query_obox_toi<0, false, kBoxCastAxes>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, (uint2*)nullptr);
}

hipError_t launch_query_box_toi_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n,
                                    uint8_t* blocked, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_obox_toi_any<11>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, blocked);
    return launch_lane_stack(k_query_obox_toi_any<0>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, blocked);
}

hipError_t launch_box_toi_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                 uint2* visits, bool axes, hipStream_t stream)
{
    if (fmt == 11) {
        if (axes) return launch_lane_stack(k_query_obox_toi<11, true, true>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, visits);
        return launch_lane_stack(k_query_obox_toi<11, true, false>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, visits);
    }
    if (axes) return launch_lane_stack(k_query_obox_toi<0, true, true>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, visits);
    return launch_lane_stack(k_query_obox_toi<0, true, false>, stack_entries, n, stream, sc, stack_entries, scene_scale, casts, n, out, visits);
}

}  // namespace ptd
