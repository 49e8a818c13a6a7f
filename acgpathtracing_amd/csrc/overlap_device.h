// overlap_device.h — the device functions the box-overlap query (overlap.hip) shares with the complete-list queries (lists.hip): the
// triangle-box test, the child-box admission of both node formats, the sorted register list, the query record BoxQuery and the
// policies of the walk (bvh_walk.h) over a query record.  tritri_device.h takes fmin3 / fmax3, child_admitted_hc, the list and the
// policies from here.  Include only from a unit built with
// -ffp-contract=off (the triangle-box test is evaluated as written, and tests/overlap_ref.py mirrors it operation for operation).
#pragma once
#include "overlap.h"

namespace ptd {

__device__ __forceinline__ float fmin3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float fmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// One of the nine edge axes, cross(unit i, f) with (j, k) the two axes after i: the three vertices projected, against the box's radius.
// A NaN radius, or three NaN projections, separates.
__device__ __forceinline__ bool edge_axis_keeps(float p0j, float p0k, float p1j, float p1k, float p2j, float p2k, float fj, float fk, float hj, float hk)
{
    const float s0 = p0k * fj - p0j * fk, s1 = p1k * fj - p1j * fk, s2 = p2k * fj - p2j * fk;
    const float r = hj * fabsf(fk) + hk * fabsf(fj);
    return fmin3(s0, s1, s2) <= r && fmax3(s0, s1, s2) >= -r;
}
__device__ __forceinline__ bool edge_keeps(const f3& p0, const f3& p1, const f3& p2, const f3& f, const f3& h)
{
    const bool x = edge_axis_keeps(p0.y, p0.z, p1.y, p1.z, p2.y, p2.z, f.y, f.z, h.y, h.z);
    const bool y = edge_axis_keeps(p0.z, p0.x, p1.z, p1.x, p2.z, p2.x, f.z, f.x, h.z, h.x);
    const bool z = edge_axis_keeps(p0.x, p0.y, p1.x, p1.y, p2.x, p2.y, f.x, f.y, h.x, h.y);
    return x & y & z;
}

// Does the triangle {v0, v0 + e1, v0 + e2} overlap the box of centre c and half extent h: the separating-axis test of Akenine-Moeller
// (Fast 3D Triangle-Box Overlap Testing) in keep form, the three box faces, the triangle's plane and the nine edge axes, on the
// record's own vectors.  The 13 conditions are closed (touching overlaps) and combined without a branch, so a wave's lanes run one
// instruction stream.
__device__ __forceinline__ bool tri_box_overlap(const f3& c, const f3& h, const f3& v0, const f3& e1, const f3& e2)
{
    const f3 p0 = v0 - c, p1 = p0 + e1, p2 = p0 + e2;
    const bool faces = (fmin3(p0.x, p1.x, p2.x) <= h.x) & (fmax3(p0.x, p1.x, p2.x) >= -h.x) &
                       (fmin3(p0.y, p1.y, p2.y) <= h.y) & (fmax3(p0.y, p1.y, p2.y) >= -h.y) &
                       (fmin3(p0.z, p1.z, p2.z) <= h.z) & (fmax3(p0.z, p1.z, p2.z) >= -h.z);
    const f3 nrm = cross(e1, e2);
    const float d = dot(nrm, p0);
    const float r = (h.x * fabsf(nrm.x) + h.y * fabsf(nrm.y)) + h.z * fabsf(nrm.z);
    const bool plane = (d <= r) & (d >= -r);
    const f3 f1 = e2 - e1;
    return faces & plane & edge_keeps(p0, p1, p2, e1, h) & edge_keeps(p0, p1, p2, f1, h) & edge_keeps(p0, p1, p2, e2, h);
}

// The per-axis gap between the query centre and one child box, e_k = max(|centre_k - c_k| - half_k, 0); NaNs for an empty child, which
// no compare admits.
//   FMT 11: qc = c - centre of HSpace, once per lane; per axis t = g_c * is - qc (g_c, g_h the fp16 centre and half extent: world =
//           g * is + centre), e = max(|t| - g_h * is, 0): two v_fma_mix_f32 and a max, box_bound_hc's decode.  An empty child has g_h < 0.
//   FMT 0:  e = max(lo - c, c - hi, 0) from the fp32 planes.  An empty child has lo = +inf.
__device__ __forceinline__ bool child_admitted_hc(uint32_t px, uint32_t py, uint32_t pz, const f3& qc, const HSpace& hs, const f3& thr)
{
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const float tx = __builtin_fmaf((float)hx.x, hs.isx, -qc.x), ty = __builtin_fmaf((float)hy.x, hs.isy, -qc.y), tz = __builtin_fmaf((float)hz.x, hs.isz, -qc.z);
    float ex = fmaxf(__builtin_fmaf((float)hx.y, -hs.isx, fabsf(tx)), 0.0f);
    const float ey = fmaxf(__builtin_fmaf((float)hy.y, -hs.isy, fabsf(ty)), 0.0f);
    const float ez = fmaxf(__builtin_fmaf((float)hz.y, -hs.isz, fabsf(tz)), 0.0f);
    ex = (float)hx.y < 0.0f ? __builtin_nanf("") : ex;
    return (ex <= thr.x) & (ey <= thr.y) & (ez <= thr.z);
}
__device__ __forceinline__ bool child_admitted_f32(const f3& c, float lx, float ly, float lz, float hx, float hy, float hz, const f3& thr)
{
    float ex = fmaxf(fmaxf(lx - c.x, c.x - hx), 0.0f);
    const float ey = fmaxf(fmaxf(ly - c.y, c.y - hy), 0.0f), ez = fmaxf(fmaxf(lz - c.z, c.z - hz), 0.0f);
    ex = lx <= hx ? ex : __builtin_nanf("");
    return (ex <= thr.x) & (ey <= thr.y) & (ez <= thr.z);
}

// The lane's lowest triangle indices so far, ascending.  An empty entry is 0xFFFFFFFF, which is no triangle's index (n_tris < 2^32 - 1)
// and sorts behind every one.  N = 0 leaves nothing behind.
template <int N>
struct PrimList { uint32_t prim[N ? N : 1]; };

// Insert prim among the first max_prims entries; what falls off the end is dropped.  The candidate is carried down the list: at each
// entry it sorts before, the two change places.  Every triangle sits in one leaf, so no index comes twice.
template <int N>
__device__ __forceinline__ void list_insert(PrimList<N>& L, uint32_t max_prims, uint32_t prim)
{
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint32_t lp = L.prim[j];
        const bool sw = (uint32_t)j < max_prims && prim < lp;
        L.prim[j] = sw ? prim : lp;
        prim = sw ? lp : prim;
    }
}

// What the walk asks of a query record Q (BoxQuery here, TriQuery in tritri_device.h): load() the record (false: a miss before any
// traversal, or a lane past n), prepare() the walk's constants, admit a child box of either format, accept a triangle.
struct BoxQuery {
    f3 c, h, thr, qc;
    __device__ __forceinline__ bool load(const float4* __restrict__ boxes, uint32_t i, uint32_t n)
    {
        c = mk(0.0f); h = mk(0.0f);
        if (i >= n) return false;
        const float4 a = boxes[2ull * i], b = boxes[2ull * i + 1ull];
        c = mk(a.x, a.y, a.z);
        h = mk(a.w, b.x, b.y);
        return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) && __builtin_isfinite(a.w) && __builtin_isfinite(b.x) &&
               __builtin_isfinite(b.y) && a.w >= 0.0f && b.x >= 0.0f && b.y >= 0.0f;
    }
    __device__ __forceinline__ void prepare(const DeviceScene& sc, float scene_term)
    {
        thr = mk(h.x + (scene_term + (fabsf(c.x) + h.x) * kOverlapQuery), h.y + (scene_term + (fabsf(c.y) + h.y) * kOverlapQuery),
                 h.z + (scene_term + (fabsf(c.z) + h.z) * kOverlapQuery));
        qc = mk(c.x - sc.hspace.cx, c.y - sc.hspace.cy, c.z - sc.hspace.cz);
    }
    __device__ __forceinline__ bool admit_hc(uint32_t px, uint32_t py, uint32_t pz, const HSpace& hs) const { return child_admitted_hc(px, py, pz, qc, hs, thr); }
    __device__ __forceinline__ bool admit_f32(float lx, float ly, float lz, float hx, float hy, float hz) const { return child_admitted_f32(c, lx, ly, lz, hx, hy, hz, thr); }
    __device__ __forceinline__ bool accept(const f3& v0, const f3& e1, const f3& e2) const { return tri_box_overlap(c, h, v0, e1, e2); }
};

// The admission of the walks that keep the tree's order (overlap, triangles, lists): a child is entered iff q admits its box; of two
// admitted children the first is entered and the second pushed.
template <class Q>
struct AdmitBoth {
    Q q;
    __device__ __forceinline__ explicit AdmitBoth(const Q& q_) : q(q_) {}
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        h0 = q.admit_hc(qa.x, qa.y, qa.z, hs);
        h1 = q.admit_hc(qb.x, qb.y, qb.z, hs);
        first0 = true;
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        h0 = q.admit_f32(a.x, a.y, a.z, a.w, b.x, b.y);
        h1 = q.admit_f32(b.z, b.w, c.x, c.y, c.z, c.w);
        first0 = true;
    }
};

// The capped queries' policy: count what q accepts and keep the lowest max_prims indices in a list of CAP entries; ANY ends the lane at
// the first accepted triangle.  The boxes only prune: which triangles are accepted is decided by q.accept alone.
template <class Q, int CAP, bool ANY>
struct PrimListWalk : AdmitBoth<Q> {
    PrimList<CAP>& L;      // the kernel's: its epilogue writes the words
    uint32_t max_prims, count;
    __device__ __forceinline__ PrimListWalk(const Q& q_, uint32_t max_prims_, PrimList<CAP>& L_) : AdmitBoth<Q>(q_), L(L_), max_prims(max_prims_), count(0u)
    {
#pragma unroll
        for (int j = 0; j < CAP; j++) L.prim[j] = 0xFFFFFFFFu;
    }
    __device__ __forceinline__ bool leaf(int, const float4& r0, const float4& r1, const float4& r2)
    {
        if (this->q.accept(mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x))) {
            count++;
            if (ANY) return true;
            if constexpr (CAP > 0) list_insert(L, max_prims, __float_as_uint(r2.y));
        }
        return false;
    }
};

}  // namespace ptd
