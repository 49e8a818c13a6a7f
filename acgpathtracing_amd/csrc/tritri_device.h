// tritri_device.h — the device functions the triangle-against-mesh query (tritri.hip) shares with the complete-list queries
// (lists.hip): the triangle-triangle test, the child-box admission of the fp32 nodes and the query record TriQuery.  fmin3 / fmax3,
// child_admitted_hc (the fp16 nodes' admission, the same for a box and for a triangle's bounding box), the sorted register list and
// the walk's policies come from overlap_device.h.  Include only from a unit built with -ffp-contract=off (the test is evaluated as written, and
// tests/tritri_ref.py mirrors it operation for operation).
#pragma once
#include "tritri.h"
#include "overlap_device.h"

namespace ptd {

// One separating axis L in keep form.  The scene triangle's vertices relative to a0 are p0, p1, p2; the query triangle's are 0, f1, f2.
// Three NaN s fail the condition; a NaN t is ignored by fmin3 / fmax3, which always have the 0 to return.
__device__ __forceinline__ bool axis_keeps(const f3& L, const f3& p0, const f3& p1, const f3& p2, const f3& f1, const f3& f2)
{
    const float s0 = dot(L, p0), s1 = dot(L, p1), s2 = dot(L, p2);
    const float t1 = dot(L, f1), t2 = dot(L, f2);
    return (fmin3(s0, s1, s2) <= fmax3(0.0f, t1, t2)) & (fmax3(s0, s1, s2) >= fmin3(0.0f, t1, t2));
}

// The running conjunction of the conditions, kept in a vector register and closed after every axis.  Left to itself the compiler keeps
// all 40 lane masks in scalar registers and combines them at the end: 106 SGPRs, with kernel arguments spilled to make room, and 20
// more VGPRs for the axes it computes ahead.  The empty statement pins the select; the barrier keeps the next axis from starting early.
__device__ __forceinline__ void fold(uint32_t& keep, bool c)
{
    keep = c ? keep : 0u;
    asm volatile("" : "+v"(keep));
    __builtin_amdgcn_sched_barrier(0);
}

// The three axes cross(a, b) of one edge a of the query triangle against the scene triangle's edges b in (e1, e2 - e1, e2)
__device__ __forceinline__ bool edge_keeps(const f3& a, const f3& e1, const f3& e21, const f3& e2, const f3& p0, const f3& p1, const f3& p2, const f3& f1, const f3& f2)
{
    return axis_keeps(cross(a, e1), p0, p1, p2, f1, f2) & axis_keeps(cross(a, e21), p0, p1, p2, f1, f2) & axis_keeps(cross(a, e2), p0, p1, p2, f1, f2);
}

// Does the scene triangle {v0, v0 + e1, v0 + e2} intersect the query triangle {a0, a0 + f1, a0 + f2}, whose bounding box is [qlo, qhi]:
// the separating-axis test in keep form, on the record's own vectors.  Three box conditions on the coordinates as they are, then 17
// axes: the two normals, the nine products of an edge of each, and per triangle the three in-plane normals of its edges, without which
// two coplanar triangles always intersect.  The 20 conditions are closed (touching intersects) and combined without a branch, so a
// wave's lanes run one instruction stream.
__device__ __forceinline__ bool tri_tri_intersect(const f3& a0, const f3& f1, const f3& f2, const f3& qlo, const f3& qhi, const f3& v0, const f3& e1, const f3& e2)
{
    const f3 w1 = v0 + e1, w2 = v0 + e2;
    const bool boxes = (fmin3(v0.x, w1.x, w2.x) <= qhi.x) & (fmax3(v0.x, w1.x, w2.x) >= qlo.x) &
                       (fmin3(v0.y, w1.y, w2.y) <= qhi.y) & (fmax3(v0.y, w1.y, w2.y) >= qlo.y) &
                       (fmin3(v0.z, w1.z, w2.z) <= qhi.z) & (fmax3(v0.z, w1.z, w2.z) >= qlo.z);
    const f3 p0 = v0 - a0, p1 = p0 + e1, p2 = p0 + e2;
    const f3 f21 = f2 - f1, e21 = e2 - e1;
    const f3 nA = cross(f1, f2), nB = cross(e1, e2);
    uint32_t keep = boxes ? 1u : 0u;
    fold(keep, axis_keeps(nA, p0, p1, p2, f1, f2));
    fold(keep, axis_keeps(nB, p0, p1, p2, f1, f2));
    fold(keep, edge_keeps(f1, e1, e21, e2, p0, p1, p2, f1, f2));
    fold(keep, edge_keeps(f21, e1, e21, e2, p0, p1, p2, f1, f2));
    fold(keep, edge_keeps(f2, e1, e21, e2, p0, p1, p2, f1, f2));
    fold(keep, axis_keeps(cross(nA, f1), p0, p1, p2, f1, f2));
    fold(keep, axis_keeps(cross(nA, f21), p0, p1, p2, f1, f2));
    fold(keep, axis_keeps(cross(nA, f2), p0, p1, p2, f1, f2));
    fold(keep, axis_keeps(cross(nB, e1), p0, p1, p2, f1, f2));
    fold(keep, axis_keeps(cross(nB, e21), p0, p1, p2, f1, f2));
    fold(keep, axis_keeps(cross(nB, e2), p0, p1, p2, f1, f2));
    return keep != 0u;
}

// FMT 0: the child's planes against the query box's, as they are.  An empty child has lo = +inf, which no finite qhi admits.
__device__ __forceinline__ bool child_admitted_f32(const f3& qlo, const f3& qhi, float lx, float ly, float lz, float hx, float hy, float hz)
{
    return (lx <= qhi.x) & (hx >= qlo.x) & (ly <= qhi.y) & (hy >= qlo.y) & (lz <= qhi.z) & (hz >= qlo.z);
}

// The query record of the walk's policies (overlap_device.h says what they ask of it).
struct TriQuery {
    f3 a0, f1, f2, qlo, qhi, thr, qc;
    __device__ __forceinline__ bool load(const float4* __restrict__ tris, uint32_t i, uint32_t n)
    {
        f3 a1 = mk(0.0f), a2 = mk(0.0f);
        a0 = mk(0.0f);
        bool ok = false;
        if (i < n) {
            const float4 r0 = tris[3ull * i], r1 = tris[3ull * i + 1ull], r2 = tris[3ull * i + 2ull];
            a0 = mk(r0.x, r0.y, r0.z);
            a1 = mk(r1.x, r1.y, r1.z);
            a2 = mk(r2.x, r2.y, r2.z);
            ok = __builtin_isfinite(r0.x) && __builtin_isfinite(r0.y) && __builtin_isfinite(r0.z) && __builtin_isfinite(r1.x) && __builtin_isfinite(r1.y) &&
                 __builtin_isfinite(r1.z) && __builtin_isfinite(r2.x) && __builtin_isfinite(r2.y) && __builtin_isfinite(r2.z);
        }
        qlo = mk(fmin3(a0.x, a1.x, a2.x), fmin3(a0.y, a1.y, a2.y), fmin3(a0.z, a1.z, a2.z));
        qhi = mk(fmax3(a0.x, a1.x, a2.x), fmax3(a0.y, a1.y, a2.y), fmax3(a0.z, a1.z, a2.z));
        f1 = a1 - a0;
        f2 = a2 - a0;
        return ok;
    }
    // load()'s record from three vertices in registers (poses.hip transforms them there).  False: a coordinate is not finite.
    __device__ __forceinline__ bool set(const f3& a0_, const f3& a1, const f3& a2)
    {
        a0 = a0_;
        qlo = mk(fmin3(a0.x, a1.x, a2.x), fmin3(a0.y, a1.y, a2.y), fmin3(a0.z, a1.z, a2.z));
        qhi = mk(fmax3(a0.x, a1.x, a2.x), fmax3(a0.y, a1.y, a2.y), fmax3(a0.z, a1.z, a2.z));
        f1 = a1 - a0;
        f2 = a2 - a0;
        return __builtin_isfinite(a0.x) && __builtin_isfinite(a0.y) && __builtin_isfinite(a0.z) && __builtin_isfinite(a1.x) && __builtin_isfinite(a1.y) &&
               __builtin_isfinite(a1.z) && __builtin_isfinite(a2.x) && __builtin_isfinite(a2.y) && __builtin_isfinite(a2.z);
    }
    __device__ __forceinline__ void prepare(const DeviceScene& sc, float scene_term)
    {
        // FMT 11 only: the query box as centre and half extent (the halves are exact, the sum and the difference round once each)
        const f3 c = mk(0.5f * qlo.x + 0.5f * qhi.x, 0.5f * qlo.y + 0.5f * qhi.y, 0.5f * qlo.z + 0.5f * qhi.z);
        const f3 h = mk(0.5f * qhi.x - 0.5f * qlo.x, 0.5f * qhi.y - 0.5f * qlo.y, 0.5f * qhi.z - 0.5f * qlo.z);
        thr = mk(h.x + (scene_term + (fabsf(c.x) + h.x) * kOverlapQuery), h.y + (scene_term + (fabsf(c.y) + h.y) * kOverlapQuery),
                 h.z + (scene_term + (fabsf(c.z) + h.z) * kOverlapQuery));
        qc = mk(c.x - sc.hspace.cx, c.y - sc.hspace.cy, c.z - sc.hspace.cz);
    }
    __device__ __forceinline__ bool admit_hc(uint32_t px, uint32_t py, uint32_t pz, const HSpace& hs) const { return child_admitted_hc(px, py, pz, qc, hs, thr); }
    __device__ __forceinline__ bool admit_f32(float lx, float ly, float lz, float hx, float hy, float hz) const { return child_admitted_f32(qlo, qhi, lx, ly, lz, hx, hy, hz); }
    __device__ __forceinline__ bool accept(const f3& v0, const f3& e1, const f3& e2) const { return tri_tri_intersect(a0, f1, f2, qlo, qhi, v0, e1, e2); }
};

}  // namespace ptd
