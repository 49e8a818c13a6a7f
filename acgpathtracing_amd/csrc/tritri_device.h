// tritri_device.h — the device functions the triangle-against-mesh query (tritri.hip) shares with the complete-list queries
// (lists.hip): the triangle-triangle test and the child-box admission of the fp32 nodes.  fmin3 / fmax3, child_admitted_hc (the fp16
// nodes' admission, the same for a box and for a triangle's bounding box) and the sorted register list come from overlap_device.h.
// Moved out of tritri.hip word for word; include only from a unit built with -ffp-contract=off (the test is evaluated as written, and
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

}  // namespace ptd
