// traverse_hc.h — one ray per lane through the fp16 centre / half-extent nodes (NODE_FMT 11, sc.hcnodes) outside the render kernels'
// fused loop: the closest-hit walk of k_dn_features (denoise.hip) and k_query_closest (query.hip), and the any-hit walk of
// k_query_any.  The box test of the default render kernels (setup_ray_hc / slab_hc), the LDS lane stack of traverse().  No render
// kernel includes this file: it is not part of pt_kernel_source_hash.
#pragma once
#include "pt_device.h"

namespace ptd {

// Closest hit.  Boxes only prune; the triangle test, the interval (tmin, tmax) and the tie rule (equal t -> lowest triangle index) are
// those of traverse<false>, so the hit triangle and t equal pt_trace_closest's bit for bit.
__device__ __forceinline__ void traverse_hc(const DeviceScene& sc, const LaneStack& st, bool active, const f3& o, const f3& d, float tmin, float tmax,
                                            HitRec& hit)
{
    hit.t = tmax; hit.slot = -1; hit.prim = 0xFFFFFFFFu;
    f3 mul, add;
    setup_ray_hc(o, d, sc.hspace, mul, add);
    int sp = 0;
    int node = (active && sc.n_tris != 0u) ? 0 : kSentinel;
    while (node != kSentinel) {
        if (node >= 0) {
            // child references of inner nodes are byte offsets into hcnodes; a leaf is ~slot
            const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
            const uint4 qa = np[0], qb = np[1];
            float n0, f0, n1, f1;
            slab_hc(qa.x, qa.y, qa.z, mul, add, tmin, n0, f0);
            slab_hc(qb.x, qb.y, qb.z, mul, add, tmin, n1, f1);
            f0 = fminf(f0, hit.t * kTieWiden);
            f1 = fminf(f1, hit.t * kTieWiden);
            const bool h0 = n0 <= f0, h1 = n1 <= f1;
            if (h0 && h1) {
                const bool first0 = n0 <= n1;
                st.push(sp, first0 ? (int)qb.w : (int)qa.w);
                sp++;
                node = first0 ? (int)qa.w : (int)qb.w;
            } else if (h0) {
                node = (int)qa.w;
            } else if (h1) {
                node = (int)qb.w;
            } else {
                if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
            }
        } else {
            const int slot = ~node;
            const TriRecord* tp = sc.tris + slot;
            const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
            float t;
            const bool ok = tri_test(o, d, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x), tmin, tmax, t);
            const uint32_t prim = __float_as_uint(r2.y);
            if (ok && (t < hit.t || (t == hit.t && prim < hit.prim))) { hit.t = t; hit.slot = slot; hit.prim = prim; }
            if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
}

// Any hit: true if some triangle passes tri_test inside (tmin, tmax).  The same box test; the far side is cut at the ray's own tmax
// (widened as traverse<true> widens it) and never at a hit, because the first accepted triangle ends the walk.  Which triangle that
// is depends on the order of the walk; whether there is one does not: the boxes are conservative, so every triangle that
// traverse<true> can accept is reached here too, and the answer equals pt_trace_any's.
__device__ __forceinline__ bool traverse_hc_any(const DeviceScene& sc, const LaneStack& st, bool active, const f3& o, const f3& d, float tmin, float tmax)
{
    f3 mul, add;
    setup_ray_hc(o, d, sc.hspace, mul, add);
    const float far_cut = fmaxf(tmax * kTieWiden, tmax);      // tmax < 0: the product would move the cut inward
    int sp = 0;
    int node = (active && sc.n_tris != 0u) ? 0 : kSentinel;
    bool found = false;
    while (node != kSentinel) {
        if (node >= 0) {
            const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
            const uint4 qa = np[0], qb = np[1];
            float n0, f0, n1, f1;
            slab_hc(qa.x, qa.y, qa.z, mul, add, tmin, n0, f0);
            slab_hc(qb.x, qb.y, qb.z, mul, add, tmin, n1, f1);
            f0 = fminf(f0, far_cut);
            f1 = fminf(f1, far_cut);
            const bool h0 = n0 <= f0, h1 = n1 <= f1;
            if (h0 && h1) {
                const bool first0 = n0 <= n1;
                st.push(sp, first0 ? (int)qb.w : (int)qa.w);
                sp++;
                node = first0 ? (int)qa.w : (int)qb.w;
            } else if (h0) {
                node = (int)qa.w;
            } else if (h1) {
                node = (int)qb.w;
            } else {
                if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
            }
        } else {
            const TriRecord* tp = sc.tris + ~node;
            const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
            float t;
            if (tri_test(o, d, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x), tmin, tmax, t)) { found = true; node = kSentinel; }
            else if (sp == 0) node = kSentinel;
            else { sp--; node = st.pop(sp); }
        }
    }
    return found;
}

}  // namespace ptd
