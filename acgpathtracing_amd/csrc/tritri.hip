// tritri.hip — the kernels behind pt_query_triangles and pt_query_triangles_any (include/acgpt.h).
//
//   k_query_triangles<FMT, CAP, MODE>   one query triangle per lane from a device array: every scene triangle the separating-axis test
//                                       accepts.  MODE kList keeps the lowest max_prims indices among them, ascending, in a sorted list
//                                       of CAP = 1, 4 or 8 entries (the smallest that holds max_prims; CAP = 0 carries no list) and
//                                       counts them; kAny leaves at the first accepted triangle and writes one byte; kVisits is the
//                                       counting walk that also writes how many inner nodes the lane visited and how many triangles
//                                       it tested (the test hook's instantiation).
//
// The shape is overlap.hip's: FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes; 256-lane workgroups over a
// one-dimensional grid, the LDS lane stack of query.hip (stack_entries * 64 words per wave), the sorted list in registers.  A query is
// three 16-byte loads per lane.  Lanes past n and lanes whose triangle is a miss before any traversal stay in the wave, inactive.  No
// atomics: two calls give the same bits.
//
// The walk prunes a child box against the query triangle's bounding box (tritri.h says how, per format); the leaves run the 20
// conditions of the triangle-triangle test.  Built with -ffp-contract=off: the test is evaluated as written, and tests/tritri_ref.py
// mirrors it operation for operation.  The child boxes of the fp16 nodes are outside that contract (they only prune) and use explicit
// fused multiply-adds.
#include "tritri.h"
#include "tritri_device.h"

namespace ptd {

extern __shared__ uint32_t tritri_lds[];

enum { kList = 0, kAny = 1, kVisits = 2 };

// axis_keeps, fold, tri_tri_intersect, the child-box admission of both formats and the sorted register list: tritri_device.h,
// which lists.hip shares.

// One query triangle per lane through the two-child BVH, as traverse_overlap walks a box: of two admitted children the first is
// entered and the second pushed, so a visit pushes at most one reference per level and max_depth + 1 stack entries suffice; a popped
// reference is entered without a second look at its own box.  The boxes only prune: which pairs intersect is decided by
// tri_tri_intersect alone, whatever order the walk reaches them in.
template <int FMT, int CAP, int MODE>
__device__ __forceinline__ void traverse_triangles(const DeviceScene& sc, const LaneStack& st, bool active, const f3& a0, const f3& f1, const f3& f2, const f3& qlo,
                                                   const f3& qhi, float scene_term, uint32_t max_prims, PrimList<CAP>& L, uint32_t& count, uint2& visits)
{
#pragma unroll
    for (int j = 0; j < CAP; j++) L.prim[j] = 0xFFFFFFFFu;
    count = 0u;
    // FMT 11 only: the query box as centre and half extent (the halves are exact, the sum and the difference round once each)
    const f3 c = mk(0.5f * qlo.x + 0.5f * qhi.x, 0.5f * qlo.y + 0.5f * qhi.y, 0.5f * qlo.z + 0.5f * qhi.z);
    const f3 h = mk(0.5f * qhi.x - 0.5f * qlo.x, 0.5f * qhi.y - 0.5f * qlo.y, 0.5f * qhi.z - 0.5f * qlo.z);
    const f3 thr = mk(h.x + (scene_term + (fabsf(c.x) + h.x) * kOverlapQuery), h.y + (scene_term + (fabsf(c.y) + h.y) * kOverlapQuery),
                      h.z + (scene_term + (fabsf(c.z) + h.z) * kOverlapQuery));
    const f3 qc = mk(c.x - sc.hspace.cx, c.y - sc.hspace.cy, c.z - sc.hspace.cz);
    int sp = 0;
    int node = (active && sc.n_tris != 0u) ? 0 : kSentinel;
    while (node != kSentinel) {
        if (node >= 0) {
            bool h0, h1;
            int c0, c1;
            if (FMT == 11) {
                // child references of inner nodes are byte offsets into hcnodes; a leaf is ~slot
                const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
                const uint4 qa = np[0], qb = np[1];
                h0 = child_admitted_hc(qa.x, qa.y, qa.z, qc, sc.hspace, thr);
                h1 = child_admitted_hc(qb.x, qb.y, qb.z, qc, sc.hspace, thr);
                c0 = (int)qa.w; c1 = (int)qb.w;
            } else {
                // child 0: lo (a.x a.y a.z) hi (a.w b.x b.y); child 1: lo (b.z b.w c.x) hi (c.y c.z c.w)
                const BvhNode* np = sc.nodes + node;
                const float4 a = np->a, b = np->b, cc = np->c;
                const int4 ch = np->d;
                h0 = child_admitted_f32(qlo, qhi, a.x, a.y, a.z, a.w, b.x, b.y);
                h1 = child_admitted_f32(qlo, qhi, b.z, b.w, cc.x, cc.y, cc.z, cc.w);
                c0 = ch.x; c1 = ch.y;
            }
            if (MODE == kVisits) visits.x++;
            if (h0 && h1) {
                st.push(sp, c1);
                sp++;
                node = c0;
            } else if (h0) {
                node = c0;
            } else if (h1) {
                node = c1;
            } else {
                if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
            }
        } else {
            const int slot = ~node;
            const TriRecord* tp = sc.tris + slot;
            const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
            const bool ok = tri_tri_intersect(a0, f1, f2, qlo, qhi, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
            if (MODE == kVisits) visits.y++;
            if (ok) {
                count++;
                if (MODE == kAny) { node = kSentinel; continue; }
                if constexpr (CAP > 0) list_insert(L, max_prims, __float_as_uint(r2.y));
            }
            if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
}

// out8: the any byte per query (kAny).  prims / counts: the list and the number (kList; either may be null), counts alone (kVisits).
template <int FMT, int CAP, int MODE>
__global__ void __launch_bounds__(256)
k_query_triangles(const DeviceScene sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ tris, uint32_t n, uint32_t max_prims,
                  uint32_t* __restrict__ prims, uint32_t* __restrict__ counts, uint8_t* __restrict__ out8, uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    LaneStack st;
    st.base = tritri_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    // triangle i of the array, or an inert one for a lane past n.  ok: the lane has a triangle and its nine coordinates are finite
    // (include/acgpt.h: "a miss before any traversal").  The fourth float of each vertex is not looked at.
    f3 a0 = mk(0.0f), a1 = mk(0.0f), a2 = mk(0.0f);
    bool ok = false;
    if (i < n) {
        const float4 r0 = tris[3ull * i], r1 = tris[3ull * i + 1ull], r2 = tris[3ull * i + 2ull];
        a0 = mk(r0.x, r0.y, r0.z);
        a1 = mk(r1.x, r1.y, r1.z);
        a2 = mk(r2.x, r2.y, r2.z);
        ok = __builtin_isfinite(r0.x) && __builtin_isfinite(r0.y) && __builtin_isfinite(r0.z) && __builtin_isfinite(r1.x) && __builtin_isfinite(r1.y) &&
             __builtin_isfinite(r1.z) && __builtin_isfinite(r2.x) && __builtin_isfinite(r2.y) && __builtin_isfinite(r2.z);
    }
    const f3 qlo = mk(fmin3(a0.x, a1.x, a2.x), fmin3(a0.y, a1.y, a2.y), fmin3(a0.z, a1.z, a2.z));
    const f3 qhi = mk(fmax3(a0.x, a1.x, a2.x), fmax3(a0.y, a1.y, a2.y), fmax3(a0.z, a1.z, a2.z));
    PrimList<CAP> L;
    uint32_t count;
    uint2 visits = make_uint2(0u, 0u);
    traverse_triangles<FMT, CAP, MODE>(sc, st, ok, a0, a1 - a0, a2 - a0, qlo, qhi, scene_term, max_prims, L, count, visits);
    if (i >= n) return;
    if (MODE == kAny) { out8[i] = count != 0u ? 1 : 0; return; }
    if (counts) counts[i] = count;
    if (MODE == kVisits) visits_out[i] = visits;
    if constexpr (CAP > 0) {
        uint32_t* out = prims + (unsigned long long)i * max_prims;      // n * max_prims is formed in 64 bits
#pragma unroll 1
        for (uint32_t j = 0; j < max_prims; j++) {
            // the next word is entry 0; the rest move down one, so that no index depends on j
            out[j] = L.prim[0];
#pragma unroll
            for (int k = 0; k + 1 < CAP; k++) L.prim[k] = L.prim[k + 1];
            L.prim[CAP - 1] = 0xFFFFFFFFu;
        }
    }
}

template <int FMT, int CAP, int MODE>
static hipError_t launch_triangles(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, uint32_t max_prims,
                                   uint32_t* prims, uint32_t* counts, uint8_t* out8, uint2* visits, hipStream_t stream)
{
    const size_t lds = (size_t)(256 / 64) * stack_entries * 64u * sizeof(uint32_t);
    auto kernel = k_query_triangles<FMT, CAP, MODE>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<(n + 255u) / 256u, 256, lds, stream>>>(sc, stack_entries, scene_term, tris, n, max_prims, prims, counts, out8, visits);
    return hipGetLastError();
}

template <int FMT>
static hipError_t launch_triangles_fmt(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, uint32_t max_prims,
                                       uint32_t* prims, uint32_t* counts, hipStream_t stream)
{
    if (max_prims == 0u) return launch_triangles<FMT, 0, kList>(sc, stack_entries, scene_term, tris, n, max_prims, prims, counts, nullptr, nullptr, stream);
    if (max_prims == 1u) return launch_triangles<FMT, 1, kList>(sc, stack_entries, scene_term, tris, n, max_prims, prims, counts, nullptr, nullptr, stream);
    if (max_prims <= 4u) return launch_triangles<FMT, 4, kList>(sc, stack_entries, scene_term, tris, n, max_prims, prims, counts, nullptr, nullptr, stream);
    return launch_triangles<FMT, 8, kList>(sc, stack_entries, scene_term, tris, n, max_prims, prims, counts, nullptr, nullptr, stream);
}

hipError_t launch_query_triangles(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, uint32_t max_prims,
                                  uint32_t* prims, uint32_t* counts, hipStream_t stream)
{
    if (max_prims > kTrianglesMaxPrims || (max_prims == 0u && !counts) || ((max_prims != 0u) != (prims != nullptr))) return hipErrorInvalidValue;
    if (fmt == 11) return launch_triangles_fmt<11>(sc, stack_entries, scene_term, tris, n, max_prims, prims, counts, stream);
    return launch_triangles_fmt<0>(sc, stack_entries, scene_term, tris, n, max_prims, prims, counts, stream);
}

hipError_t launch_query_triangles_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, uint8_t* hit,
                                      hipStream_t stream)
{
    if (fmt == 11) return launch_triangles<11, 0, kAny>(sc, stack_entries, scene_term, tris, n, 0u, nullptr, nullptr, hit, nullptr, stream);
    return launch_triangles<0, 0, kAny>(sc, stack_entries, scene_term, tris, n, 0u, nullptr, nullptr, hit, nullptr, stream);
}

hipError_t launch_triangles_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, uint32_t* counts,
                                   uint2* visits, hipStream_t stream)
{
    if (fmt == 11) return launch_triangles<11, 0, kVisits>(sc, stack_entries, scene_term, tris, n, 0u, nullptr, counts, nullptr, visits, stream);
    return launch_triangles<0, 0, kVisits>(sc, stack_entries, scene_term, tris, n, 0u, nullptr, counts, nullptr, visits, stream);
}

}  // namespace ptd
