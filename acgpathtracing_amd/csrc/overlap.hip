// overlap.hip — the kernels behind pt_query_overlap and pt_query_overlap_any (include/acgpt.h).
//
//   k_query_overlap<FMT, CAP, MODE>   one axis-aligned box per lane from a device array: every triangle the separating-axis test
//                                     accepts.  MODE kList keeps the lowest max_prims indices among them, ascending, in a sorted list
//                                     of CAP = 1, 4 or 8 entries (the smallest that holds max_prims; CAP = 0 carries no list) and
//                                     counts them; kAny leaves at the first accepted triangle and writes one byte; kVisits is the
//                                     counting walk that also writes how many inner nodes the lane visited and how many triangles
//                                     it tested (the test hook's instantiation).
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk prunes by the
// per-axis gap between the query box's centre and each child box, the leaves run the triangle-box test.  256-lane workgroups over a
// one-dimensional grid, the LDS lane stack of query.hip (stack_entries * 64 words per wave).  A box is two 16-byte loads per lane.
// Lanes past n and lanes whose box is a miss before any traversal stay in the wave, inactive.  No atomics: two calls give the same
// bits.
//
// The list lives in registers, as multihit.hip keeps its list: the insertion is a chain of CAP compare-and-swaps, the epilogue
// takes entry 0 and shifts the rest down once per word, so every access has an index the compiler knows.
// Built with -ffp-contract=off: the triangle-box test is evaluated as written, and tests/overlap_ref.py mirrors it operation for
// operation.  The child boxes are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "overlap.h"
#include "overlap_device.h"

namespace ptd {

extern __shared__ uint32_t overlap_lds[];

enum { kList = 0, kAny = 1, kVisits = 2 };

// tri_box_overlap, child_admitted_hc / child_admitted_f32 and the sorted register list (PrimList, list_insert): overlap_device.h,
// which lists.hip shares.

// One box per lane through the two-child BVH.  thr = h + margin per axis (overlap.h): a child is entered iff its gap is at most thr on
// all three axes; of two such children the first is entered and the second pushed.  A visit pushes at most one reference and descends
// one level, so the references on the stack belong to siblings of nodes on the current root-to-node path, at most one per level: the
// depth the ray walks need (size_stack, capi.hip: max_depth + 1) holds here too.  A popped reference is entered without a second look
// at its own box.  The boxes only prune: which triangles overlap is decided by tri_box_overlap alone, whatever order the walk reaches
// them in.
template <int FMT, int CAP, int MODE>
__device__ __forceinline__ void traverse_overlap(const DeviceScene& sc, const LaneStack& st, bool active, const f3& c, const f3& h, float scene_term,
                                                 uint32_t max_prims, PrimList<CAP>& L, uint32_t& count, uint2& visits)
{
#pragma unroll
    for (int j = 0; j < CAP; j++) L.prim[j] = 0xFFFFFFFFu;
    count = 0u;
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
                h0 = child_admitted_f32(c, a.x, a.y, a.z, a.w, b.x, b.y, thr);
                h1 = child_admitted_f32(c, b.z, b.w, cc.x, cc.y, cc.z, cc.w, thr);
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
            const bool ok = tri_box_overlap(c, h, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
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

// out8: the any byte per box (kAny).  prims / counts: the list and the number (kList; either may be null), counts alone (kVisits).
template <int FMT, int CAP, int MODE>
__global__ void __launch_bounds__(256)
k_query_overlap(const DeviceScene sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ boxes, uint32_t n, uint32_t max_prims,
                uint32_t* __restrict__ prims, uint32_t* __restrict__ counts, uint8_t* __restrict__ out8, uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    LaneStack st;
    st.base = overlap_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    // box i of the array, or an inert one for a lane past n.  ok: the lane has a box and the box can overlap something — centre and
    // half extent finite, no half extent negative or NaN (include/acgpt.h: "a miss before any traversal").  -0 is a zero.
    f3 c = mk(0.0f), h = mk(0.0f);
    bool ok = false;
    if (i < n) {
        const float4 a = boxes[2ull * i], b = boxes[2ull * i + 1ull];
        c = mk(a.x, a.y, a.z);
        h = mk(a.w, b.x, b.y);
        ok = __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) && __builtin_isfinite(a.w) && __builtin_isfinite(b.x) &&
             __builtin_isfinite(b.y) && a.w >= 0.0f && b.x >= 0.0f && b.y >= 0.0f;
    }
    PrimList<CAP> L;
    uint32_t count;
    uint2 visits = make_uint2(0u, 0u);
    traverse_overlap<FMT, CAP, MODE>(sc, st, ok, c, h, scene_term, max_prims, L, count, visits);
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
static hipError_t launch_overlap(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                 uint32_t* prims, uint32_t* counts, uint8_t* out8, uint2* visits, hipStream_t stream)
{
    const size_t lds = (size_t)(256 / 64) * stack_entries * 64u * sizeof(uint32_t);
    auto kernel = k_query_overlap<FMT, CAP, MODE>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<(n + 255u) / 256u, 256, lds, stream>>>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, out8, visits);
    return hipGetLastError();
}

template <int FMT>
static hipError_t launch_overlap_fmt(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                     uint32_t* prims, uint32_t* counts, hipStream_t stream)
{
    if (max_prims == 0u) return launch_overlap<FMT, 0, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    if (max_prims == 1u) return launch_overlap<FMT, 1, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    if (max_prims <= 4u) return launch_overlap<FMT, 4, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    return launch_overlap<FMT, 8, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
}

float overlap_scene_term(const float scene_lo[3], const float scene_hi[3])
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) {
        const double a = fabs((double)scene_lo[k]), b = fabs((double)scene_hi[k]);
        if (a > s && a < (double)INFINITY) s = a;
        if (b > s && b < (double)INFINITY) s = b;
    }
    const double t = s * (double)kOverlapScene;
    float f = (float)t;
    if ((double)f < t) f = nextafterf(f, INFINITY);
    return f;
}

hipError_t launch_query_overlap(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                uint32_t* prims, uint32_t* counts, hipStream_t stream)
{
    if (max_prims > kOverlapMaxPrims || (max_prims == 0u && !counts) || ((max_prims != 0u) != (prims != nullptr))) return hipErrorInvalidValue;
    if (fmt == 11) return launch_overlap_fmt<11>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, stream);
    return launch_overlap_fmt<0>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, stream);
}

hipError_t launch_query_overlap_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint8_t* hit,
                                    hipStream_t stream)
{
    if (fmt == 11) return launch_overlap<11, 0, kAny>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, nullptr, hit, nullptr, stream);
    return launch_overlap<0, 0, kAny>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, nullptr, hit, nullptr, stream);
}

hipError_t launch_overlap_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t* counts,
                                 uint2* visits, hipStream_t stream)
{
    if (fmt == 11) return launch_overlap<11, 0, kVisits>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, counts, nullptr, visits, stream);
    return launch_overlap<0, 0, kVisits>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, counts, nullptr, visits, stream);
}

}  // namespace ptd
