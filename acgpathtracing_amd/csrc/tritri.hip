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
// one-dimensional grid, the lane stack of query_launch.h (stack_entries * 64 words per wave), the sorted list in registers.  A query is
// three 16-byte loads per lane.  Lanes past n and lanes whose triangle is a miss before any traversal stay in the wave, inactive.  No
// atomics: two calls give the same bits.
//
// The walk prunes a child box against the query triangle's bounding box (tritri.h says how, per format); the leaves run the 20
// conditions of the triangle-triangle test.  Built with -ffp-contract=off: the test is evaluated as written, and tests/tritri_ref.py
// mirrors it operation for operation.  The child boxes of the fp16 nodes are outside that contract (they only prune) and use explicit
// fused multiply-adds.
#include "tritri.h"
#include "bvh_walk.h"
#include "tritri_device.h"

namespace ptd {

enum { kList = 0, kAny = 1, kVisits = 2 };

// axis_keeps, fold, tri_tri_intersect, the child-box admission of both formats, the sorted register list, the query record TriQuery and
// the walk's policy PrimListWalk: tritri_device.h and overlap_device.h, which lists.hip shares.
//
// One query triangle per lane through the two-child BVH (bvh_walk.h), as overlap.hip walks a box: of two admitted children the first
// is entered and the second pushed.  The boxes only prune: which pairs intersect is decided by tri_tri_intersect alone, whatever order
// the walk reaches them in.

// out8: the any byte per query (kAny).  prims / counts: the list and the number (kList; either may be null), counts alone (kVisits).
template <int FMT, int CAP, int MODE>
__global__ void __launch_bounds__(256)
k_query_triangles(const DeviceScene sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ tris, uint32_t n, uint32_t max_prims,
                  uint32_t* __restrict__ prims, uint32_t* __restrict__ counts, uint8_t* __restrict__ out8, uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    // triangle i of the array, or an inert one for a lane past n.  ok: the lane has a triangle and its nine coordinates are finite
    // (include/acgpt.h: "a miss before any traversal").  The fourth float of each vertex is not looked at.
    TriQuery q;
    const bool ok = q.load(tris, i, n);
    q.prepare(sc, scene_term);
    PrimList<CAP> L;
    PrimListWalk<TriQuery, CAP, MODE == kAny> walk(q, max_prims, L);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, MODE == kVisits>(sc, st, ok, walk, visits);
    const uint32_t count = walk.count;
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
    return launch_lane_stack(k_query_triangles<FMT, CAP, MODE>, stack_entries, n, stream, sc, stack_entries, scene_term, tris, n, max_prims, prims, counts, out8, visits);
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
