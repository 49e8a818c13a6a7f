// oriented.hip — the kernels behind pt_query_overlap_oriented, pt_query_overlap_oriented_any and pt_pose_boxes (include/acgpt.h).
//
//   k_query_oriented<FMT, CAP, MODE>   one oriented box per lane from a device array: every triangle the statement accepts — the
//                                      triangle's stored vectors taken into the box's frame by nine dot products, then the 13 conditions
//                                      of the axis-aligned test about the origin (tri_box_overlap, overlap_device.h, as it is).  The
//                                      modes, the list sizes and the epilogue are k_query_overlap's (overlap.hip).  CROSS is false in every
//                                      kernel of the product; the two counting walks with it set are the other arm of the admission's
//                                      measurement (oriented_device.h).
//   k_posed_boxes                       one pose per lane: the pose with its fourth column replaced by the posed local centre, and the
//                                      half extent behind it.  Plain vector stores.
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes.  The walk prunes on six axes — the three world axes against the
// box's world half extent, the three box axes against the child box's radius along them (oriented.h derives the margin) —, the leaves
// run the statement.  256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h.  A box is four 16-byte loads
// per lane.  Lanes past n and lanes whose box is a miss before any traversal stay in the wave, inactive.  No atomics: two calls give
// the same bits.  Built with -ffp-contract=off: the statement is evaluated as written, and tests/oriented_ref.py mirrors it operation
// for operation.
#include "oriented.h"
#include "bvh_walk.h"
#include "oriented_device.h"

namespace ptd {

enum { kList = 0, kAny = 1, kVisits = 2 };

// out8: the any byte per box (kAny).  prims / counts: the list and the number (kList; either may be null), counts alone (kVisits).
template <int FMT, int CAP, int MODE, bool CROSS>
__global__ void __launch_bounds__(256)
k_query_oriented(const DeviceScene sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ boxes, uint32_t n, uint32_t max_prims,
                 uint32_t* __restrict__ prims, uint32_t* __restrict__ counts, uint8_t* __restrict__ out8, uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    // box i of the array, or an inert one for a lane past n.  ok: the lane has a box and the box can overlap something (include/acgpt.h:
    // "a miss before any traversal")
    OBoxQueryT<CROSS> q;
    const bool ok = q.load(boxes, i, n);
    q.prepare(sc, scene_term);
    PrimList<CAP> L;
    PrimListWalk<OBoxQueryT<CROSS>, CAP, MODE == kAny> walk(q, max_prims, L);
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

// The pose statement of include/acgpt.h on the local centre: every multiply and add on its own, in that order.
__global__ void __launch_bounds__(256)
k_posed_boxes(const float4* __restrict__ poses, uint32_t P, float cx, float cy, float cz, float hx, float hy, float hz, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // P <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    if (i >= P) return;
    const float4 m0 = poses[3ull * i], m1 = poses[3ull * i + 1ull], m2 = poses[3ull * i + 2ull];
    out[4ull * i] = make_float4(m0.x, m0.y, m0.z, ((m0.x * cx + m0.y * cy) + m0.z * cz) + m0.w);
    out[4ull * i + 1ull] = make_float4(m1.x, m1.y, m1.z, ((m1.x * cx + m1.y * cy) + m1.z * cz) + m1.w);
    out[4ull * i + 2ull] = make_float4(m2.x, m2.y, m2.z, ((m2.x * cx + m2.y * cy) + m2.z * cz) + m2.w);
    out[4ull * i + 3ull] = make_float4(hx, hy, hz, 0.0f);
}

template <int FMT, int CAP, int MODE, bool CROSS = false>
static hipError_t launch_oriented(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                  uint32_t* prims, uint32_t* counts, uint8_t* out8, uint2* visits, hipStream_t stream)
{
    return launch_lane_stack(k_query_oriented<FMT, CAP, MODE, CROSS>, stack_entries, n, stream, sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, out8, visits);
}

template <int FMT>
static hipError_t launch_oriented_fmt(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                      uint32_t* prims, uint32_t* counts, hipStream_t stream)
{
    if (max_prims == 0u) return launch_oriented<FMT, 0, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    if (max_prims == 1u) return launch_oriented<FMT, 1, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    if (max_prims <= 4u) return launch_oriented<FMT, 4, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    return launch_oriented<FMT, 8, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
}

float oriented_scene_term(const float scene_lo[3], const float scene_hi[3])
{
    return round_up_to_float((double)scene_max_abs(scene_lo, scene_hi) * (double)kOBoxScene);
}

hipError_t launch_query_oriented(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                 uint32_t* prims, uint32_t* counts, hipStream_t stream)
{
    if (n == 0u || n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    if (max_prims > kOverlapMaxPrims || (max_prims == 0u && !counts) || ((max_prims != 0u) != (prims != nullptr))) return hipErrorInvalidValue;
    if (fmt == 11) return launch_oriented_fmt<11>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, stream);
    return launch_oriented_fmt<0>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, stream);
}

hipError_t launch_query_oriented_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint8_t* hit,
                                     hipStream_t stream)
{
    if (n == 0u || n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    if (fmt == 11) return launch_oriented<11, 0, kAny>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, nullptr, hit, nullptr, stream);
    return launch_oriented<0, 0, kAny>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, nullptr, hit, nullptr, stream);
}

hipError_t launch_oriented_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t* counts,
                                  uint2* visits, bool cross, hipStream_t stream)
{
    if (n == 0u || n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    if (cross) {
        if (fmt == 11) return launch_oriented<11, 0, kVisits, true>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, counts, nullptr, visits, stream);
        return launch_oriented<0, 0, kVisits, true>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, counts, nullptr, visits, stream);
    }
    if (fmt == 11) return launch_oriented<11, 0, kVisits>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, counts, nullptr, visits, stream);
    return launch_oriented<0, 0, kVisits>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, counts, nullptr, visits, stream);
}

hipError_t launch_pose_boxes(const float4* poses, uint32_t P, float cx, float cy, float cz, float hx, float hy, float hz, float4* out, hipStream_t stream)
{
    if (P == 0u || P > 0x7FFFFFFFu) return hipErrorInvalidValue;
    k_posed_boxes<<<(P + 255u) / 256u, 256, 0, stream>>>(poses, P, cx, cy, cz, hx, hy, hz, out);
    return hipGetLastError();
}

}  // namespace ptd
