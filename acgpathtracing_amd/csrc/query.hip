// query.hip — the kernels behind pt_query_closest and pt_query_any (include/acgpt.h).
//
//   k_query_closest<FMT>   one ray per lane from a device array: closest hit, then the hit record (t, triangle, barycentrics, unit
//                          normal towards the ray's origin, material)
//   k_query_any<FMT>       one ray per lane: one byte, 1 if any triangle is hit inside the interval
//
// FMT 11 walks the fp16 centre / half-extent nodes (traverse_hc.h), FMT 0 the fp32 nodes (traverse<>, pt_device.h): the node array the
// scene holds.  256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h (stack_entries * 64 words per
// wave).  A ray is two 16-byte loads and a record two 16-byte stores per lane, 64 B each way; everything else is the traversal.  Lanes
// past n and lanes whose ray is a miss before any traversal stay in the wave, inactive.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the epilogue is evaluated as written, and tests/query_ref.py mirrors it operation for operation.
#include "query.h"
#include "query_launch.h"
#include "traverse_hc.h"

namespace ptd {

struct QueryRay { f3 o, d; float tmin, tmax; bool ok; };

// Ray i of the array, or an inert one for a lane past n.  ok: the lane has a ray and the ray can hit something — every origin and
// direction component finite, tmin and tmax no NaN, tmax > tmin (include/acgpt.h: "a miss before any traversal").
__device__ __forceinline__ QueryRay load_query_ray(const float4* __restrict__ rays, uint32_t i, uint32_t n)
{
    QueryRay r;
    r.o = mk(0.0f); r.d = mk(0.0f, 0.0f, 1.0f); r.tmin = 0.0f; r.tmax = 0.0f; r.ok = false;
    if (i < n) {
        const float4 a = rays[2ull * i], b = rays[2ull * i + 1ull];
        r.o = mk(a.x, a.y, a.z); r.d = mk(a.w, b.x, b.y); r.tmin = b.z; r.tmax = b.w;
        const bool finite = __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) && __builtin_isfinite(a.w) &&
                            __builtin_isfinite(b.x) && __builtin_isfinite(b.y);
        r.ok = finite && r.tmax > r.tmin;      // false when either is a NaN
    }
    return r;
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_closest(const DeviceScene sc, uint32_t stack_entries, const float4* __restrict__ rays, uint32_t n, float4* __restrict__ hits)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    const QueryRay r = load_query_ray(rays, i, n);
    HitRec hit;
    if (FMT == 11) traverse_hc(sc, st, r.ok, r.o, r.d, r.tmin, r.tmax, hit);
    else traverse<false>(sc, st, r.ok, r.o, r.d, r.tmin, r.tmax, hit);
    if (i >= n) return;
    float4 h0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), h1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (r.ok && hit.slot >= 0) {
        // barycentrics of v1 and v2 once more, in plain multiplies and adds (tri_test's are fused): Moeller-Trumbore as include/acgpt.h writes it
        const TriRecord* tp = sc.tris + hit.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
        const f3 v0 = mk(r0.x, r0.y, r0.z), e1 = mk(r0.w, r1.x, r1.y), e2 = mk(r1.z, r1.w, r2.x);
        const f3 p = cross(r.d, e2);
        const float det = dot(e1, p);
        const f3 s = r.o - v0;
        const float u = dot(s, p) / det;
        const f3 q = cross(s, e1);
        const float v = dot(r.d, q) / det;
        const float4 sr = sc.shade[hit.slot];          // normalize(cross(e1, e2)) and the material id (pt_device.h)
        f3 nrm = mk(sr.x, sr.y, sr.z);
        if (dot(nrm, r.d) > 0.0f) nrm = -nrm;          // towards the ray's origin
        h0 = make_float4(hit.t, __uint_as_float(hit.prim), u, v);
        h1 = make_float4(nrm.x, nrm.y, nrm.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
    }
    hits[2ull * i] = h0;
    hits[2ull * i + 1ull] = h1;
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_any(const DeviceScene sc, uint32_t stack_entries, const float4* __restrict__ rays, uint32_t n, uint8_t* __restrict__ occluded)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    const QueryRay r = load_query_ray(rays, i, n);
    bool found;
    if (FMT == 11) found = traverse_hc_any(sc, st, r.ok, r.o, r.d, r.tmin, r.tmax);
    else { HitRec hit; found = traverse<true>(sc, st, r.ok, r.o, r.d, r.tmin, r.tmax, hit); }
    if (i < n) occluded[i] = found ? 1 : 0;
}

hipError_t launch_query_closest(int fmt, const DeviceScene& sc, uint32_t stack_entries, const float4* rays, uint32_t n, float4* hits, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_closest<11>, stack_entries, n, stream, sc, stack_entries, rays, n, hits);
    return launch_lane_stack(k_query_closest<0>, stack_entries, n, stream, sc, stack_entries, rays, n, hits);
}

hipError_t launch_query_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, const float4* rays, uint32_t n, uint8_t* occluded, hipStream_t stream)
{
    if (fmt == 11) return launch_lane_stack(k_query_any<11>, stack_entries, n, stream, sc, stack_entries, rays, n, occluded);
    return launch_lane_stack(k_query_any<0>, stack_entries, n, stream, sc, stack_entries, rays, n, occluded);
}

}  // namespace ptd
