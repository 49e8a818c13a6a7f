// tricast.hip — the kernels behind pt_query_triangle_cast, pt_query_triangle_cast_any and pt_query_poses_cast (include/acgpt.h).
//
//   k_query_triangle_cast<FMT, COUNT>   one translating triangle per lane from a device array: the scene triangle with the smallest
//                                       time of impact within [0, tmax], then the record (t, triangle, feature, contact, material).
//                                       COUNT also writes how many inner nodes the lane visited and how many triangles it tested
//                                       (the test hook's instantiation).
//   k_query_triangle_cast_any<FMT>      one byte per cast; a lane leaves the walk at its first triangle with a time of impact
//                                       within [0, tmax].
//   k_cast_pose<FMT>                    phase 1 of the posed call, one lane per (pose, mesh triangle): the lane transforms its
//                                       triangle in registers, walks as k_query_triangle_cast does (the same walk) and fetch_mins
//                                       (bits of t) << 32 | mesh triangle into the pose's 64-bit key.
//   k_cast_pose_record<FMT>             phase 2, one lane per pose: the winning triangle transformed again, k_query_triangle_cast's
//                                       own walk and epilogue for it with the full tmax, the record written with query_triangle.
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk, the any-hit
// kernel and the record kernel's frame are cast_walk.h's; what is this unit's own (the leaf statement cast_pair, the centre line of
// the query's box, the inflation and the cut of tricast.h) is in tricast_device.h.  A cast is four 16-byte loads and a record two
// 16-byte stores per lane.  The per-triangle kernels use no atomics: two calls give the same bits.
//
// The posed kernels follow poses.hip's k_pose_distance and k_pose_record.  The transform is include/acgpt.h's statement, x' = ((m[0] x
// + m[1] y) + m[2] z) + m[3] per row, every operation on its own, so the posed vertices are pt_pose_triangles' bits.  The per-pose keys
// are the only memory that lanes of different workgroups share inside a launch; they are touched by agent-scope relaxed atomic loads
// and fetch_min alone, filled before the launch and read plainly only by the next kernel on the stream.  No lane waits for another.
// Before walking, a lane reads its pose's key and walks with tmax = min(tmax, t of the key); it stays out if the key holds t = 0 from a
// lower index.  The look is a hint whose only effect is less work: the key ends as the minimum of (t, triangle) over all candidates
// whatever the schedule.  A lane whose true t exceeds the shrunken tmax cannot win (a key with a smaller t is already there), a lane
// whose t equals it is still a candidate (t <= tmax), so a lower index still wins the tie, and a lane that finds its t under a
// smaller tmax finds the same t.  The key orders exactly as (t, triangle) does: a candidate's t is never a NaN, never negative and
// never -0 (the statement's + 0), so its bits order as an unsigned integer and stay below the all-ones of an empty key.
// Built with -ffp-contract=off: the time of impact is evaluated as written, and tests/tricast_ref.py mirrors it operation for
// operation.
#include "tricast.h"
#include "tricast_device.h"
#include "poses.h"

namespace ptd {

template <int FMT, bool COUNT>
__global__ void __launch_bounds__(256)
k_query_triangle_cast(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, float4* __restrict__ out,
                      uint2* __restrict__ visits_out)
{
    cast_record_body<FMT, COUNT, CastQuery, const CastQuery&>(sc, stack_entries, scene_scale, casts, n, visits_out,
                                                              [&](uint32_t i, const CastQuery& q, bool found, const TriCastWalk& best) {
        float4 o0, o1;
        cast_record(sc, q, found, best, 0u, o0, o1);
        out[2ull * i] = o0;
        out[2ull * i + 1ull] = o1;
    });
}

template <int FMT>
__global__ void __launch_bounds__(256)
k_query_triangle_cast_any(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ casts, uint32_t n, uint8_t* __restrict__ blocked)
{
    cast_any_body<FMT, CastQuery, const CastQuery&>(sc, stack_entries, scene_scale, casts, n, blocked);
}

// ---- the posed call ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f3 cast_pose_point(const float4& m0, const float4& m1, const float4& m2, float x, float y, float z)
{
    return mk(((m0.x * x + m0.y * y) + m0.z * z) + m0.w, ((m1.x * x + m1.y * y) + m1.z * z) + m1.w, ((m2.x * x + m2.y * y) + m2.z * z) + m2.w);
}

// mesh triangle t under pose p with motions[p] as the lane's cast.  The fourth floats of the mesh records are loaded with their
// float4 and never used.  False: the cast is a miss before any traversal.
__device__ __forceinline__ bool cast_pose_query(CastQuery& q, const float4* __restrict__ mesh, uint32_t t, const float4* __restrict__ poses,
                                                const float4* __restrict__ motions, uint32_t p, bool have)
{
    const float4 m0 = poses[3ull * p], m1 = poses[3ull * p + 1ull], m2 = poses[3ull * p + 2ull];
    const float4 g0 = mesh[3ull * t], g1 = mesh[3ull * t + 1ull], g2 = mesh[3ull * t + 2ull];
    const float4 mo = motions[p];
    return q.set(cast_pose_point(m0, m1, m2, g0.x, g0.y, g0.z), cast_pose_point(m0, m1, m2, g1.x, g1.y, g1.z), cast_pose_point(m0, m1, m2, g2.x, g2.y, g2.z),
                 mk(mo.x, mo.y, mo.z), mo.w, have);
}

// keys[p]: all ones before the launch.  A lane past n takes the last pair's data and stays inactive.  Lane j < P * T as (pose, mesh
// triangle): triangle-major (all poses' triangle 0 first: later workgroups find most poses already cut short), or pose-major under
// kPosePoseMajor; which of the two changes no output bit.
template <int FMT>
__global__ void __launch_bounds__(256)
k_cast_pose(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ mesh, uint32_t T, const float4* __restrict__ poses,
            const float4* __restrict__ motions, uint32_t P, uint32_t n, unsigned long long* keys, uint32_t flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    const uint32_t j = i < n ? i : n - 1u;
    uint32_t p, t;
    if (flags & kPosePoseMajor) { p = j / T; t = j - p * T; }
    else { t = j / P; p = j - t * P; }
    CastQuery q;
    bool ok = cast_pose_query(q, mesh, t, poses, motions, p, i < n);
    float tmax = q.tmax;
    if (!(flags & kPoseNoEarly)) {
        const unsigned long long key = __hip_atomic_load(keys + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (key != ~0ull) {
            const float kt = __uint_as_float((uint32_t)(key >> 32));      // a candidate's t: no NaN, not negative
            tmax = fminf(tmax, kt);
            if (kt == 0.0f && (uint32_t)key < t) ok = false;                // nothing is below (0, a lower index)
        }
    }
    q.line<FMT>(scene_scale, sc.hspace);
    TriCastWalk best(q, tmax);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, best, visits);
    if (ok && best.slot >= 0)
        __hip_atomic_fetch_min(keys + p, ((unsigned long long)__float_as_uint(best.t) << 32) | t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per pose.  Phase 1 has ended: the keys are read as they are.  A pose with an empty key gets the miss record.
template <int FMT>
__global__ void __launch_bounds__(256)
k_cast_pose_record(const DeviceScene sc, uint32_t stack_entries, float scene_scale, const float4* __restrict__ mesh, const float4* __restrict__ poses,
                   const float4* __restrict__ motions, uint32_t P, const unsigned long long* __restrict__ keys, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    const uint32_t p = i < P ? i : P - 1u;
    const unsigned long long key = keys[p];
    const bool found = key != ~0ull && i < P;
    const uint32_t t = found ? (uint32_t)key : 0u;
    CastQuery q;
    const bool ok = cast_pose_query(q, mesh, t, poses, motions, p, found);
    q.line<FMT>(scene_scale, sc.hspace);
    TriCastWalk best(q, q.tmax);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, best, visits);
    if (i >= P) return;
    float4 o0, o1;
    const bool found_one = ok && best.slot >= 0;
    cast_record(sc, q, found_one, best, found_one ? t : 0xFFFFFFFFu, o0, o1);
    out[2ull * i] = o0;
    out[2ull * i + 1ull] = o1;
}

hipError_t launch_query_triangle_cast(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                      hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) {
        return launch_cast(k_query_triangle_cast<decltype(F)::value, false>, sc, stack_entries, scene_scale, casts, n, stream, out, (uint2*)nullptr);
    });
}

hipError_t launch_query_triangle_cast_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n,
                                          uint8_t* blocked, hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) { return launch_cast(k_query_triangle_cast_any<decltype(F)::value>, sc, stack_entries, scene_scale, casts, n, stream, blocked); });
}

hipError_t launch_triangle_cast_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* casts, uint32_t n, float4* out,
                                       uint2* visits, hipStream_t stream)
{
    return dispatch_format(fmt, [&](auto F) { return launch_cast(k_query_triangle_cast<decltype(F)::value, true>, sc, stack_entries, scene_scale, casts, n, stream, out, visits); });
}

hipError_t launch_poses_cast(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_scale, const float4* mesh, uint32_t T, const float4* poses,
                             const float4* motions, uint32_t P, unsigned long long* keys, float4* out, uint32_t flags, hipStream_t stream)
{
    const uint32_t n = P * T;      // <= 2^31 - 1 (capi_query.hip)
    hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)P * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    return dispatch_format(fmt, [&](auto F) {
        const hipError_t e1 = launch_lane_stack(k_cast_pose<decltype(F)::value>, stack_entries, n, stream, sc, stack_entries, scene_scale, mesh, T, poses, motions, P, n, keys, flags);
        if (e1 != hipSuccess) return e1;
        return launch_lane_stack(k_cast_pose_record<decltype(F)::value>, stack_entries, P, stream, sc, stack_entries, scene_scale, mesh, poses, motions, P, (const unsigned long long*)keys, out);
    });
}

}  // namespace ptd
