// poses.hip — the kernels behind pt_pose_triangles, pt_query_poses_any and pt_query_poses_distance (include/acgpt.h).
//
//   k_pose_triangles            one lane per (pose, mesh triangle): the transform and nothing else, the posed record written out.
//   k_pose_any<FMT, FIRST>      one lane per (pose, mesh triangle): the lane transforms its triangle in registers and walks as
//                               k_query_triangles_any does (the same TriQuery, the same PrimListWalk); on a hit it fetch_mins its mesh
//                               triangle index into the pose's 32-bit word.
//   k_pose_finish               one lane per pose: hit and first from the words.
//   k_pose_distance<FMT>        phase 1, one lane per (pose, mesh triangle): the lane walks as k_query_triangle_distance does (the same
//                               TriDistWalk) and fetch_mins (bits of d2) << 32 | mesh triangle into the pose's 64-bit key.
//   k_pose_record<FMT>          phase 2, one lane per pose: the winning triangle transformed again, k_query_triangle_distance's own
//                               walk and epilogue for it with the full max_radius, the record written with query_triangle.
//
// The transform is include/acgpt.h's statement, x' = ((m[0] x + m[1] y) + m[2] z) + m[3] per row, every operation on its own
// (-ffp-contract=off), so the posed vertices are the same bits wherever they are formed: in k_pose_triangles, in a walking lane, in
// phase 2, in tests/poses_ref.py.
//
// Shared words.  The per-pose words and keys are the only memory that lanes of different workgroups share inside a launch; they are
// touched by agent-scope relaxed atomic loads and fetch_min alone, never by a plain load or store.  They are filled before the launch
// and read plainly only by the next kernel on the stream (visibility is relied on at kernel boundaries only).  No lane waits for
// another: no spinning, no look-back, no order between workgroups.
//
// The early look.  Before walking, a lane reads its pose's word.  k_pose_any stays out if it cannot change the answer: with FIRST a
// lower index is already there, without FIRST any index is.  k_pose_distance walks with r2 = min(max_radius^2, d2 of the key) and stays
// out if the key holds d2 = 0 from a lower index.  The look is a hint whose only effect is less work; the results are decided by
// fetch_min alone, which does not depend on order, so two calls give the same bits on any schedule and in any dealing of the lanes:
//   * any: the word ends as the minimum of the indices of all lanes that hit.  A lane that stays out has an index above a value
//     that is already there (FIRST), or would only lower a word of which nothing but "is there one" is reported (no FIRST).
//   * distance: the key ends as the minimum of (d2, triangle) over all candidates.  A lane whose true d2 exceeds the shrunken r2
//     cannot win: a key with a smaller d2 is already there.  A lane whose d2 equals it is still a candidate (d2 <= r2), so a lower
//     index still wins the tie.  A lane that finds its d2 under a smaller radius finds the same d2: the walk's minimum over the scene
//     triangles within r2 is the minimum over all of them whenever that lies within r2.
// The key orders exactly as (d2, triangle) does: a candidate's d2 is never a NaN (d2 <= r2 is false for one) and never negative, so
// its bits order as an unsigned integer; -0 is stored as +0, which it equals; +inf (a candidate under max_radius = +inf) is 0x7F800000
// and stays below the all-ones of an empty key.
// 256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h.  Vector memory instructions throughout.
#include "poses.h"
#include "bvh_walk.h"
#include "tritri_device.h"
#include "tridist_device.h"

namespace ptd {

struct PosedTri { f3 a0, a1, a2; };

__device__ __forceinline__ f3 pose_point(const float4& m0, const float4& m1, const float4& m2, float x, float y, float z)
{
    return mk(((m0.x * x + m0.y * y) + m0.z * z) + m0.w, ((m1.x * x + m1.y * y) + m1.z * z) + m1.w, ((m2.x * x + m2.y * y) + m2.z * z) + m2.w);
}

// mesh triangle t under pose p.  The fourth floats of the mesh records are loaded with their float4 and never used.
__device__ __forceinline__ PosedTri pose_triangle(const float4* __restrict__ mesh, uint32_t t, const float4* __restrict__ poses, uint32_t p)
{
    const float4 m0 = poses[3ull * p], m1 = poses[3ull * p + 1ull], m2 = poses[3ull * p + 2ull];
    const float4 g0 = mesh[3ull * t], g1 = mesh[3ull * t + 1ull], g2 = mesh[3ull * t + 2ull];
    PosedTri r;
    r.a0 = pose_point(m0, m1, m2, g0.x, g0.y, g0.z);
    r.a1 = pose_point(m0, m1, m2, g1.x, g1.y, g1.z);
    r.a2 = pose_point(m0, m1, m2, g2.x, g2.y, g2.z);
    return r;
}

// Lane j < P * T as (pose, mesh triangle): triangle-major, all poses' triangle 0 first, so that later workgroups find most poses
// already decided (the product's order: the faster of the two on the sets of tools/poses_timing.py), or
// pose-major, consecutive lanes on consecutive triangles of one pose.  Which of the two changes no output bit.
__device__ __forceinline__ void pose_pair(uint32_t j, uint32_t T, uint32_t P, uint32_t flags, uint32_t& p, uint32_t& t)
{
    if (flags & kPosePoseMajor) { p = j / T; t = j - p * T; }
    else { t = j / P; p = j - t * P; }
}

__global__ void __launch_bounds__(256)
k_pose_triangles(const float4* __restrict__ mesh, uint32_t T, const float4* __restrict__ poses, uint32_t n, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    if (i >= n) return;
    const uint32_t p = i / T, t = i - p * T;
    const PosedTri r = pose_triangle(mesh, t, poses, p);
    out[3ull * i] = make_float4(r.a0.x, r.a0.y, r.a0.z, 0.0f);
    out[3ull * i + 1ull] = make_float4(r.a1.x, r.a1.y, r.a1.z, 0.0f);
    out[3ull * i + 2ull] = make_float4(r.a2.x, r.a2.y, r.a2.z, 0.0f);
}

// words[p]: 0xFFFFFFFF before the launch.  A lane past n takes the last pair's data and stays inactive.
template <int FMT, bool FIRST>
__global__ void __launch_bounds__(256)
k_pose_any(const DeviceScene sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ mesh, uint32_t T, const float4* __restrict__ poses, uint32_t P,
           uint32_t n, uint32_t* words, uint32_t flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    uint32_t p, t;
    pose_pair(i < n ? i : n - 1u, T, P, flags, p, t);
    const PosedTri r = pose_triangle(mesh, t, poses, p);
    TriQuery q;
    bool ok = q.set(r.a0, r.a1, r.a2) && i < n;      // a non-finite posed coordinate: a miss before any traversal
    q.prepare(sc, scene_term);
    if (!(flags & kPoseNoEarly)) {
        const uint32_t cur = __hip_atomic_load(words + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = ok && (FIRST ? cur > t : cur == 0xFFFFFFFFu);
    }
    PrimList<0> L;
    PrimListWalk<TriQuery, 0, true> walk(q, 0u, L);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, walk, visits);
    if (walk.count != 0u) __hip_atomic_fetch_min(words + p, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The launch before this one has ended: the words are read as they are.
__global__ void __launch_bounds__(256)
k_pose_finish(const uint32_t* __restrict__ words, uint32_t P, uint8_t* __restrict__ hit, uint32_t* __restrict__ first)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t w = words[i];
    hit[i] = w != 0xFFFFFFFFu ? 1 : 0;
    if (first) first[i] = w;
}

// keys[p]: all ones before the launch.
template <int FMT>
__global__ void __launch_bounds__(256)
k_pose_distance(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ mesh, uint32_t T, const float4* __restrict__ poses, uint32_t P,
                uint32_t n, float max_radius, unsigned long long* keys, uint32_t flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    uint32_t p, t;
    pose_pair(i < n ? i : n - 1u, T, P, flags, p, t);
    const PosedTri r = pose_triangle(mesh, t, poses, p);
    TriDistQuery tq;
    bool ok = tri_dist_query(tq, r.a0, r.a1, r.a2, max_radius) && i < n;
    float r2 = max_radius * max_radius;
    if (!(flags & kPoseNoEarly)) {
        const unsigned long long key = __hip_atomic_load(keys + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (key != ~0ull) {
            const float kd2 = __uint_as_float((uint32_t)(key >> 32));      // a candidate's d2: no NaN, not negative
            r2 = fminf(r2, kd2);
            if (kd2 == 0.0f && (uint32_t)key < t) ok = false;               // nothing is below (0, a lower index)
        }
    }
    TriBound tb;
    const float lane_abs = tri_dist_bounds<FMT, false>(sc, tq, abs_term, 0u, tb);
    TriDistWalk best(tq, tb, r2, lane_abs);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, best, visits);
    if (ok && best.slot >= 0) {
        const uint32_t bits = best.d2 == 0.0f ? 0u : __float_as_uint(best.d2);
        __hip_atomic_fetch_min(keys + p, ((unsigned long long)bits << 32) | t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One lane per pose.  Phase 1 has ended: the keys are read as they are.  A pose with an empty key gets the miss record.
template <int FMT>
__global__ void __launch_bounds__(256)
k_pose_record(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ mesh, const float4* __restrict__ poses, uint32_t P,
              float max_radius, const unsigned long long* __restrict__ keys, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    const uint32_t p = i < P ? i : P - 1u;
    const unsigned long long key = keys[p];
    const bool found = key != ~0ull && i < P;
    const uint32_t t = found ? (uint32_t)key : 0u;
    const PosedTri r = pose_triangle(mesh, t, poses, p);
    TriDistQuery tq;
    const bool ok = tri_dist_query(tq, r.a0, r.a1, r.a2, max_radius) && found;
    TriBound tb;
    const float lane_abs = tri_dist_bounds<FMT, false>(sc, tq, abs_term, 0u, tb);
    TriDistWalk best(tq, tb, max_radius * max_radius, lane_abs);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, ok, best, visits);
    if (i >= P) return;
    float4 o0, o1, o2;
    tri_dist_record(sc, tq, ok, best, o0, o1, o2);
    o1.w = __uint_as_float(ok && best.slot >= 0 ? t : 0xFFFFFFFFu);      // query_triangle, in the place of pad0
    out[3ull * i] = o0;
    out[3ull * i + 1ull] = o1;
    out[3ull * i + 2ull] = o2;
}

hipError_t launch_pose_triangles(const float4* mesh, uint32_t T, const float4* poses, uint32_t P, float4* out, hipStream_t stream)
{
    const uint32_t n = P * T;      // <= 2^31 - 1 (capi_query.hip)
    k_pose_triangles<<<(n + 255u) / 256u, 256, 0, stream>>>(mesh, T, poses, n, out);
    return hipGetLastError();
}

hipError_t launch_poses_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* mesh, uint32_t T, const float4* poses, uint32_t P,
                            uint32_t* words, uint8_t* hit, uint32_t* first, uint32_t flags, hipStream_t stream)
{
    const uint32_t n = P * T;
    hipError_t e = hipMemsetAsync(words, 0xFF, (size_t)P * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (fmt == 11) {
        e = first ? launch_lane_stack(k_pose_any<11, true>, stack_entries, n, stream, sc, stack_entries, scene_term, mesh, T, poses, P, n, words, flags)
                  : launch_lane_stack(k_pose_any<11, false>, stack_entries, n, stream, sc, stack_entries, scene_term, mesh, T, poses, P, n, words, flags);
    } else {
        e = first ? launch_lane_stack(k_pose_any<0, true>, stack_entries, n, stream, sc, stack_entries, scene_term, mesh, T, poses, P, n, words, flags)
                  : launch_lane_stack(k_pose_any<0, false>, stack_entries, n, stream, sc, stack_entries, scene_term, mesh, T, poses, P, n, words, flags);
    }
    if (e != hipSuccess) return e;
    k_pose_finish<<<(P + 255u) / 256u, 256, 0, stream>>>(words, P, hit, first);
    return hipGetLastError();
}

hipError_t launch_poses_distance(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* mesh, uint32_t T, const float4* poses, uint32_t P,
                                 float max_radius, unsigned long long* keys, float4* out, uint32_t flags, hipStream_t stream)
{
    const uint32_t n = P * T;
    hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)P * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if (fmt == 11) e = launch_lane_stack(k_pose_distance<11>, stack_entries, n, stream, sc, stack_entries, abs_term, mesh, T, poses, P, n, max_radius, keys, flags);
    else e = launch_lane_stack(k_pose_distance<0>, stack_entries, n, stream, sc, stack_entries, abs_term, mesh, T, poses, P, n, max_radius, keys, flags);
    if (e != hipSuccess) return e;
    if (fmt == 11) return launch_lane_stack(k_pose_record<11>, stack_entries, P, stream, sc, stack_entries, abs_term, mesh, poses, P, max_radius, (const unsigned long long*)keys, out);
    return launch_lane_stack(k_pose_record<0>, stack_entries, P, stream, sc, stack_entries, abs_term, mesh, poses, P, max_radius, (const unsigned long long*)keys, out);
}

}  // namespace ptd
