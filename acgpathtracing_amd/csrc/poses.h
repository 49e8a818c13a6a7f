// poses.h — posed-mesh queries: pt_pose_triangles, pt_query_poses_any, pt_query_poses_distance (include/acgpt.h states the
// contracts; tests/poses_ref.py is the NumPy statement).  One registered query mesh, P poses of 12 floats, one byte or one closest
// pair per pose; the P x T posed records are never materialised.  Kernels in poses.hip; the walk, the leaf tests and the policies
// are bvh_walk.h's, tritri_device.h's and tridist_device.h's, shared with the per-triangle kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

constexpr size_t kPoseMeshMaxTris = (size_t)1 << 20;      // pt_set_query_mesh's limit

// flags of the launches below (acgpt_test.h pt_debug_query_poses; the product passes 0)
constexpr uint32_t kPoseNoEarly = 1u;          // no early look at the pose's word, no shrinking radius: every lane walks as the per-triangle kernels do
constexpr uint32_t kPosePoseMajor = 2u;        // lanes are dealt pose-major (consecutive lanes on consecutive triangles of one pose) instead of
                                               // triangle-major (all poses' triangle 0 first), the product's order

// mesh: T records of three float4 (DEVICE, the context's copy); poses: P records of three float4 (the rows of the 3 x 4 matrix);
// out: P * T records of three float4, pose-major.  P * T <= 2^31 - 1.
hipError_t launch_pose_triangles(const float4* mesh, uint32_t T, const float4* poses, uint32_t P, float4* out, hipStream_t stream);

// words: P 32-bit words of scratch, written here (0xFFFFFFFF, then the lowest hit triangle index by fetch_min); hit: P bytes;
// first: P words or null.  scene_term: overlap_scene_term of the scene.  Three steps on the stream: fill, walk, finish.
hipError_t launch_poses_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* mesh, uint32_t T, const float4* poses, uint32_t P,
                            uint32_t* words, uint8_t* hit, uint32_t* first, uint32_t flags, hipStream_t stream);

// keys: P 64-bit words of scratch, written here (all ones, then (bits of d2) << 32 | mesh triangle by fetch_min); out: P records of
// three float4 (pt_pose_distance_hit).  abs_term: nearest_abs_term of the scene.  Three steps on the stream: fill, phase 1, phase 2.
hipError_t launch_poses_distance(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* mesh, uint32_t T, const float4* poses, uint32_t P,
                                 float max_radius, unsigned long long* keys, float4* out, uint32_t flags, hipStream_t stream);

}  // namespace ptd
