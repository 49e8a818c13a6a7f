// ao.h — ambient occlusion traced on the device: pt_ao_points / pt_ao_image (include/acgpt.h states the contract; tests/ao_ref.py is
// the NumPy statement of the rays and the counts).  Kernels in ao.hip; they read the render kernels' headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

constexpr uint32_t kAoMaxSamples = 256u;

// what a call passes to the kernel besides its arrays: pt_ao_params after the host's checks
struct AoArgs {
    uint32_t samples;         // K, 1..kAoMaxSamples
    float radius, bias;
    uint32_t seed;
    uint32_t accumulate;      // 0 / 1
    uint32_t total_samples;   // the divisor of ao
};
// the view of the image form: the camera pt_render_features traced normal_depth with
struct AoView { pt_float3 eye, U, V, W; uint32_t w, h; };

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  points: n records of two float4 {P.xyz, -}
// {N.xyz, -}; normal_depth: float4[w*h]; disk: args.samples pairs (x, y); visible: uint32[n]; ao: float[n] or null.  All DEVICE, points
// and normal_depth 16-byte aligned, n >= 1 (w * h >= 1).
hipError_t launch_ao_points(int fmt, const DeviceScene& sc, uint32_t stack_entries, const float4* points, uint32_t n, const float2* disk, const AoArgs& args,
                            uint32_t* visible, float* ao, hipStream_t stream);
hipError_t launch_ao_image(int fmt, const DeviceScene& sc, uint32_t stack_entries, const AoView& view, const float4* normal_depth, const float2* disk,
                           const AoArgs& args, uint32_t* visible, float* ao, hipStream_t stream);

}  // namespace ptd
