// denoise.h — first-hit feature buffers and the edge-avoiding a-trous filter of pt_render_features / pt_denoise (include/acgpt.h
// states the filter; tests/denoise_ref.py is its NumPy reference).  Kernels in denoise.hip; they read the render kernels' headers
// and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// the constants of the filter (include/acgpt.h, tests/denoise_ref.py)
constexpr float kDnSigmaZ = 0.01f;         // depth: exp(-|t_p - t_q| / (sigma_z * step * t_p))
constexpr int   kDnNormalSquarings = 7;    // normals: max(0, n_p . n_q)^128, as seven squarings
constexpr float kDnSigmaL = 5.0f;          // luminance: exp(-|l_p - l_q| / (sigma_l * sqrt(g(var)_p) + 1e-6))
constexpr float kDnAlbedoFloor = 0.01f;    // demodulation: c = rgb / max(albedo, 0.01) on a hit
constexpr uint32_t kDnMaxIterations = 8u;

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes)
hipError_t launch_features(int fmt, const DeviceScene& sc, uint32_t stack_entries, uint32_t w, uint32_t h, pt_float3 eye, pt_float3 U, pt_float3 V,
                           pt_float3 W, float4* albedo_prim, float4* normal_depth, hipStream_t stream);
// accum, albedo_prim, normal_depth: float4[w*h]; scratch: two float4[w*h]; out: float4[w*h]
hipError_t launch_denoise(const float4* accum, const float4* albedo_prim, const float4* normal_depth, uint32_t w, uint32_t h, uint32_t iterations,
                          float4* scratch0, float4* scratch1, float4* out, hipStream_t stream);

}  // namespace ptd
