// temporal.h — the temporal reprojection of pt_temporal_blend (include/acgpt.h states it; tests/temporal_ref.py is its NumPy
// reference).  Kernels in temporal.hip; they read the render kernels' headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// The previous view: its camera, its size, and its history + features (float4[w*h] each), or all three null (no history).
struct TpPrev {
    pt_float3 eye, U, V, W;
    uint32_t w, h;
    const float4* hist;
    const float4* albedo_prim;
    const float4* normal_depth;
};

// pt_temporal_blend_motion's additions: the scene's index buffer and the positions each view was traced with (float4[n_verts] each,
// both or neither: no motion), and the clip's gamma (0: off).  pt_temporal_blend passes none and runs the kernel without them.
struct TpMotion {
    const uint32_t* idx;
    const float4* verts;
    const float4* prev_verts;
    float gamma;
};

// bsdf[prim] = the bsdfType of triangle prim (caller's index order), from the leaf slots' TriRecord::r2.y and shade .w; n_tris bytes
hipError_t launch_tri_bsdf(const DeviceScene& sc, uint8_t* bsdf, hipStream_t stream);
// accum, albedo_prim, normal_depth, out: float4[w*h] of the current view; n_samples: what accum stands for (N > 0).  motion: null
// for pt_temporal_blend (k_tp_blend<false>), else pt_temporal_blend_motion's motion and clip (k_tp_blend<true>); idx and the vertex
// arrays are read only for diffuse hits
hipError_t launch_temporal(const float4* accum, const float4* albedo_prim, const float4* normal_depth, uint32_t w, uint32_t h, pt_float3 eye,
                           pt_float3 U, pt_float3 V, pt_float3 W, float n_samples, const TpPrev& prev, const uint8_t* bsdf, uint32_t n_tris,
                           float cap, const TpMotion* motion, float4* out, hipStream_t stream);

}  // namespace ptd
