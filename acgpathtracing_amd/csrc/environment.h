// environment.h — the device side of pt_set_environment (include/acgpt.h): the map's texels and its importance-sampling CDFs.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "pt_environment.h"

namespace ptd {

struct EnvDevice {
    float4* texels = nullptr;       // [h][w] {r, g, b, sampling weight}
    float* marginal = nullptr;      // [h]
    float* conditional = nullptr;   // [h][w]
    uint32_t w = 0, h = 0;
    float total = 0.0f;             // sum of the sampling weights (0: a black map)
    float pdf_scale = 0.0f;         // w h / (2 pi^2 total), 0 when total is 0
};

constexpr uint32_t kEnvMaxDim = 16384u, kEnvMaxTexels = 1u << 25;

// Uploads h_rgba ({r, g, b, 0} per texel, scale already applied) and builds the CDFs on the device: one workgroup per row weighs
// and scans the row, one workgroup scans the row totals.  Fixed summation order: the same texels give the same bits.  Synchronous.
bool env_upload(EnvDevice& e, const float4* h_rgba, uint32_t w, uint32_t h, hipStream_t stream, std::string& err);
void env_free(EnvDevice& e);
inline EnvMap env_view(const EnvDevice& e) { EnvMap m; m.texels = e.texels; m.marginal = e.marginal; m.conditional = e.conditional; m.w = e.w; m.h = e.h; m.pdf_scale = e.pdf_scale; return m; }

// pt_debug_environment: op 0 dir[3] -> {r, g, b, texel index}, op 1 dir[3] -> pdf, op 2 (u1, u2) -> {dir[3], pdf}; math 0 IEEE, 1 fast
hipError_t env_debug(const EnvMap& m, int op, int math, const float* d_in, uint32_t n, float* d_out, hipStream_t stream);

}  // namespace ptd
