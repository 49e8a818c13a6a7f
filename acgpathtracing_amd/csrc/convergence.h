// convergence.h — the per-pixel error estimate of pt_convergence_update (include/acgpt.h states the arithmetic; tests/convergence_ref.py
// is its NumPy reference).  Kernels in convergence.hip; no render kernel is involved.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

constexpr uint32_t kConvBins = PT_CONVERGENCE_BINS;
constexpr uint32_t kConvTile = PT_CONVERGENCE_TILE;
constexpr uint32_t kConvBinBase = 824u;               // bits(2^-24) >> 20: the first bin
constexpr uint32_t kConvThreads = kConvTile * kConvTile;      // one lane per pixel of a tile
constexpr uint32_t kConvBlocks = 2048u;               // the update's grid is min(tiles, 2048): each workgroup strides over the rest
// live slots after the bins
constexpr uint32_t kConvUnmeasured = kConvBins, kConvInvalid = kConvBins + 1u, kConvConverged = kConvBins + 2u, kConvMax = kConvBins + 3u;
constexpr uint32_t kConvSlots = kConvBins + 4u;

// What the context keeps on the device: the live counts (bins 0..255, unmeasured, invalid, converged, the max of the error's bits),
// all zero between two calls (the meter kernel clears them after it has read them), and the record the meter kernel writes, in
// pt_convergence_info's layout.
struct ConvergenceState {
    uint32_t live[kConvSlots];
    pt_convergence_info record;
};

// accum, state: float4[w * h]; out_error: float[w * h] or null; out_tiles: float[ceil(w / 16) * ceil(h / 16)] or null.
// `st->live` must be zero on entry.
hipError_t launch_convergence(const float4* accum, uint32_t w, uint32_t h, uint32_t accum_frames, const pt_convergence_params& cp, float4* state,
                              float* out_error, float* out_tiles, ConvergenceState* st, hipStream_t stream);

}  // namespace ptd
