// firefly.h — the outlier clamp of pt_firefly_filter (include/acgpt.h states the arithmetic; tests/firefly_ref.py is its NumPy
// reference).  Kernels in firefly.hip; no render kernel is involved.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

constexpr uint32_t kFireflyTile = 16u;
constexpr uint32_t kFireflyThreads = kFireflyTile * kFireflyTile;      // one lane per pixel of a tile
constexpr uint32_t kFireflyBlocks = 4096u;           // the grid is min(tiles, 4096): each workgroup strides over the rest
constexpr uint32_t kFireflyStride = 48u;             // LDS row stride in floats: 16 mod 32, the rows a wave reads share no bank

// What the context keeps on the device: the live counts and sums, all zero between two calls (the finish kernel clears them after
// it has read them), and the record the finish kernel writes, in pt_firefly_info's layout.
struct FireflyState {
    uint32_t clamped, replaced, passed, max_ratio_bits;
    unsigned long long total_q16, removed_q16;
    pt_firefly_info record;
};

// src, out: float4[w * h], disjoint.  The live part of `st` must be zero on entry.
hipError_t launch_firefly(const float4* src, uint32_t w, uint32_t h, const pt_firefly_params& fp, float4* out, FireflyState* st, hipStream_t stream);

}  // namespace ptd
