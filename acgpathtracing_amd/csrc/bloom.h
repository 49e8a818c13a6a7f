// bloom.h — the glare pyramid of pt_bloom (include/acgpt.h states the arithmetic; tests/bloom_ref.py is its NumPy reference).
// Kernels in bloom.hip; no render kernel is involved.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

constexpr uint32_t kBloomTile = 16u;                 // a workgroup owns a 16 x 16 tile of the level it writes
constexpr uint32_t kBloomThreads = kBloomTile * kBloomTile;
constexpr uint32_t kBloomBlocks = 4096u;             // the grid is min(tiles, 4096): each workgroup strides over the rest
constexpr uint32_t kBloomFoot = 2u * kBloomTile + 2u;   // 34: the finer level's footprint of a tile under the 4-tap filter
// LDS row stride of the footprint in float4 slots.  A row keeps its even columns in slots 0..16 and its odd ones in 20..36: the
// lanes of a tile row read columns 2 lx + i, so one 16-byte read of all lanes touches one parity only, and consecutive lanes take
// consecutive slots instead of every other one (a 2-way conflict at any stride).  40 = 0 mod 8: the two tile rows a 16-lane group of
// a 16-byte LDS read spans are two footprint rows = 80 slots = 0 mod 16 apart, so its 8 + 8 lanes (lx 0-3, 12-15 of one row, 4-11
// of the next) cover the 16 slots of a 256-byte bank row once.  20 = 4 mod 8: the eight lanes of a 16-byte LDS write that fill
// eight consecutive columns put four slots into each half of a 128-byte row.
constexpr uint32_t kBloomStride = 40u, kBloomOdd = 20u;
constexpr uint32_t kBloomMaxLevels = 8u;

// What the context keeps on the device: the live counts and sums, all zero between two calls (the finish kernel clears them after
// it has read them), and the record the finish kernel writes, in pt_bloom_info's layout.
struct BloomState {
    uint32_t bright, invalid, max_luma_bits, pad;
    unsigned long long total_q16, bright_q16;
    pt_bloom_info record;
};

// The levels of a width x height source: w[0], h[0] the source itself, level k at texel offset off[k] of the pyramid (k = 1..n).
struct BloomLevels {
    uint32_t n;
    uint32_t w[kBloomMaxLevels + 1u], h[kBloomMaxLevels + 1u];
    uint64_t off[kBloomMaxLevels + 2u];              // off[n + 1]: the texels of the whole pyramid
};
BloomLevels bloom_levels(uint32_t width, uint32_t height, uint32_t levels);

// src, out: float4[w * h], disjoint; pyramid: float4[bloom_levels(...).off[n + 1]].  The live part of `st` must be zero on entry.
hipError_t launch_bloom(const float4* src, uint32_t w, uint32_t h, const pt_bloom_params& bp, float4* out, float4* pyramid, BloomState* st,
                        hipStream_t stream);

}  // namespace ptd
