// image_common.h — what the image stages share (denoise.hip, temporal.hip, display.hip, convergence.hip, firefly.hip, bloom.hip): the luminance,
// the wave helpers of the metered stages, the tile walk, the per-pixel launch shape and the pixel-centre camera ray.  A new stage
// starts from here.
//
// The files that include this one are built with -ffp-contract=off: every expression below is evaluated as written, operation for
// operation, and the NumPy references under tests/ mirror them.  A wave is 64 lanes; the wave helpers want all 64 active unless they
// say otherwise.  No render kernel includes this file: it is not part of pt_kernel_source_hash.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// Rec. 709 luminance, left to right: (0.2126 r + 0.7152 g) + 0.0722 b
__device__ __forceinline__ float image_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// ---- wave helpers -----------------------------------------------------------------------------------------------------------
// One count per lane into slot k of `mine`, the wave's own LDS slots; k < 0: this lane counts nothing.  Called by the active lanes of
// the wave together, `lane` in 0..63.
// A flat region puts all 64 lanes into one slot, an edge into two: 64 adds to one LDS word would run one after the other.  Up to
// two rounds take the first pending lane's slot and add the number of lanes that share it at once; what is left adds singly.
__device__ __forceinline__ void wave_count(uint32_t* mine, int k, int lane)
{
    uint64_t todo = __ballot(k >= 0);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (todo == 0ull) break;
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const int kb = __shfl(k, lead);
        const uint64_t same = __ballot(k == kb);
        if (lane == lead) atomicAdd(&mine[kb], (uint32_t)__popcll(same));
        if (k == kb) k = -1;
        todo &= ~same;
    }
    if (k >= 0) atomicAdd(&mine[k], 1u);
}

// The workgroup's epilogue after wave_count and a __syncthreads: the kWaves waves' slots (kWaves x kSlots words of LDS, wave-major)
// summed per slot, every non-zero sum added to `live` with one vector atomic.
template <uint32_t kSlots, uint32_t kWaves, uint32_t kThreads>
__device__ __forceinline__ void flush_wave_counts(const uint32_t* slots, uint32_t* __restrict__ live)
{
    for (uint32_t b = threadIdx.x; b < kSlots; b += kThreads) {
        uint32_t s = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) s += slots[w * kSlots + b];
        if (s != 0u) atomicAdd(&live[b], s);
    }
}

// inclusive prefix sum over the wave's 64 lanes: lane j gets v_0 + ... + v_j
__device__ __forceinline__ uint32_t wave_scan_inclusive(uint32_t v, uint32_t lane)
{
    for (uint32_t d = 1u; d < 64u; d <<= 1) { const uint32_t o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}

// the max over the wave's 64 lanes, in every lane (bit patterns of non-negative floats: unsigned order is float order)
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d); v = o > v ? o : v; }
    return v;
}

// ---- launch shapes ----------------------------------------------------------------------------------------------------------
// The tile walk: one workgroup per edge x edge tile and step, tiles in row-major order, the grid one-dimensional and strided
// (for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x)): no 65 535 limit on the tile rows, and the tile index stays 64-bit.
struct TileWalk { uint32_t tiles_x; uint64_t tiles; uint32_t grid; };      // grid = min(tiles, cap)
constexpr TileWalk tile_walk(uint32_t w, uint32_t h, uint32_t edge, uint32_t cap)
{
    const uint32_t tiles_x = (w + edge - 1u) / edge, tiles_y = (h + edge - 1u) / edge;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y;
    return {tiles_x, tiles, (uint32_t)(tiles < cap ? tiles : cap)};
}
// tile t's column (.x) and row (.y)
__device__ __forceinline__ ulonglong2 tile_xy(uint64_t t, uint32_t tiles_x)
{
    const uint64_t ty = t / tiles_x;
    return make_ulonglong2(t - ty * tiles_x, ty);
}

// The per-pixel stages: one lane per pixel, 32 x 8 workgroups, x = blockIdx.x * blockDim.x + threadIdx.x and y likewise.
struct PixelLaunch { dim3 grid, block; };
inline PixelLaunch pixel_launch(uint32_t w, uint32_t h) { return {dim3((w + 31u) / 32u, (h + 7u) / 8u), dim3(32, 8)}; }

// ---- camera -----------------------------------------------------------------------------------------------------------------
// The unit direction of the camera ray through the centre of pixel (x, y): pathTracerPrograms.cu:730-740 with the jitter at 0.5.
// The feature buffers are traced along it (k_dn_features), and whoever needs a first hit's position again multiplies the stored
// distance by this same function's result (k_tp_blend): one expression, so the same bits.
__device__ __forceinline__ f3 pixel_centre_dir(uint32_t x, uint32_t y, uint32_t w, uint32_t h, const pt_float3& U, const pt_float3& V, const pt_float3& W)
{
    const float dx = 2.0f * (((float)x + 0.5f) / (float)w) - 1.0f;
    const float dy = 2.0f * (((float)y + 0.5f) / (float)h) - 1.0f;
    return normalize(dx * mk(U) + dy * mk(V) + mk(W));
}

}  // namespace ptd
