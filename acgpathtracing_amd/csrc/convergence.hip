// convergence.hip — the kernels behind pt_convergence_update (include/acgpt.h).
//
//   k_convergence_update  one workgroup of 256 lanes per 16 x 16 tile and step (the grid strides over the tiles), one pixel per lane:
//                         a 16-byte load of the accumulation and of the state, West's weighted update, a 16-byte store of the state
//                         and an optional 4-byte store of the error; the tile max through wave shuffles and LDS; every wave counts
//                         into its own LDS slots, the workgroup adds its non-empty slots to the context's counts with vector atomics
//   k_convergence_meter   one wave: a shuffle scan of the 256 bins gives the quantile; writes the record and clears the counts for the
//                         next call
//
// Every expression is mirrored operation for operation by tests/convergence_ref.py (fp32, same order; this file is built with
// -ffp-contract=off).  The counts are integers and the max is a max of bit patterns: the order of the atomics cannot change a bit.
#include "convergence.h"
#include "image_common.h"

namespace ptd {

__global__ void __launch_bounds__(kConvThreads)
k_convergence_update(const float4* __restrict__ accum, float4* __restrict__ state, uint32_t w, uint32_t h, uint32_t tiles_x, uint64_t tiles, float k1,
                     float lum_floor, float threshold, float* __restrict__ out_error, float* __restrict__ out_tiles, uint32_t* __restrict__ live)
{
    constexpr uint32_t kCounts = kConvBins + 3u, kWaves = kConvThreads / 64u;      // bins, unmeasured, invalid, converged
    __shared__ uint32_t counts[kWaves * kCounts];
    __shared__ uint32_t tile_max[2][kWaves], tile_any[2][kWaves], block_max;
    for (uint32_t b = threadIdx.x; b < kWaves * kCounts; b += kConvThreads) counts[b] = 0u;
    if (threadIdx.x == 0u) block_max = 0u;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    const int lane = (int)(threadIdx.x & 63u);
    uint32_t* mine = counts + wave * kCounts;
    const uint32_t lx = threadIdx.x & (kConvTile - 1u), ly = threadIdx.x / kConvTile;      // a wave covers four rows of the tile
    uint32_t run_max = 0u, par = 0u;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x, par ^= 1u) {
        const ulonglong2 tile = tile_xy(t, tiles_x);
        const uint64_t x = tile.x * kConvTile + lx, y = tile.y * kConvTile + ly;
        int k = -1;                      // the slot this pixel counts in; -1 outside the image
        uint32_t err_bits = 0u;
        bool measured = false, converged = false;
        if (x < w && y < h) {
            const uint64_t i = y * w + x;
            const float4 a = accum[i];
            float4 s = state[i];
            const float l1 = image_lum(a.x, a.y, a.z);
            float err = -1.0f;
            if (!(fabsf(l1) <= 3.402823466e+38f)) {
                s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                k = (int)kConvInvalid;
            } else if (!(s.z > 0.0f) || !(k1 > s.z)) {
                s = make_float4(l1, 0.0f, k1, 1.0f);
                k = (int)kConvUnmeasured;
            } else {
                const float n = k1 - s.z;
                const float d = l1 - s.x;
                const float wt = (s.z * k1) / n;
                const float m2 = s.y + wt * (d * d);
                const float b = s.w + 1.0f;
                s = make_float4(l1, m2, k1, b);
                const float v = m2 / ((b - 1.0f) * k1);
                const float sem = sqrtf(v);
                err = sem / fmaxf(l1, lum_floor);
                err_bits = __float_as_uint(err);
                const int j = (int)(err_bits >> 20) - (int)kConvBinBase;
                k = j < 0 ? 0 : (j > (int)kConvBins - 1 ? (int)kConvBins - 1 : j);
                measured = true;
                converged = err <= threshold;
            }
            state[i] = s;
            if (out_error) out_error[i] = err;
        }
        // the tile's max: the error's bits as uint32 (non-negative floats: unsigned order is float order)
        const uint32_t wmax = wave_max(err_bits);
        const uint64_t any = __ballot(measured), conv = __ballot(converged);
        run_max = wmax > run_max ? wmax : run_max;
        if (out_tiles) {
            if (lane == 0) { tile_max[par][wave] = wmax; tile_any[par][wave] = any != 0ull ? 1u : 0u; }
            __syncthreads();            // one barrier per tile: the next tile writes the other half
            if (threadIdx.x == 0u) {
                uint32_t m = 0u, has = 0u;
#pragma unroll
                for (uint32_t v = 0; v < kWaves; v++) { m = tile_max[par][v] > m ? tile_max[par][v] : m; has |= tile_any[par][v]; }
                out_tiles[t] = has ? __uint_as_float(m) : -1.0f;
            }
        }
        if (lane == 0 && conv != 0ull) atomicAdd(&mine[kConvConverged], (uint32_t)__popcll(conv));
        wave_count(mine, k, lane);
    }
    if (lane == 0 && run_max != 0u) atomicMax(&block_max, run_max);
    __syncthreads();
    flush_wave_counts<kCounts, kWaves, kConvThreads>(counts, live);
    if (threadIdx.x == kConvThreads - 1u && block_max != 0u) atomicMax(&live[kConvMax], block_max);
}

// <<<1, 64>>>: lane j owns bins 4j .. 4j+3
__global__ void __launch_bounds__(64)
k_convergence_meter(ConvergenceState* __restrict__ st, uint32_t frames, uint32_t quantile_permille)
{
    constexpr uint32_t kPer = kConvBins / 64u;
    static_assert(kPer * 64u == kConvBins, "bins per lane");
    const uint32_t lane = threadIdx.x;
    uint32_t hgm[kPer], sum = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) { hgm[j] = st->live[lane * kPer + j]; sum += hgm[j]; }
    const uint32_t unmeasured = st->live[kConvUnmeasured], invalid = st->live[kConvInvalid], converged = st->live[kConvConverged], max_bits = st->live[kConvMax];
    const uint32_t incl = wave_scan_inclusive(sum, lane);      // counts are at most 2^31 in all: uint32 holds every partial sum
    const uint32_t n = __shfl(incl, 63);
    uint64_t r = ((uint64_t)n * quantile_permille + 999u) / 1000u;
    if (r < 1u) r = 1u;
    // the first bin whose inclusive prefix count reaches r
    uint32_t c = incl - sum, found = kConvBins;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        c += hgm[j];
        if (found == kConvBins && c >= r) found = lane * kPer + j;
    }
    const uint64_t who = __ballot(found != kConvBins);
    const uint32_t bin = who != 0ull ? (uint32_t)__shfl((int)found, __ffsll((unsigned long long)who) - 1) : kConvBins;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) { st->record.histogram[lane * kPer + j] = hgm[j]; st->live[lane * kPer + j] = 0u; }
    if (lane != 0u) return;
    st->live[kConvUnmeasured] = 0u; st->live[kConvInvalid] = 0u; st->live[kConvConverged] = 0u; st->live[kConvMax] = 0u;
    st->record.frames = frames;
    st->record.measured_pixels = n;
    st->record.unmeasured_pixels = unmeasured;
    st->record.invalid_pixels = invalid;
    st->record.converged_pixels = converged;
    st->record.max_error = n != 0u ? __uint_as_float(max_bits) : 0.0f;
    st->record.quantile_error = n != 0u ? __uint_as_float((kConvBinBase + bin + 1u) << 20) : 0.0f;
    st->record.reserved = 0u;
}

hipError_t launch_convergence(const float4* accum, uint32_t w, uint32_t h, uint32_t accum_frames, const pt_convergence_params& cp, float4* state,
                              float* out_error, float* out_tiles, ConvergenceState* st, hipStream_t stream)
{
    const TileWalk tw = tile_walk(w, h, kConvTile, kConvBlocks);
    k_convergence_update<<<tw.grid, kConvThreads, 0, stream>>>(accum, state, w, h, tw.tiles_x, tw.tiles, (float)accum_frames, cp.lum_floor, cp.threshold, out_error,
                                                           out_tiles, st->live);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_convergence_meter<<<1, 64, 0, stream>>>(st, accum_frames, cp.quantile_permille);
    return hipGetLastError();
}

}  // namespace ptd
