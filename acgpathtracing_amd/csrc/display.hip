// display.hip — the kernels behind pt_display_transform (include/acgpt.h).
//
//   k_display_histogram   grid-stride over the image, one float4 per lane and step; every wave counts into its own LDS histogram, the
//                         workgroup adds its non-empty bins to the context's counts with vector atomicAdd
//   k_display_meter       one wave: the 320 counts -> the windowed mean of the bin centres -> the exposure, all on integers up to the
//                         one division key / L_avg; writes the record and clears the counts for the next call
//   k_display_apply       one pixel per lane: exposure from the record, clamp, tone curve, float4 and / or make_color
//
// Every expression is mirrored operation for operation by tests/display_ref.py (fp32, same order; this file is built with
// -ffp-contract=off).  The counts are integers: the order of the atomic adds cannot change a bit, two calls give the same bits.
#include "display.h"
#include "image_common.h"
#include "pt_shading.h"

namespace ptd {

// bin of a luminance, kDisplayBins for a pixel that is not metered (below 2^-20, zero, negative, NaN or infinite)
__device__ __forceinline__ uint32_t dp_bin(float l)
{
    if (!(l >= 0x1p-20f && l <= 3.402823466e+38f)) return kDisplayBins;
    const uint32_t k = (__float_as_uint(l) >> 20) - kDisplayBinBase;
    return k < kDisplayBins - 1u ? k : kDisplayBins - 1u;
}

__global__ void __launch_bounds__(kDisplayThreads)
k_display_histogram(const float4* __restrict__ src, uint64_t n, uint32_t* __restrict__ live)
{
    constexpr uint32_t kSlots = kDisplayBins + 1u, kWaves = kDisplayThreads / 64u;
    __shared__ uint32_t hist[kWaves * kSlots];
    for (uint32_t b = threadIdx.x; b < kWaves * kSlots; b += kDisplayThreads) hist[b] = 0u;
    __syncthreads();
    uint32_t* mine = hist + (threadIdx.x >> 6) * kSlots;
    const int lane = (int)(threadIdx.x & 63u);
    const uint64_t stride = (uint64_t)gridDim.x * kDisplayThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kDisplayThreads + threadIdx.x; i < n; i += stride) {
        const float4 c = src[i];
        wave_count(mine, (int)dp_bin(image_lum(c.x, c.y, c.z)), lane);      // every active lane counts: no k < 0 here
    }
    __syncthreads();
    flush_wave_counts<kSlots, kWaves, kDisplayThreads>(hist, live);
}

// <<<1, 64>>>: lane j owns bins 5j .. 5j+4
__global__ void __launch_bounds__(64)
k_display_meter(DisplayState* __restrict__ st, float key, uint32_t lo_permille, uint32_t hi_permille, float min_exposure, float max_exposure,
                float prev_exposure, float adapt)
{
    constexpr uint32_t kPer = kDisplayBins / 64u;
    static_assert(kPer * 64u == kDisplayBins, "bins per lane");
    const uint32_t lane = threadIdx.x;
    uint32_t h[kPer], sum = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) { h[j] = st->live[lane * kPer + j]; sum += h[j]; }
    const uint32_t unmetered = st->live[kDisplayBins];
    const uint32_t incl = wave_scan_inclusive(sum, lane);      // counts are at most 2^31 in all: uint32 holds every partial sum
    const uint32_t n = __shfl(incl, 63);
    uint64_t r_lo = (uint64_t)n * lo_permille / 1000u, r_hi = (uint64_t)n * hi_permille / 1000u;
    if (r_hi <= r_lo) { r_lo = 0u; r_hi = n; }
    uint64_t c = incl - sum, T = 0u, S = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint64_t a = c > r_lo ? c : r_lo, b = c + h[j] < r_hi ? c + h[j] : r_hi;
        const uint64_t t = b > a ? b - a : 0u;
        T += t;
        S += t * (2u * (lane * kPer + j) + 1u);
        c += h[j];
    }
    for (int d = 32; d >= 1; d >>= 1) { T += __shfl_xor((unsigned long long)T, d); S += __shfl_xor((unsigned long long)S, d); }
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) { st->record.histogram[lane * kPer + j] = h[j]; st->live[lane * kPer + j] = 0u; }
    if (lane != 0u) return;
    st->live[kDisplayBins] = 0u;
    float exposure, l_avg = 0.0f;
    if (n == 0u) {
        exposure = prev_exposure > 0.0f ? prev_exposure : 1.0f;
    } else {
        l_avg = __uint_as_float((kDisplayBinBase << 20) + (uint32_t)((S << 19) / T));
        float target = key / l_avg;
        target = fmaxf(target, min_exposure);
        target = fminf(target, max_exposure);
        exposure = prev_exposure > 0.0f ? prev_exposure + (target - prev_exposure) * adapt : target;
    }
    st->record.exposure = exposure;
    st->record.metered_luminance = l_avg;
    st->record.metered_pixels = n;
    st->record.unmetered_pixels = unmetered;
}

__device__ __forceinline__ float dp_range(float v) { return v > 0.0f ? (v < 65504.0f ? v : 65504.0f) : 0.0f; }
__device__ __forceinline__ float dp_aces(float x) { return fminf((x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f), 1.0f); }

// manual > 0: that exposure; else the record's
template <int CURVE>
__global__ void __launch_bounds__(kDisplayThreads)
k_display_apply(const float4* __restrict__ src, uint64_t n, const DisplayState* __restrict__ st, float manual, float white2,
                float4* __restrict__ out, uint32_t* __restrict__ fb)
{
    const uint64_t i = (uint64_t)blockIdx.x * kDisplayThreads + threadIdx.x;
    if (i >= n) return;
    const float e = manual > 0.0f ? manual : st->record.exposure;
    const float4 c = src[i];
    const float xr = dp_range(c.x * e), xg = dp_range(c.y * e), xb = dp_range(c.z * e);
    float yr, yg, yb;
    if (CURVE == PT_TONE_ACES) {
        yr = dp_aces(xr); yg = dp_aces(xg); yb = dp_aces(xb);
    } else if (CURVE == PT_TONE_REINHARD) {
        const float l = image_lum(xr, xg, xb);
        const float s = l > 0.0f ? (1.0f + l / white2) / (1.0f + l) : 0.0f;
        yr = fminf(xr * s, 1.0f); yg = fminf(xg * s, 1.0f); yb = fminf(xb * s, 1.0f);
    } else {
        yr = fminf(xr, 1.0f); yg = fminf(xg, 1.0f); yb = fminf(xb, 1.0f);
    }
    if (out) out[i] = make_float4(yr, yg, yb, 1.0f);
    if (fb) fb[i] = make_color(mk(yr, yg, yb));
}

hipError_t launch_display(const float4* src, uint64_t n, const pt_display_params& dp, DisplayState* st, float4* out, uint32_t* fb, hipStream_t stream)
{
    const uint64_t blocks = (n + kDisplayThreads - 1u) / kDisplayThreads;      // n <= 2^31: at most 2^23
    hipError_t e = hipSuccess;
    if (!(dp.exposure > 0.0f)) {
        const uint32_t grid = (uint32_t)(blocks < kDisplayHistBlocks ? blocks : kDisplayHistBlocks);
        k_display_histogram<<<grid, kDisplayThreads, 0, stream>>>(src, n, st->live);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_display_meter<<<1, 64, 0, stream>>>(st, dp.key, dp.lo_permille, dp.hi_permille, dp.min_exposure, dp.max_exposure, dp.prev_exposure, dp.adapt);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const float white2 = dp.white * dp.white;
    const uint32_t grid = (uint32_t)blocks;
    if (dp.tone_curve == PT_TONE_ACES) k_display_apply<PT_TONE_ACES><<<grid, kDisplayThreads, 0, stream>>>(src, n, st, dp.exposure, white2, out, fb);
    else if (dp.tone_curve == PT_TONE_REINHARD) k_display_apply<PT_TONE_REINHARD><<<grid, kDisplayThreads, 0, stream>>>(src, n, st, dp.exposure, white2, out, fb);
    else k_display_apply<PT_TONE_LINEAR><<<grid, kDisplayThreads, 0, stream>>>(src, n, st, dp.exposure, white2, out, fb);
    return hipGetLastError();
}

}  // namespace ptd
