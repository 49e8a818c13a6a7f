// bloom.hip — the kernels behind pt_bloom (include/acgpt.h).
//
//   k_bloom_down<PREFILTER>  one workgroup of 256 lanes per 16 x 16 tile of the level it writes and step (the grid strides over the
//                            tiles), one texel per lane.  The tile's 34 x 34 footprint on the finer level, edge-clamped, goes into
//                            LDS by 16-byte loads and stores (four or five entries per lane); every lane then evaluates the 4 x 4
//                            binomial of its texel from 16 16-byte LDS reads and stores 16 bytes.  PREFILTER = true is the first level:
//                            the footprint entries are the prefiltered source pixels, and the entries a tile owns (its own 32 x 32
//                            source pixels inside the image) are counted: per lane, then wave shuffles and LDS, then one vector atomic
//                            per workgroup and field
//   k_bloom_up               one lane per texel of the finer level: out = base + factor * U(coarse), .w = base.w as bits.  In the
//                            pyramid base == out (E_k = D_k + spread * U(E_(k+1)), a texel reads only itself on its own level); the last
//                            step is the composite, base = src, factor = gain
//   k_bloom_finish           one lane: copies the live counts into the record and clears them for the next call
//
// Every expression is mirrored operation for operation by tests/bloom_ref.py (fp32, same order; this file is built with
// -ffp-contract=off).  The reductions are integer sums and a max of bit patterns: the order of the atomics cannot change a bit.
#include "bloom.h"
#include "image_common.h"

namespace ptd {

struct BloomPre { float threshold, knee, clamp; };

__device__ __forceinline__ bool bl_valid(float l) { return l >= 0.0f && l <= 3.402823466e+38f; }
__device__ __forceinline__ unsigned long long bl_q16(float x) { return (unsigned long long)(fminf(x, 16777216.0f) * 65536.0f); }
// the binomial {1, 3, 3, 1} / 8, left to right
__device__ __forceinline__ float bl_tap4(float a, float b, float c, float d) { return ((0.125f * a + 0.375f * b) + 0.375f * c) + 0.125f * d; }
// the footprint slot of column c inside its row: the even columns first, the odd ones from kBloomOdd (bloom.h)
__device__ __forceinline__ uint32_t bl_slot(uint32_t c) { return (c & 1u) * kBloomOdd + (c >> 1); }

template <bool PREFILTER>
__global__ void __launch_bounds__(kBloomThreads)
k_bloom_down(const float4* __restrict__ fine, uint32_t fw, uint32_t fh, float4* __restrict__ coarse, uint32_t cw, uint32_t ch, uint32_t tiles_x,
             uint64_t tiles, BloomPre pre, BloomState* __restrict__ st)
{
    constexpr uint32_t kEntries = kBloomFoot * kBloomFoot, kWaves = kBloomThreads / 64u;
    __shared__ float4 foot[kBloomFoot * kBloomStride];
    const uint32_t tid = threadIdx.x, lx = tid & (kBloomTile - 1u), ly = tid / kBloomTile;      // a wave covers four rows of the tile
    uint32_t n_bright = 0u, n_invalid = 0u, max_bits = 0u;
    unsigned long long total = 0ull, bright = 0ull;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const ulonglong2 tile = tile_xy(t, tiles_x);
        const int64_t X0 = (int64_t)(tile.x * kBloomTile), Y0 = (int64_t)(tile.y * kBloomTile);
        const int64_t fx0 = 2 * X0 - 1, fy0 = 2 * Y0 - 1;          // the footprint's first column and row on the finer level
#pragma unroll
        for (uint32_t round = 0; round < (kEntries + kBloomThreads - 1u) / kBloomThreads; round++) {
            const uint32_t e = round * kBloomThreads + tid;
            if (e >= kEntries) break;
            const uint32_t r = e / kBloomFoot, c = e - r * kBloomFoot;
            const int64_t x = fx0 + (int64_t)c, y = fy0 + (int64_t)r;
            const int64_t qx = x < 0 ? 0 : (x < (int64_t)fw ? x : (int64_t)fw - 1), qy = y < 0 ? 0 : (y < (int64_t)fh ? y : (int64_t)fh - 1);
            float4 p = fine[(uint64_t)qy * fw + (uint64_t)qx];
            if (PREFILTER) {
                const float l = image_lum(p.x, p.y, p.z);
                const bool ok = bl_valid(l);
                // the tile's own source pixels: every pixel of the image belongs to one tile and is counted there
                const bool own = r >= 1u && r <= 2u * kBloomTile && c >= 1u && c <= 2u * kBloomTile && x < (int64_t)fw && y < (int64_t)fh;
                float ev = 0.0f;
                if (ok) {
                    const float d = l - pre.threshold;
                    if (pre.knee > 0.0f) {
                        const float s = fminf(fmaxf(l - (pre.threshold - pre.knee), 0.0f), pre.knee + pre.knee);
                        const float q = (s * s) / ((pre.knee + pre.knee) + (pre.knee + pre.knee));
                        ev = fmaxf(q, d);
                    } else {
                        ev = fmaxf(d, 0.0f);
                    }
                    if (pre.clamp > 0.0f) ev = fminf(ev, pre.clamp);
                }
                const bool lit = ok && ev > 0.0f;
                if (lit) {
                    const float s = ev / l;
                    p.x = p.x * s; p.y = p.y * s; p.z = p.z * s;
                } else {
                    p.x = 0.0f; p.y = 0.0f; p.z = 0.0f;
                }
                if (own) {
                    if (ok) {
                        total += bl_q16(l);
                        const uint32_t lb = __float_as_uint(l);
                        max_bits = lb > max_bits ? lb : max_bits;
                        if (lit) { n_bright++; bright += bl_q16(ev); }
                    } else {
                        n_invalid++;
                    }
                }
            }
            p.w = 0.0f;
            foot[r * kBloomStride + bl_slot(c)] = p;
        }
        __syncthreads();
        const int64_t X = X0 + lx, Y = Y0 + ly;
        if (X < (int64_t)cw && Y < (int64_t)ch) {
            // columns 2 lx .. 2 lx + 3 of the footprint: even, odd, even, odd
            const float4* f = foot + (2u * ly) * kBloomStride + lx;
            float rr[4], rg[4], rb[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const float4 a0 = f[j * kBloomStride], a1 = f[j * kBloomStride + kBloomOdd], a2 = f[j * kBloomStride + 1u], a3 = f[j * kBloomStride + kBloomOdd + 1u];
                rr[j] = bl_tap4(a0.x, a1.x, a2.x, a3.x);
                rg[j] = bl_tap4(a0.y, a1.y, a2.y, a3.y);
                rb[j] = bl_tap4(a0.z, a1.z, a2.z, a3.z);
            }
            coarse[(uint64_t)Y * cw + (uint64_t)X] = make_float4(bl_tap4(rr[0], rr[1], rr[2], rr[3]), bl_tap4(rg[0], rg[1], rg[2], rg[3]),
                                                                bl_tap4(rb[0], rb[1], rb[2], rb[3]), 0.0f);
        }
        __syncthreads();                 // the next tile overwrites the footprint
    }
    if (PREFILTER) {
        __shared__ unsigned long long part[kWaves][5];
        unsigned long long counts = (unsigned long long)n_bright | ((unsigned long long)n_invalid << 32);      // two counts per shuffle: neither can carry
        for (int d = 32; d >= 1; d >>= 1) {
            counts += __shfl_xor(counts, d);
            total += __shfl_xor(total, d);
            bright += __shfl_xor(bright, d);
        }
        max_bits = wave_max(max_bits);
        const uint32_t wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0u) {
            part[wave][0] = counts & 0xFFFFFFFFull; part[wave][1] = counts >> 32; part[wave][2] = total; part[wave][3] = bright; part[wave][4] = max_bits;
        }
        __syncthreads();
        if (threadIdx.x < 5u) {
            unsigned long long s = 0ull;
            if (threadIdx.x == 4u) { for (uint32_t v = 0; v < kWaves; v++) s = part[v][4] > s ? part[v][4] : s; }
            else { for (uint32_t v = 0; v < kWaves; v++) s += part[v][threadIdx.x]; }
            if (s != 0ull) {
                switch (threadIdx.x) {
                    case 0u: atomicAdd(&st->bright, (uint32_t)s); break;
                    case 1u: atomicAdd(&st->invalid, (uint32_t)s); break;
                    case 2u: atomicAdd(&st->total_q16, s); break;
                    case 3u: atomicAdd(&st->bright_q16, s); break;
                    default: atomicMax(&st->max_luma_bits, (uint32_t)s); break;
                }
            }
        }
    }
}

// base and out are the same buffer inside the pyramid: neither is __restrict__
__global__ void __launch_bounds__(kBloomThreads)
k_bloom_up(const float4* base, const float4* __restrict__ coarse, float4* out, uint32_t w, uint32_t h, uint32_t cw, uint32_t ch, uint32_t tiles_x,
           uint64_t tiles, float factor)
{
    const uint32_t lx = threadIdx.x & (kBloomTile - 1u), ly = threadIdx.x / kBloomTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const ulonglong2 tile = tile_xy(t, tiles_x);
        const uint64_t x = tile.x * kBloomTile + lx, y = tile.y * kBloomTile + ly;
        if (x >= w || y >= h) continue;
        // bilinear at the texel centres: the nearer coarse texel weighs 0.75, the farther one (edge-clamped) 0.25
        const uint64_t i = x >> 1, k = y >> 1;
        const bool xo = (x & 1ull) != 0ull, yo = (y & 1ull) != 0ull;
        const uint64_t j0 = xo ? i : (i > 0ull ? i - 1ull : 0ull), j1 = xo ? (i + 1ull < cw ? i + 1ull : (uint64_t)cw - 1ull) : i;
        const uint64_t k0 = yo ? k : (k > 0ull ? k - 1ull : 0ull), k1 = yo ? (k + 1ull < ch ? k + 1ull : (uint64_t)ch - 1ull) : k;
        const float a0 = xo ? 0.75f : 0.25f, a1 = xo ? 0.25f : 0.75f, b0 = yo ? 0.75f : 0.25f, b1 = yo ? 0.25f : 0.75f;
        const float4 e00 = coarse[k0 * cw + j0], e01 = coarse[k0 * cw + j1], e10 = coarse[k1 * cw + j0], e11 = coarse[k1 * cw + j1];
        const uint64_t idx = y * w + x;
        float4 c = base[idx];
        const float ur = b0 * (a0 * e00.x + a1 * e01.x) + b1 * (a0 * e10.x + a1 * e11.x);
        const float ug = b0 * (a0 * e00.y + a1 * e01.y) + b1 * (a0 * e10.y + a1 * e11.y);
        const float ub = b0 * (a0 * e00.z + a1 * e01.z) + b1 * (a0 * e10.z + a1 * e11.z);
        c.x = c.x + factor * ur; c.y = c.y + factor * ug; c.z = c.z + factor * ub;
        out[idx] = c;
    }
}

__global__ void __launch_bounds__(64)
k_bloom_finish(BloomState* __restrict__ st, uint32_t levels)
{
    if (threadIdx.x != 0u) return;
    pt_bloom_info r;
    r.levels = levels; r.bright_pixels = st->bright; r.invalid_pixels = st->invalid; r.reserved = 0u;
    r.total_luma_q16 = st->total_q16; r.bright_luma_q16 = st->bright_q16;
    r.max_luma = __uint_as_float(st->max_luma_bits); r.reserved2 = 0u;
    st->record = r;
    st->bright = 0u; st->invalid = 0u; st->max_luma_bits = 0u; st->pad = 0u;
    st->total_q16 = 0ull; st->bright_q16 = 0ull;
}

BloomLevels bloom_levels(uint32_t width, uint32_t height, uint32_t levels)
{
    BloomLevels lv = {};
    lv.w[0] = width; lv.h[0] = height;
    lv.off[1] = 0ull;
    for (uint32_t k = 1u; k <= levels && k <= kBloomMaxLevels; k++) {
        lv.w[k] = (lv.w[k - 1u] + 1u) / 2u; lv.h[k] = (lv.h[k - 1u] + 1u) / 2u;
        lv.off[k + 1u] = lv.off[k] + (uint64_t)lv.w[k] * lv.h[k];
        lv.n = k;
        if (lv.w[k] == 1u && lv.h[k] == 1u) break;
    }
    return lv;
}

hipError_t launch_bloom(const float4* src, uint32_t w, uint32_t h, const pt_bloom_params& bp, float4* out, float4* pyramid, BloomState* st,
                        hipStream_t stream)
{
    const BloomLevels lv = bloom_levels(w, h, bp.levels);
    const BloomPre pre = {bp.threshold, bp.knee, bp.clamp};
    hipError_t e = hipSuccess;
    for (uint32_t k = 1u; k <= lv.n && e == hipSuccess; k++) {              // level k = D of level k - 1
        const TileWalk tw = tile_walk(lv.w[k], lv.h[k], kBloomTile, kBloomBlocks);
        float4* dst = pyramid + lv.off[k];
        if (k == 1u) k_bloom_down<true><<<tw.grid, kBloomThreads, 0, stream>>>(src, w, h, dst, lv.w[1], lv.h[1], tw.tiles_x, tw.tiles, pre, st);
        else k_bloom_down<false><<<tw.grid, kBloomThreads, 0, stream>>>(pyramid + lv.off[k - 1u], lv.w[k - 1u], lv.h[k - 1u], dst, lv.w[k], lv.h[k],
                                                                          tw.tiles_x, tw.tiles, pre, st);
        e = hipGetLastError();
    }
    for (uint32_t k = lv.n - 1u; k >= 1u && e == hipSuccess; k--) {         // E_k = D_k + spread * U(E_(k+1)), in place
        const TileWalk tw = tile_walk(lv.w[k], lv.h[k], kBloomTile, kBloomBlocks);
        float4* own = pyramid + lv.off[k];
        k_bloom_up<<<tw.grid, kBloomThreads, 0, stream>>>(own, pyramid + lv.off[k + 1u], own, lv.w[k], lv.h[k], lv.w[k + 1u], lv.h[k + 1u], tw.tiles_x,
                                                          tw.tiles, bp.spread);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    float norm = 1.0f, t = 1.0f;
    for (uint32_t k = 1u; k < lv.n; k++) { t = t * bp.spread; norm = norm + t; }
    const float gain = bp.intensity / norm;
    const TileWalk tw = tile_walk(w, h, kBloomTile, kBloomBlocks);
    k_bloom_up<<<tw.grid, kBloomThreads, 0, stream>>>(src, pyramid, out, w, h, lv.w[1], lv.h[1], tw.tiles_x, tw.tiles, gain);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_bloom_finish<<<1, 64, 0, stream>>>(st, lv.n);
    return hipGetLastError();
}

}  // namespace ptd
