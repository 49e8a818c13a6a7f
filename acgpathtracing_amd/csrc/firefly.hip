// firefly.hip — the kernels behind pt_firefly_filter (include/acgpt.h).
//
//   k_firefly_filter<RADIUS>  one workgroup of 256 lanes per 16 x 16 tile and step (the grid strides over the tiles), one pixel per lane:
//                             a 16-byte load of the lane's own pixel, kept in registers; the tile's luminances and their halo of RADIUS
//                             (18^2 or 20^2 floats, -1 for an invalid or out-of-image entry) in LDS, the halo loaded by the first 68 or
//                             144 lanes; the rank-th largest neighbour through a branch-free insertion list of four registers; one
//                             16-byte store.  An invalid pixel (the rare path) reads its valid neighbours' colours from global memory.
//                             Counts, sums and the max go through wave shuffles and LDS to one vector atomic per workgroup and field
//   k_firefly_finish          one lane: copies the live counts into the record and clears them for the next call
//
// Every expression is mirrored operation for operation by tests/firefly_ref.py (fp32, same order; this file is built with
// -ffp-contract=off).  The reductions are integer sums and a max of bit patterns: the order of the atomics cannot change a bit, and
// neighbours are read from src only, so two calls give the same bits.
#include "firefly.h"
#include "image_common.h"

namespace ptd {

__device__ __forceinline__ bool ff_valid(float l) { return l >= 0.0f && l <= 3.402823466e+38f; }
__device__ __forceinline__ unsigned long long ff_q16(float x) { return (unsigned long long)(fminf(x, 16777216.0f) * 65536.0f); }

// the list m0 >= m1 >= m2 >= m3 of the largest values so far takes v
__device__ __forceinline__ void ff_insert(float& m0, float& m1, float& m2, float& m3, float v)
{
    float hi;
    hi = fmaxf(m0, v); v = fminf(m0, v); m0 = hi;
    hi = fmaxf(m1, v); v = fminf(m1, v); m1 = hi;
    hi = fmaxf(m2, v); v = fminf(m2, v); m2 = hi;
    m3 = fmaxf(m3, v);
}

template <int RADIUS>
__global__ void __launch_bounds__(kFireflyThreads)
k_firefly_filter(const float4* __restrict__ src, float4* __restrict__ out, uint32_t w, uint32_t h, uint32_t tiles_x, uint64_t tiles, float ratio,
                 float floor_lum, uint32_t rank, FireflyState* __restrict__ st)
{
    constexpr int kTile = (int)kFireflyTile, kSide = kTile + 2 * RADIUS, kHalo = kSide * kSide - kTile * kTile, kStride = (int)kFireflyStride;
    constexpr uint32_t kWaves = kFireflyThreads / 64u;
    static_assert(kHalo <= (int)kFireflyThreads && kSide <= kStride, "one halo entry per lane at the most");
    __shared__ float lds[kSide * kStride];
    __shared__ unsigned long long part[kWaves][6];
    const int tid = (int)threadIdx.x, lx = tid & (kTile - 1), ly = tid / kTile;        // a wave covers four rows of the tile
    // this lane's halo entry: the RADIUS rows below the tile, the RADIUS rows above it, then the 2 RADIUS columns beside each tile row
    int hrow = 0, hcol = 0;
    if (tid < 2 * RADIUS * kSide) {
        const int r = tid / kSide;
        hrow = r < RADIUS ? r : kTile + r;
        hcol = tid - r * kSide;
    } else if (tid < kHalo) {
        const int e = tid - 2 * RADIUS * kSide, r = e / (2 * RADIUS), c = e - r * (2 * RADIUS);
        hrow = RADIUS + r;
        hcol = c < RADIUS ? c : kTile + c;
    }
    uint32_t n_clamped = 0u, n_replaced = 0u, n_passed = 0u, max_bits = 0u;
    unsigned long long total = 0ull, removed = 0ull;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const ulonglong2 tile = tile_xy(t, tiles_x);
        const int64_t x0 = (int64_t)(tile.x * kFireflyTile), y0 = (int64_t)(tile.y * kFireflyTile);
        const int64_t x = x0 + lx, y = y0 + ly;
        const bool inside = x < (int64_t)w && y < (int64_t)h;
        const uint64_t i = (uint64_t)y * w + (uint64_t)x;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float l = -1.0f;
        bool ok = false;
        if (inside) {
            c = src[i];
            l = image_lum(c.x, c.y, c.z);
            ok = ff_valid(l);
        }
        lds[(ly + RADIUS) * kStride + lx + RADIUS] = ok ? l : -1.0f;
        if (tid < kHalo) {
            const int64_t qx = x0 + hcol - RADIUS, qy = y0 + hrow - RADIUS;
            float v = -1.0f;
            if (qx >= 0 && qx < (int64_t)w && qy >= 0 && qy < (int64_t)h) {
                const float4 q = src[(uint64_t)qy * w + (uint64_t)qx];
                const float lq = image_lum(q.x, q.y, q.z);
                if (ff_valid(lq)) v = lq;
            }
            lds[hrow * kStride + hcol] = v;
        }
        __syncthreads();
        if (inside) {
            const float* centre = lds + (ly + RADIUS) * kStride + lx + RADIUS;
            float m0 = -1.0f, m1 = -1.0f, m2 = -1.0f, m3 = -1.0f;
            uint32_t n = 0u;
#pragma unroll
            for (int dy = -RADIUS; dy <= RADIUS; dy++)
#pragma unroll
                for (int dx = -RADIUS; dx <= RADIUS; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    const float v = centre[dy * kStride + dx];
                    n += v >= 0.0f ? 1u : 0u;
                    ff_insert(m0, m1, m2, m3, v);
                }
            if (ok) {
                const float ref = rank == 1u ? m0 : (rank == 2u ? m1 : (rank == 3u ? m2 : m3));
                const float lim = ratio * fmaxf(ref, floor_lum);
                const bool clamp = n >= rank && l > lim;
                if (clamp) {
                    const float s = lim / l;
                    c.x = c.x * s; c.y = c.y * s; c.z = c.z * s;
                    const uint32_t over = __float_as_uint(l / lim);
                    max_bits = over > max_bits ? over : max_bits;
                    removed += ff_q16(l - lim);
                    n_clamped++;
                } else {
                    n_passed++;
                }
                total += ff_q16(l);
            } else {
                // the rare path: the mean of the valid neighbours' colours, added in tap order; an entry >= 0 is inside the image
                float sr = 0.0f, sg = 0.0f, sb = 0.0f;
                for (int dy = -RADIUS; dy <= RADIUS; dy++)
                    for (int dx = -RADIUS; dx <= RADIUS; dx++) {
                        if ((dx == 0 && dy == 0) || !(centre[dy * kStride + dx] >= 0.0f)) continue;
                        const float4 q = src[(uint64_t)(y + dy) * w + (uint64_t)(x + dx)];
                        sr = sr + q.x; sg = sg + q.y; sb = sb + q.z;
                    }
                if (n != 0u) { const float d = (float)n; c.x = sr / d; c.y = sg / d; c.z = sb / d; }
                else { c.x = 0.0f; c.y = 0.0f; c.z = 0.0f; }
                n_replaced++;
            }
            out[i] = c;
        }
        __syncthreads();                 // the next tile overwrites the luminances
    }
    unsigned long long counts = (unsigned long long)n_clamped | ((unsigned long long)n_replaced << 32);      // two counts per shuffle: neither can carry
    unsigned long long passed = n_passed;
    for (int d = 32; d >= 1; d >>= 1) {
        counts += __shfl_xor(counts, d);
        passed += __shfl_xor(passed, d);
        total += __shfl_xor(total, d);
        removed += __shfl_xor(removed, d);
    }
    max_bits = wave_max(max_bits);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        part[wave][0] = counts & 0xFFFFFFFFull; part[wave][1] = counts >> 32; part[wave][2] = passed;
        part[wave][3] = total; part[wave][4] = removed; part[wave][5] = max_bits;
    }
    __syncthreads();
    if (threadIdx.x < 6u) {
        unsigned long long s = 0ull;
        if (threadIdx.x == 5u) { for (uint32_t v = 0; v < kWaves; v++) s = part[v][5] > s ? part[v][5] : s; }
        else { for (uint32_t v = 0; v < kWaves; v++) s += part[v][threadIdx.x]; }
        if (s != 0ull) {
            switch (threadIdx.x) {
                case 0u: atomicAdd(&st->clamped, (uint32_t)s); break;
                case 1u: atomicAdd(&st->replaced, (uint32_t)s); break;
                case 2u: atomicAdd(&st->passed, (uint32_t)s); break;
                case 3u: atomicAdd(&st->total_q16, s); break;
                case 4u: atomicAdd(&st->removed_q16, s); break;
                default: atomicMax(&st->max_ratio_bits, (uint32_t)s); break;
            }
        }
    }
}

__global__ void __launch_bounds__(64)
k_firefly_finish(FireflyState* __restrict__ st)
{
    if (threadIdx.x != 0u) return;
    pt_firefly_info r;
    r.clamped_pixels = st->clamped; r.replaced_pixels = st->replaced; r.passed_pixels = st->passed; r.reserved = 0u;
    r.total_luma_q16 = st->total_q16; r.removed_luma_q16 = st->removed_q16;
    r.max_ratio = __uint_as_float(st->max_ratio_bits); r.reserved2 = 0u;
    st->record = r;
    st->clamped = 0u; st->replaced = 0u; st->passed = 0u; st->max_ratio_bits = 0u;
    st->total_q16 = 0ull; st->removed_q16 = 0ull;
}

hipError_t launch_firefly(const float4* src, uint32_t w, uint32_t h, const pt_firefly_params& fp, float4* out, FireflyState* st, hipStream_t stream)
{
    const TileWalk tw = tile_walk(w, h, kFireflyTile, kFireflyBlocks);
    if (fp.radius == 1u) k_firefly_filter<1><<<tw.grid, kFireflyThreads, 0, stream>>>(src, out, w, h, tw.tiles_x, tw.tiles, fp.ratio, fp.floor, fp.rank, st);
    else k_firefly_filter<2><<<tw.grid, kFireflyThreads, 0, stream>>>(src, out, w, h, tw.tiles_x, tw.tiles, fp.ratio, fp.floor, fp.rank, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_firefly_finish<<<1, 64, 0, stream>>>(st);
    return hipGetLastError();
}

}  // namespace ptd
