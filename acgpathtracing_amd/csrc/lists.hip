// lists.hip — the kernels behind pt_list_offsets, pt_query_overlap_lists, pt_query_triangles_lists and pt_query_overlap_oriented_lists
// (include/acgpt.h).
//
//   k_list_tile_sums / k_list_scan_tiles / k_list_add_back   the scan: counts -> offsets, 64-bit sums, three launches, no look-back
//   k_fill_lists<FMT, Q, REG>   (k_fill_oriented<FMT, REG> for the oriented boxes of oriented_device.h: the same body, fill_lists)
//                          one query per lane (Q: a box, a triangle or an oriented box), the walk and the leaf test of overlap.hip / tritri.hip through
//                          the shared device headers.  The lane reads its slice [lo, hi) of prims first.  A slice of at most
//                          kListRegister words is the capped kernels' sorted register list, written once in the epilogue: ascending
//                          already.  A longer slice is stored as the walk accepts, in walk order, and its surplus slots are filled
//                          with 0xFFFFFFFF.  A lane whose slice is not lo <= hi <= capacity stores nothing.
//   k_sort_lists           sorts every slice longer than kListRegister in place: each workgroup finds those of its 256 queries by
//                          ballot and takes them one after the other, all 256 lanes on one list — the normalised bitonic network, whose
//                          comparators all put the larger word at the higher index, so a length that is no power of two only skips the
//                          comparators whose upper index is past the end.  Up to kListSortLds words in LDS, beyond that in global memory
//                          with workgroup barriers between steps: one workgroup owns the whole list, so workgroup scope suffices.
//
// 256-lane workgroups over one-dimensional grids; the fill has overlap.hip's LDS lane stack (stack_entries * 64 words per wave).  No
// atomics: the mismatch flag is a plain store of 1 by every lane that raises it.  Two calls give the same bits.  Built with
// -ffp-contract=off like the units it shares the leaf tests with.
#include <type_traits>

#include "lists.h"
#include "bvh_walk.h"
#include "overlap_device.h"      // BoxQuery, AdmitBoth, the sorted register list
#include "tritri_device.h"       // TriQuery
#include "oriented_device.h"     // OBoxQuery

namespace ptd {

typedef unsigned long long u64;

// ---- the scan --------------------------------------------------------------------------------------------------------------------
// Exclusive scan of one value per lane over the 256 lanes of the workgroup, in lane order (Hillis-Steele in LDS); total: the sum of
// all.  s: 256 words of LDS, free again on return.
__device__ __forceinline__ u64 block_scan_exclusive(u64 v, u64* s, u64& total)
{
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
#pragma unroll 1
    for (uint32_t d = 1u; d < 256u; d <<= 1) {
        const u64 x = t >= d ? s[t - d] : 0ull;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const u64 inclusive = s[t];
    total = s[255];
    __syncthreads();
    return inclusive - v;
}

// the lane's kListScanTile / 256 consecutive counts of tile blockIdx.x (0 past n) and their sum.  n <= 2^31 - 1: no index wraps.
__device__ __forceinline__ u64 load_counts(const uint32_t* __restrict__ counts, uint32_t n, uint32_t (&c)[kListScanTile / 256u], uint32_t& first)
{
    first = blockIdx.x * kListScanTile + threadIdx.x * (kListScanTile / 256u);
    u64 sum = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < kListScanTile / 256u; j++) {
        c[j] = first + j < n ? counts[first + j] : 0u;
        sum += c[j];
    }
    return sum;
}

__global__ void __launch_bounds__(256)
k_list_tile_sums(const uint32_t* __restrict__ counts, uint32_t n, u64* __restrict__ sums)
{
    __shared__ u64 s[256];
    uint32_t c[kListScanTile / 256u], first;
    u64 total;
    (void)block_scan_exclusive(load_counts(counts, n, c, first), s, total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}

// One workgroup: sums[0 .. tiles) become their exclusive prefixes, sums[tiles] the total.  Lane t owns the run of `run` consecutive
// tiles from t * run, run = ceil(tiles / kListScanRuns).
__global__ void __launch_bounds__(256)
k_list_scan_tiles(u64* sums, uint32_t tiles)
{
    __shared__ u64 s[256];
    const uint32_t run = (tiles + kListScanRuns - 1u) / kListScanRuns;
    const u64 lo = (u64)threadIdx.x * run, hi = lo + run < (u64)tiles ? lo + run : (u64)tiles;
    u64 sum = 0ull;
    for (u64 k = lo; k < hi; k++) sum += sums[k];
    u64 total;
    u64 prefix = block_scan_exclusive(sum, s, total);
    for (u64 k = lo; k < hi; k++) {
        const u64 v = sums[k];
        sums[k] = prefix;
        prefix += v;
    }
    if (threadIdx.x == 0u) sums[tiles] = total;
}

__global__ void __launch_bounds__(256)
k_list_add_back(const uint32_t* __restrict__ counts, uint32_t n, const u64* __restrict__ sums, uint32_t* __restrict__ offsets)
{
    __shared__ u64 s[256];
    uint32_t c[kListScanTile / 256u], first;
    u64 total;
    u64 prefix = block_scan_exclusive(load_counts(counts, n, c, first), s, total) + sums[blockIdx.x];
    if (blockIdx.x == 0u && threadIdx.x == 0u) offsets[0] = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kListScanTile / 256u; j++) {
        prefix += c[j];
        if (first + j < n) offsets[(size_t)first + j + 1u] = (uint32_t)prefix;
    }
}

hipError_t launch_list_offsets(const uint32_t* counts, uint32_t n, uint32_t* offsets, unsigned long long* scratch, hipStream_t stream)
{
    if (n == 0u || n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    const uint32_t tiles = (n + kListScanTile - 1u) / kListScanTile;
    u64* sums = scratch + 1;
    k_list_tile_sums<<<tiles, 256, 0, stream>>>(counts, n, sums);
    k_list_scan_tiles<<<1, 256, 0, stream>>>(sums, tiles);
    k_list_add_back<<<tiles, 256, 0, stream>>>(counts, n, sums, offsets);
    return hipGetLastError();
}

// ---- the fill ----------------------------------------------------------------------------------------------------------------------
// overlap.hip's walk (bvh_walk.h): of two admitted children the first is entered and the second pushed.  Which triangles are accepted is
// decided by q.accept alone, so the set does not depend on the tree; the order of a long slice does, until k_sort_lists has run.
// in_regs: the slice fits the register list, which the epilogue writes; otherwise out[0 .. m) is stored as the walk accepts.
template <class Q>
struct FillWalk : AdmitBoth<Q> {
    PrimList<kListRegister>& L;      // the kernel's: its epilogue writes the words
    uint32_t* out;
    uint32_t m, count;
    bool in_regs;
    __device__ __forceinline__ FillWalk(const Q& q_, PrimList<kListRegister>& L_, uint32_t* out_, uint32_t m_, bool in_regs_)
        : AdmitBoth<Q>(q_), L(L_), out(out_), m(m_), count(0u), in_regs(in_regs_)
    {
#pragma unroll
        for (uint32_t j = 0; j < kListRegister; j++) L.prim[j] = 0xFFFFFFFFu;
    }
    __device__ __forceinline__ bool leaf(int, const float4& r0, const float4& r1, const float4& r2)
    {
        if (this->q.accept(mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x))) {
            const uint32_t prim = __float_as_uint(r2.y);
            if (in_regs) list_insert(L, kListRegister, prim);
            else if (count < m) out[count] = prim;
            count++;
        }
        return false;
    }
};

// REG: kListRegister, or 0 for the measurement without the register list (every slice stored as the walk finds it).  The body of the
// fill kernels: k_fill_lists for boxes and triangles, k_fill_oriented for oriented boxes.
template <int FMT, class Q, uint32_t REG>
__device__ __forceinline__ void fill_lists(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ recs, uint32_t n,
                                           const uint32_t* __restrict__ offsets, uint32_t* prims, uint32_t capacity, uint32_t* __restrict__ found,
                                           uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    Q q;
    const bool active = q.load(recs, i, n);
    q.prepare(sc, scene_term);
    // the slice: m words from lo, or none where the offsets do not describe a slice inside prims
    uint32_t lo = 0u, m = 0u;
    bool fits = false;
    if (i < n) {
        lo = offsets[i];
        const uint32_t hi = offsets[(size_t)i + 1u];
        fits = lo <= hi && hi <= capacity;
        m = fits ? hi - lo : 0u;
    }
    uint32_t* out = prims + lo;                 // read or written at j < m only: m == 0 where prims is null (capacity == 0)
    const bool in_regs = m <= REG;
    PrimList<kListRegister> L;
    FillWalk<Q> walk(q, L, out, m, in_regs);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, active, walk, visits);
    const uint32_t count = walk.count;
    if (i >= n) return;
    if (found) found[i] = count;
    if (!fits || count > m) *flag = 1u;         // every writer stores the same word
    if (in_regs) {
#pragma unroll 1
        for (uint32_t j = 0; j < m; j++) {
            // the next word is entry 0; the rest move down one, so that no index depends on j.  Behind the indices: 0xFFFFFFFF
            out[j] = L.prim[0];
#pragma unroll
            for (uint32_t k = 0; k + 1u < kListRegister; k++) L.prim[k] = L.prim[k + 1u];
            L.prim[kListRegister - 1u] = 0xFFFFFFFFu;
        }
    } else {
#pragma unroll 1
        for (uint32_t j = count; j < m; j++) out[j] = 0xFFFFFFFFu;
    }
}

template <int FMT, class Q, uint32_t REG>
__global__ void __launch_bounds__(256)
k_fill_lists(const DeviceScene sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ recs, uint32_t n, const uint32_t* __restrict__ offsets,
             uint32_t* prims, uint32_t capacity, uint32_t* __restrict__ found, uint32_t* __restrict__ flag)
{
    fill_lists<FMT, Q, REG>(sc, stack_entries, scene_term, recs, n, offsets, prims, capacity, found, flag);
}

// The same fill for the 64-byte records of pt_query_overlap_oriented_lists (oriented_device.h), under a name of its own.
template <int FMT, uint32_t REG>
__global__ void __launch_bounds__(256)
k_fill_oriented(const DeviceScene sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ recs, uint32_t n, const uint32_t* __restrict__ offsets,
                uint32_t* prims, uint32_t capacity, uint32_t* __restrict__ found, uint32_t* __restrict__ flag)
{
    fill_lists<FMT, OBoxQuery, REG>(sc, stack_entries, scene_term, recs, n, offsets, prims, capacity, found, flag);
}

// ---- the sort ----------------------------------------------------------------------------------------------------------------------
// One compare-exchange: the larger word goes to the higher index.  i < l always; a comparator whose upper index is past the end is
// skipped, which is what the network does with a list padded by words larger than all.
__device__ __forceinline__ void compare_exchange(uint32_t* a, uint32_t i, uint32_t l, uint32_t m)
{
    if (l < m) {
        const uint32_t x = a[i], y = a[l];
        if (x > y) { a[i] = y; a[l] = x; }
    }
}

// All 256 lanes sort a[0 .. m) ascending, m >= 2.  levels = ceil(log2 m); every step has 2^(levels - 1) comparators, dealt to the lanes
// round robin, and a workgroup barrier behind it.  Level kb merges sorted blocks of 2^(kb - 1) into blocks of 2^kb: its first step
// compares word r of a block with word 2^kb - 1 - r, the steps after it words 2^jb apart, jb = kb - 2 .. 0.  Index arithmetic stays
// below 2^32 for every m a 32-bit offset can describe.
__device__ __forceinline__ void bitonic_sort(uint32_t* a, uint32_t m)
{
    const uint32_t levels = 32u - (uint32_t)__builtin_clz(m - 1u);
    const uint32_t half = 1u << (levels - 1u);
#pragma unroll 1
    for (uint32_t kb = 1u; kb <= levels; kb++) {
        const uint32_t flip = (2u << (kb - 1u)) - 1u;
#pragma unroll 1
        for (uint32_t t = threadIdx.x; t < half; t += 256u) {
            const uint32_t i = ((t >> (kb - 1u)) << (kb - 1u) << 1) + (t & (flip >> 1));
            compare_exchange(a, i, i ^ flip, m);
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t jb = kb - 1u; jb-- != 0u;) {
            const uint32_t j = 1u << jb;
#pragma unroll 1
            for (uint32_t t = threadIdx.x; t < half; t += 256u) {
                const uint32_t i = ((t >> jb) << jb << 1) + (t & (j - 1u));
                compare_exchange(a, i, i + j, m);
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256)
k_sort_lists(const uint32_t* __restrict__ offsets, uint32_t n, uint32_t* prims, uint32_t capacity, uint32_t sorted_up_to)
{
    __shared__ uint32_t keys[kListSortLds];
    __shared__ u64 wanted[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool want = false;
    if (i < n) {
        const uint32_t lo = offsets[i], hi = offsets[(size_t)i + 1u];
        want = lo <= hi && hi <= capacity && hi - lo > sorted_up_to;      // the slices k_fill_lists stored in walk order
    }
    const u64 mask = vote(want);
    if ((threadIdx.x & 63u) == 0u) wanted[threadIdx.x >> 6] = mask;
    __syncthreads();
    // every lane reads the same four masks, so the loops and the barriers inside them are uniform over the workgroup
#pragma unroll 1
    for (uint32_t w = 0; w < 4u; w++) {
        u64 left = wanted[w];
#pragma unroll 1
        while (left != 0ull) {
            const uint32_t b = (uint32_t)__builtin_ctzll(left);
            left &= left - 1ull;
            const size_t qi = (size_t)blockIdx.x * 256u + w * 64u + b;
            const uint32_t lo = offsets[qi], m = offsets[qi + 1u] - lo;
            uint32_t* a = prims + lo;
            if (m <= kListSortLds) {
                for (uint32_t t = threadIdx.x; t < m; t += 256u) keys[t] = a[t];
                __syncthreads();
                bitonic_sort(keys, m);
                for (uint32_t t = threadIdx.x; t < m; t += 256u) a[t] = keys[t];
                __syncthreads();
            } else {
                bitonic_sort(a, m);
            }
        }
    }
}

template <int FMT, class Q, uint32_t REG>
static hipError_t launch_fill(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* recs, uint32_t n, const uint32_t* offsets,
                              uint32_t* prims, uint32_t capacity, uint32_t* found, uint32_t* flag, uint32_t phases, hipStream_t stream)
{
    if (phases & kListPhaseFill) {
        hipError_t e;
        if constexpr (std::is_same<Q, OBoxQuery>::value)
            e = launch_lane_stack(k_fill_oriented<FMT, REG>, stack_entries, n, stream, sc, stack_entries, scene_term, recs, n, offsets, prims, capacity, found, flag);
        else
            e = launch_lane_stack(k_fill_lists<FMT, Q, REG>, stack_entries, n, stream, sc, stack_entries, scene_term, recs, n, offsets, prims, capacity, found, flag);
        if (e != hipSuccess) return e;
    }
    // a slice of one word is sorted as it is
    if (phases & kListPhaseSort) k_sort_lists<<<(n + 255u) / 256u, 256, 0, stream>>>(offsets, n, prims, capacity, REG ? REG : 1u);
    return hipGetLastError();
}

template <int FMT, class Q>
static hipError_t launch_fill_phases(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* recs, uint32_t n, const uint32_t* offsets,
                                     uint32_t* prims, uint32_t capacity, uint32_t* found, uint32_t* flag, uint32_t phases, hipStream_t stream)
{
    if (phases & kListPhaseNoRegisters) return launch_fill<FMT, Q, 0u>(sc, stack_entries, scene_term, recs, n, offsets, prims, capacity, found, flag, phases, stream);
    return launch_fill<FMT, Q, kListRegister>(sc, stack_entries, scene_term, recs, n, offsets, prims, capacity, found, flag, phases, stream);
}

hipError_t launch_overlap_lists(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, const uint32_t* offsets,
                                uint32_t* prims, uint32_t capacity, uint32_t* found, uint32_t* flag, uint32_t phases, hipStream_t stream)
{
    if (n == 0u || n > 0x7FFFFFFFu || (!prims && capacity != 0u)) return hipErrorInvalidValue;
    if (fmt == 11) return launch_fill_phases<11, BoxQuery>(sc, stack_entries, scene_term, boxes, n, offsets, prims, capacity, found, flag, phases, stream);
    return launch_fill_phases<0, BoxQuery>(sc, stack_entries, scene_term, boxes, n, offsets, prims, capacity, found, flag, phases, stream);
}

hipError_t launch_oriented_lists(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, const uint32_t* offsets,
                                 uint32_t* prims, uint32_t capacity, uint32_t* found, uint32_t* flag, uint32_t phases, hipStream_t stream)
{
    if (n == 0u || n > 0x7FFFFFFFu || (!prims && capacity != 0u)) return hipErrorInvalidValue;
    if (fmt == 11) return launch_fill_phases<11, OBoxQuery>(sc, stack_entries, scene_term, boxes, n, offsets, prims, capacity, found, flag, phases, stream);
    return launch_fill_phases<0, OBoxQuery>(sc, stack_entries, scene_term, boxes, n, offsets, prims, capacity, found, flag, phases, stream);
}

hipError_t launch_triangles_lists(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, const uint32_t* offsets,
                                  uint32_t* prims, uint32_t capacity, uint32_t* found, uint32_t* flag, uint32_t phases, hipStream_t stream)
{
    if (n == 0u || n > 0x7FFFFFFFu || (!prims && capacity != 0u)) return hipErrorInvalidValue;
    if (fmt == 11) return launch_fill_phases<11, TriQuery>(sc, stack_entries, scene_term, tris, n, offsets, prims, capacity, found, flag, phases, stream);
    return launch_fill_phases<0, TriQuery>(sc, stack_entries, scene_term, tris, n, offsets, prims, capacity, found, flag, phases, stream);
}

}  // namespace ptd
