// multihit.hip — the kernels behind pt_query_multi (include/acgpt.h).
//
//   k_query_multi<FMT, CAP, COUNT>   one ray per lane from a device array: every triangle that tri_test accepts inside (tmin, tmax),
//                                    the first max_hits of them in ascending (t, prim) as hit records, and (COUNT) how many there are.
//                                    CAP = 1, 2, 4 or 8 is the size of the lane's sorted list, the smallest that holds max_hits;
//                                    CAP = 0 is the count-only form, which carries no list.
//
// FMT 11 walks the fp16 centre / half-extent nodes with the box test of traverse_hc.h, FMT 0 the fp32 nodes with the box test of
// traverse<> (pt_device.h), restated here: the node array the scene holds.  256-lane workgroups over a one-dimensional grid, the LDS
// lane stack of query_launch.h (stack_entries * 64 words per wave).  Lanes past n and lanes whose ray is a miss before any traversal stay
// in the wave, inactive.  No atomics: two calls give the same bits.
//
// The list lives in registers.  Every access to it has an index the compiler knows: the insertion is a chain of CAP
// compare-and-swaps, the epilogue takes entry 0 and shifts the rest down once per record.  (An array indexed by a lane's own value
// would go to scratch.)
//
// Two regimes (include/acgpt.h).  COUNT: nothing is pruned at a hit, the far side of a box is cut at the ray's tmax as
// traverse_hc_any cuts it.  Without COUNT the far side is also cut at list[max_hits - 1].t * kTieWiden once the list is full, the
// widening traverse_hc applies to its one hit: a triangle that ties with the last kept hit and has a lower index is still reached.
// Built with -ffp-contract=off: the epilogue is k_query_closest's, evaluated as written.
#include "multihit.h"
#include "bvh_walk.h"

namespace ptd {

struct MultiRay { f3 o, d; float tmin, tmax; bool ok; };

// Ray i of the array, or an inert one for a lane past n: load_query_ray of query.hip.  ok: the lane has a ray and the ray can hit
// something — every origin and direction component finite, tmin and tmax no NaN, tmax > tmin.
__device__ __forceinline__ MultiRay load_multi_ray(const float4* __restrict__ rays, uint32_t i, uint32_t n)
{
    MultiRay r;
    r.o = mk(0.0f); r.d = mk(0.0f, 0.0f, 1.0f); r.tmin = 0.0f; r.tmax = 0.0f; r.ok = false;
    if (i < n) {
        const float4 a = rays[2ull * i], b = rays[2ull * i + 1ull];
        r.o = mk(a.x, a.y, a.z); r.d = mk(a.w, b.x, b.y); r.tmin = b.z; r.tmax = b.w;
        const bool finite = __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) && __builtin_isfinite(a.w) &&
                            __builtin_isfinite(b.x) && __builtin_isfinite(b.y);
        r.ok = finite && r.tmax > r.tmin;      // false when either is a NaN
    }
    return r;
}

// The lane's first hits so far, ascending in (t, prim).  An empty entry is {+inf, -1, 0xFFFFFFFF}: no accepted t is +inf (t < tmax),
// so every hit sorts before it.  N = 0 (count-only) leaves nothing behind.
template <int N>
struct HitList {
    float t[N ? N : 1];
    int slot[N ? N : 1];
    uint32_t prim[N ? N : 1];
};

// Insert (t, slot, prim) among the first max_hits entries; what falls off the end is dropped.  The candidate is carried down the
// list: at each entry it sorts before, the two change places.  Returns the t of entry max_hits - 1.
template <int N>
__device__ __forceinline__ float list_insert(HitList<N>& L, uint32_t max_hits, float t, int slot, uint32_t prim)
{
    float last = INFINITY;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const bool sw = (uint32_t)j < max_hits && (t < L.t[j] || (t == L.t[j] && prim < L.prim[j]));
        const float lt = L.t[j]; const int ls = L.slot[j]; const uint32_t lp = L.prim[j];
        L.t[j] = sw ? t : lt;       t = sw ? lt : t;
        L.slot[j] = sw ? slot : ls; slot = sw ? ls : slot;
        L.prim[j] = sw ? prim : lp; prim = sw ? lp : prim;
        if ((uint32_t)j + 1u == max_hits) last = L.t[j];
    }
    return last;
}

// One ray per lane through the two-child BVH (bvh_walk.h).  Boxes only prune; the triangle test and the interval are traverse_hc's.
// far_cut is the ray's tmax widened (fmaxf: under tmax < 0 the product would move the cut inward); without COUNT it shrinks to the last
// kept hit's t, widened by kTieWiden, once entry max_hits - 1 is filled.  Every triangle sits in one leaf, so each is counted once.
template <int FMT, int CAP, bool COUNT>
struct MultiWalk {
    f3 o, d, mul, add;
    float tmin, tmax, far_cut;
    uint32_t max_hits, count;
    HitList<CAP>& L;      // the kernel's: its epilogue writes the records
    __device__ __forceinline__ MultiWalk(const DeviceScene& sc, const f3& o_, const f3& d_, float tmin_, float tmax_, uint32_t max_hits_, HitList<CAP>& L_)
        : o(o_), d(d_), tmin(tmin_), tmax(tmax_), far_cut(fmaxf(tmax_ * kTieWiden, tmax_)), max_hits(max_hits_), count(0u), L(L_)
    {
#pragma unroll
        for (int j = 0; j < CAP; j++) { L.t[j] = INFINITY; L.slot[j] = -1; L.prim[j] = 0xFFFFFFFFu; }
        if (FMT == 11) setup_ray_hc(o, d, sc.hspace, mul, add);
        else { mul = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z); add = o; }
    }
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace&, bool& h0, bool& h1, bool& first0) const
    {
        // an empty child has a negative half extent, which slab_hc never hits
        float n0, f0, n1, f1;
        slab_hc(qa.x, qa.y, qa.z, mul, add, tmin, n0, f0);
        slab_hc(qb.x, qb.y, qb.z, mul, add, tmin, n1, f1);
        admit_by_interval(n0, fminf(f0, far_cut), n1, fminf(f1, far_cut), h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        // the box test of traverse<> (pt_device.h), restated: mul = 1 / d, add = o
        const float x0 = (a.x - add.x) * mul.x, x1 = (a.w - add.x) * mul.x;
        const float y0 = (a.y - add.y) * mul.y, y1 = (b.x - add.y) * mul.y;
        const float z0 = (a.z - add.z) * mul.z, z1 = (b.y - add.z) * mul.z;
        const float n0 = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), tmin));
        const float f0 = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * kFarWiden;
        const float u0 = (b.z - add.x) * mul.x, u1 = (c.y - add.x) * mul.x;
        const float v0 = (b.w - add.y) * mul.y, v1 = (c.z - add.y) * mul.y;
        const float w0 = (c.x - add.z) * mul.z, w1 = (c.w - add.z) * mul.z;
        const float n1 = fmaxf(fmaxf(fminf(u0, u1), fminf(v0, v1)), fmaxf(fminf(w0, w1), tmin));
        const float f1 = fminf(fminf(fmaxf(u0, u1), fmaxf(v0, v1)), fmaxf(w0, w1)) * kFarWiden;
        admit_by_interval(n0, fminf(f0, far_cut), n1, fminf(f1, far_cut), h0, h1, first0);
        // The one node of a single-triangle scene names its triangle in both children, the second under an empty box, lo = +inf
        // and hi = -inf, whose slabs come out as (-inf, +inf): every ray "hits" it.  traverse<> tests the triangle twice and
        // keeps one hit; a count must not.
        h0 = h0 && a.x <= a.w; h1 = h1 && b.z <= c.y;
    }
    __device__ __forceinline__ bool leaf(int slot, const float4& r0, const float4& r1, const float4& r2)
    {
        float t;
        const bool ok = tri_test(o, d, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x), tmin, tmax, t);
        if (ok) {
            if (COUNT) count++;
            if constexpr (CAP > 0) {
                const float last = list_insert(L, max_hits, t, slot, __float_as_uint(r2.y));
                // +inf while entry max_hits - 1 is empty: the cut stays at the ray's own.  The second product widens a negative t
                // (tmin < 0) outward, which t * kTieWiden alone would move inward
                if (!COUNT) far_cut = fminf(far_cut, fmaxf(last * kTieWiden, last * (2.0f - kTieWiden)));
            }
        }
        return false;
    }
};

template <int FMT, int CAP, bool COUNT>
__global__ void __launch_bounds__(256)
k_query_multi(const DeviceScene sc, uint32_t stack_entries, const float4* __restrict__ rays, uint32_t n, uint32_t max_hits, float4* __restrict__ hits,
              uint32_t* __restrict__ counts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    const MultiRay r = load_multi_ray(rays, i, n);
    HitList<CAP> L;
    MultiWalk<FMT, CAP, COUNT> walk(sc, r.o, r.d, r.tmin, r.tmax, max_hits, L);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, false>(sc, st, r.ok, walk, visits);
    if (i >= n) return;
    if (COUNT) counts[i] = walk.count;
    if constexpr (CAP > 0) {
        float4* out = hits + 2ull * ((unsigned long long)i * max_hits);      // n * max_hits is formed in 64 bits
#pragma unroll 1
        for (uint32_t j = 0; j < max_hits; j++) {
            // the next record is entry 0; the rest move down one, so that no index depends on j
            const float ht = L.t[0];
            const int hslot = L.slot[0];
            const uint32_t hprim = L.prim[0];
#pragma unroll
            for (int k = 0; k + 1 < CAP; k++) { L.t[k] = L.t[k + 1]; L.slot[k] = L.slot[k + 1]; L.prim[k] = L.prim[k + 1]; }
            L.t[CAP - 1] = INFINITY; L.slot[CAP - 1] = -1; L.prim[CAP - 1] = 0xFFFFFFFFu;
            float4 h0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), h1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
            if (hslot >= 0) {
                // k_query_closest's epilogue (query.hip): barycentrics of v1 and v2 in plain multiplies and adds, the normal towards the origin
                const TriRecord* tp = sc.tris + hslot;
                const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
                const f3 v0 = mk(r0.x, r0.y, r0.z), e1 = mk(r0.w, r1.x, r1.y), e2 = mk(r1.z, r1.w, r2.x);
                const f3 p = cross(r.d, e2);
                const float det = dot(e1, p);
                const f3 s = r.o - v0;
                const float u = dot(s, p) / det;
                const f3 q = cross(s, e1);
                const float v = dot(r.d, q) / det;
                const float4 sr = sc.shade[hslot];
                f3 nrm = mk(sr.x, sr.y, sr.z);
                if (dot(nrm, r.d) > 0.0f) nrm = -nrm;
                h0 = make_float4(ht, __uint_as_float(hprim), u, v);
                h1 = make_float4(nrm.x, nrm.y, nrm.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
            }
            out[2u * j] = h0;
            out[2u * j + 1u] = h1;
        }
    }
}

template <int FMT, int CAP, bool COUNT>
static hipError_t launch_multi(const DeviceScene& sc, uint32_t stack_entries, const float4* rays, uint32_t n, uint32_t max_hits, float4* hits, uint32_t* counts,
                               hipStream_t stream)
{
    return launch_lane_stack(k_query_multi<FMT, CAP, COUNT>, stack_entries, n, stream, sc, stack_entries, rays, n, max_hits, hits, counts);
}

template <int FMT>
static hipError_t launch_multi_fmt(const DeviceScene& sc, uint32_t stack_entries, const float4* rays, uint32_t n, uint32_t max_hits, float4* hits,
                                   uint32_t* counts, hipStream_t stream)
{
    if (max_hits == 0u) return launch_multi<FMT, 0, true>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
    if (counts) {
        if (max_hits == 1u) return launch_multi<FMT, 1, true>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
        if (max_hits == 2u) return launch_multi<FMT, 2, true>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
        if (max_hits <= 4u) return launch_multi<FMT, 4, true>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
        return launch_multi<FMT, 8, true>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
    }
    if (max_hits == 1u) return launch_multi<FMT, 1, false>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
    if (max_hits == 2u) return launch_multi<FMT, 2, false>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
    if (max_hits <= 4u) return launch_multi<FMT, 4, false>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
    return launch_multi<FMT, 8, false>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
}

hipError_t launch_query_multi(int fmt, const DeviceScene& sc, uint32_t stack_entries, const float4* rays, uint32_t n, uint32_t max_hits, float4* hits,
                              uint32_t* counts, hipStream_t stream)
{
    if (max_hits > kMultiMaxHits || (max_hits == 0u && !counts) || ((max_hits != 0u) != (hits != nullptr))) return hipErrorInvalidValue;
    if (fmt == 11) return launch_multi_fmt<11>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
    return launch_multi_fmt<0>(sc, stack_entries, rays, n, max_hits, hits, counts, stream);
}

}  // namespace ptd
