// multihit.hip — the kernels behind pt_query_multi (include/acgpt.h).
//
//   k_query_multi<FMT, CAP, COUNT>   one ray per lane from a device array: every triangle that tri_test accepts inside (tmin, tmax),
//                                    the first max_hits of them in ascending (t, prim) as hit records, and (COUNT) how many there are.
//                                    CAP = 1, 2, 4 or 8 is the size of the lane's sorted list, the smallest that holds max_hits;
//                                    CAP = 0 is the count-only form, which carries no list.
//
// FMT 11 walks the fp16 centre / half-extent nodes with the box test of traverse_hc.h, FMT 0 the fp32 nodes with the box test of
// traverse<> (pt_device.h), restated here: the node array the scene holds.  256-lane workgroups over a one-dimensional grid, the LDS
// lane stack of query.hip (stack_entries * 64 words per wave).  Lanes past n and lanes whose ray is a miss before any traversal stay
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

namespace ptd {

extern __shared__ uint32_t multihit_lds[];

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

// One ray per lane through the two-child BVH.  Boxes only prune; the triangle test and the interval are traverse_hc's.  far_cut is
// the ray's tmax widened (fmaxf: under tmax < 0 the product would move the cut inward); without COUNT it shrinks to the last kept
// hit's t, widened by kTieWiden, once entry max_hits - 1 is filled.  Every triangle sits in one leaf, so each is counted once.
template <int FMT, int CAP, bool COUNT>
__device__ __forceinline__ void traverse_multi(const DeviceScene& sc, const LaneStack& st, bool active, const f3& o, const f3& d, float tmin, float tmax,
                                               uint32_t max_hits, HitList<CAP>& L, uint32_t& count)
{
#pragma unroll
    for (int j = 0; j < CAP; j++) { L.t[j] = INFINITY; L.slot[j] = -1; L.prim[j] = 0xFFFFFFFFu; }
    count = 0u;
    f3 mul, add;
    if (FMT == 11) setup_ray_hc(o, d, sc.hspace, mul, add);
    else { mul = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z); add = o; }
    float far_cut = fmaxf(tmax * kTieWiden, tmax);
    int sp = 0;
    int node = (active && sc.n_tris != 0u) ? 0 : kSentinel;
    while (node != kSentinel) {
        if (node >= 0) {
            float n0, f0, n1, f1;
            int c0, c1;
            bool e0 = false, e1 = false;      // an empty child box
            if (FMT == 11) {
                // child references of inner nodes are byte offsets into hcnodes; a leaf is ~slot
                const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
                const uint4 qa = np[0], qb = np[1];
                slab_hc(qa.x, qa.y, qa.z, mul, add, tmin, n0, f0);
                slab_hc(qb.x, qb.y, qb.z, mul, add, tmin, n1, f1);
                c0 = (int)qa.w; c1 = (int)qb.w;
            } else {
                // child 0: lo (a.x a.y a.z) hi (a.w b.x b.y); child 1: lo (b.z b.w c.x) hi (c.y c.z c.w).  mul = 1 / d, add = o
                const BvhNode* np = sc.nodes + node;
                const float4 a = np->a, b = np->b, c = np->c;
                const int4 ch = np->d;
                const float x0 = (a.x - add.x) * mul.x, x1 = (a.w - add.x) * mul.x;
                const float y0 = (a.y - add.y) * mul.y, y1 = (b.x - add.y) * mul.y;
                const float z0 = (a.z - add.z) * mul.z, z1 = (b.y - add.z) * mul.z;
                n0 = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), tmin));
                f0 = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * kFarWiden;
                const float u0 = (b.z - add.x) * mul.x, u1 = (c.y - add.x) * mul.x;
                const float v0 = (b.w - add.y) * mul.y, v1 = (c.z - add.y) * mul.y;
                const float w0 = (c.x - add.z) * mul.z, w1 = (c.w - add.z) * mul.z;
                n1 = fmaxf(fmaxf(fminf(u0, u1), fminf(v0, v1)), fmaxf(fminf(w0, w1), tmin));
                f1 = fminf(fminf(fmaxf(u0, u1), fmaxf(v0, v1)), fmaxf(w0, w1)) * kFarWiden;
                c0 = ch.x; c1 = ch.y;
                // The one node of a single-triangle scene names its triangle in both children, the second under an empty box, lo = +inf
                // and hi = -inf, whose slabs come out as (-inf, +inf): every ray "hits" it.  traverse<> tests the triangle twice and
                // keeps one hit; a count must not.  (The fp16 nodes mark an empty child with a negative half extent, which slab_hc
                // never hits.)
                e0 = !(a.x <= a.w); e1 = !(b.z <= c.y);
            }
            f0 = fminf(f0, far_cut);
            f1 = fminf(f1, far_cut);
            const bool h0 = n0 <= f0 && !e0, h1 = n1 <= f1 && !e1;
            if (h0 && h1) {
                const bool first0 = n0 <= n1;
                st.push(sp, first0 ? c1 : c0);
                sp++;
                node = first0 ? c0 : c1;
            } else if (h0) {
                node = c0;
            } else if (h1) {
                node = c1;
            } else {
                if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
            }
        } else {
            const int slot = ~node;
            const TriRecord* tp = sc.tris + slot;
            const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
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
            if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
}

template <int FMT, int CAP, bool COUNT>
__global__ void __launch_bounds__(256)
k_query_multi(const DeviceScene sc, uint32_t stack_entries, const float4* __restrict__ rays, uint32_t n, uint32_t max_hits, float4* __restrict__ hits,
              uint32_t* __restrict__ counts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    LaneStack st;
    st.base = multihit_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    const MultiRay r = load_multi_ray(rays, i, n);
    HitList<CAP> L;
    uint32_t count;
    traverse_multi<FMT, CAP, COUNT>(sc, st, r.ok, r.o, r.d, r.tmin, r.tmax, max_hits, L, count);
    if (i >= n) return;
    if (COUNT) counts[i] = count;
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
    const size_t lds = (size_t)(256 / 64) * stack_entries * 64u * sizeof(uint32_t);
    auto kernel = k_query_multi<FMT, CAP, COUNT>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<(n + 255u) / 256u, 256, lds, stream>>>(sc, stack_entries, rays, n, max_hits, hits, counts);
    return hipGetLastError();
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
