// nearest_k.hip — the kernels behind pt_query_nearest_k and pt_query_within_any (include/acgpt.h).
//
//   k_query_nearest_k<FMT, CAP, COUNT, VISITS>   one point per lane from a device array: every triangle whose d2 is at most
//                                    max_radius^2, the first max_k of them in ascending (d2, prim) as pt_query_nearest's records,
//                                    and (COUNT) how many there are.  CAP = 1, 2, 4 or 8 is the size of the lane's sorted list,
//                                    the smallest that holds max_k; CAP = 0 is the count-only form, which carries no list.
//   k_query_within_any<FMT, VISITS>  one byte per point: 1 iff a triangle lies within max_radius.  The lane leaves at its first.
//
// VISITS also writes how many inner nodes the lane visited and how many triangles it tested (the test hook's instantiations).
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk is
// nearest.hip's (bvh_walk.h) under the same admission: the nearer child first, at most one push per visit, one-word entries, the same
// two box bounds (closest_point.h).  256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h (stack_entries * 64
// words per wave).  Lanes past n and lanes whose point is a miss before any traversal stay in the wave, inactive.  No atomics: two
// calls give the same bits.
//
// The list is multihit.hip's, in registers: every access has an index the compiler knows, the insertion is a chain of CAP
// compare-and-swaps, the epilogue takes entry 0 and shifts the rest down once per record.  The walk carries d2 alone out of a leaf;
// the weights and the point are computed in the epilogue from the kept slot, once per record.
//
// Two regimes (include/acgpt.h).  COUNT: nothing is pruned at a candidate, the threshold stays at r2's.  Without COUNT it follows
// min(d2 of entry max_k - 1, r2) once that entry is filled.  The box test is closed (<=) and the threshold widened (nearest.h), so
// a triangle that ties with the last kept entry and has a lower index is still reached.
// Built with -ffp-contract=off: the triangle test is evaluated as written, and tests/nearest_ref.py mirrors it operation for
// operation.  The box bounds are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "nearest_k.h"
#include "bvh_walk.h"
#include "closest_point.h"      // closest_on_triangle, box_bound_hc / box_bound_f32: pt_query_nearest's own

namespace ptd {

// The lane's closest candidates so far, ascending in (d2, prim).  An empty entry is {+inf, -1, 0xFFFFFFFF}: a candidate whose d2
// overflowed to +inf (max_radius = +inf) still sorts before it by its triangle index.  N = 0 (count-only) leaves nothing behind.
template <int N>
struct NearList {
    float d2[N ? N : 1];
    int slot[N ? N : 1];
    uint32_t prim[N ? N : 1];
};

// Insert (d2, slot, prim) among the first max_k entries; what falls off the end is dropped.  The candidate is carried down the
// list: at each entry it sorts before, the two change places.  Returns the d2 of entry max_k - 1.
template <int N>
__device__ __forceinline__ float near_list_insert(NearList<N>& L, uint32_t max_k, float d2, int slot, uint32_t prim)
{
    float last = INFINITY;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const bool sw = (uint32_t)j < max_k && (d2 < L.d2[j] || (d2 == L.d2[j] && prim < L.prim[j]));
        const float ld = L.d2[j]; const int ls = L.slot[j]; const uint32_t lp = L.prim[j];
        L.d2[j] = sw ? d2 : ld;     d2 = sw ? ld : d2;
        L.slot[j] = sw ? slot : ls; slot = sw ? ls : slot;
        L.prim[j] = sw ? prim : lp; prim = sw ? lp : prim;
        if ((uint32_t)j + 1u == max_k) last = L.d2[j];
    }
    return last;
}

// The admission both walks share: the two box bounds of the point against the threshold of the moment, the nearer child first.
struct NearKPrune {
    f3 q, qc;
    float r2, thr;
    __device__ __forceinline__ NearKPrune(const DeviceScene& sc, const f3& q_, float r2_, float abs_term)
        : q(q_), qc(mk(q_.x - sc.hspace.cx, q_.y - sc.hspace.cy, q_.z - sc.hspace.cz)), r2(r2_), thr(r2_ * kNearRel + abs_term) {}
    __device__ __forceinline__ void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0) const
    {
        admit_by_bound(box_bound_hc(qa.x, qa.y, qa.z, qc, hs), box_bound_hc(qb.x, qb.y, qb.z, qc, hs), thr, h0, h1, first0);
    }
    __device__ __forceinline__ void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0) const
    {
        admit_by_bound(box_bound_f32(q, a.x, a.y, a.z, a.w, b.x, b.y), box_bound_f32(q, b.z, b.w, c.x, c.y, c.z, c.w), thr, h0, h1, first0);
    }
};

// One point per lane through the two-child BVH (bvh_walk.h): nearest.hip's walk with a list for its one best.  thr is the cut widened
// (nearest_k.h): r2 under COUNT, min(d2 of entry max_k - 1, r2) otherwise.  Every triangle sits in one leaf, so each is counted once; an
// empty child's bound is a NaN, so the single-triangle scene's second reference to its triangle is never followed.
template <int CAP, bool COUNT>
struct NearKWalk : NearKPrune {
    float abs_term;
    uint32_t max_k, count;
    NearList<CAP>& L;      // the kernel's: its epilogue writes the records
    __device__ __forceinline__ NearKWalk(const DeviceScene& sc, const f3& q_, float r2_, float abs_term_, uint32_t max_k_, NearList<CAP>& L_)
        : NearKPrune(sc, q_, r2_, abs_term_), abs_term(abs_term_), max_k(max_k_), count(0u), L(L_)
    {
#pragma unroll
        for (int j = 0; j < CAP; j++) { L.d2[j] = INFINITY; L.slot[j] = -1; L.prim[j] = 0xFFFFFFFFu; }
    }
    __device__ __forceinline__ bool leaf(int slot, const float4& r0, const float4& r1, const float4& r2_)
    {
        const ClosestPoint p = closest_on_triangle(q, r0, r1, r2_);
        if (p.d2 <= r2) {
            if (COUNT) count++;
            if constexpr (CAP > 0) {
                const float last = near_list_insert(L, max_k, p.d2, slot, __float_as_uint(r2_.y));
                // +inf while entry max_k - 1 is empty: the cut stays at r2
                if (!COUNT) thr = fminf(last, r2) * kNearRel + abs_term;
            }
        }
        return false;
    }
};

// The within-radius walk: the same order of visits under the threshold of r2, one flag instead of a list; the first candidate sets it
// and ends the lane.
struct WithinWalk : NearKPrune {
    bool found;
    __device__ __forceinline__ WithinWalk(const DeviceScene& sc, const f3& q_, float r2_, float abs_term) : NearKPrune(sc, q_, r2_, abs_term), found(false) {}
    __device__ __forceinline__ bool leaf(int, const float4& r0, const float4& r1, const float4& r2_)
    {
        found = closest_on_triangle(q, r0, r1, r2_).d2 <= r2;
        return found;
    }
};

// Point i of the array, or an inert one for a lane past n.  ok: the lane has a point and the point can find something — every
// coordinate finite, max_radius >= 0 and no NaN (include/acgpt.h: "a miss before any traversal").
struct NearKQuery { f3 q; float r2; bool ok; };
__device__ __forceinline__ NearKQuery load_near_k_point(const float4* __restrict__ points, uint32_t i, uint32_t n)
{
    NearKQuery r;
    r.q = mk(0.0f); r.r2 = 0.0f; r.ok = false;
    if (i < n) {
        const float4 p = points[i];
        r.q = mk(p.x, p.y, p.z);
        r.r2 = p.w * p.w;
        r.ok = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z) && p.w >= 0.0f;      // false when max_radius is a NaN
    }
    return r;
}

template <int FMT, int CAP, bool COUNT, bool VISITS>
__global__ void __launch_bounds__(256)
k_query_nearest_k(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ points, uint32_t n, uint32_t max_k,
                  float4* __restrict__ out, uint32_t* __restrict__ counts, uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    const NearKQuery p = load_near_k_point(points, i, n);
    // a list of 1 or 2 is chosen for max_k = 1 or 2 alone: there max_k is the compiler's, and the list of 1 is k_query_nearest's best
    if (CAP == 1 || CAP == 2) max_k = (uint32_t)CAP;
    NearList<CAP> L;
    NearKWalk<CAP, COUNT> walk(sc, p.q, p.r2, abs_term, max_k, L);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, VISITS>(sc, st, p.ok, walk, visits);
    if (i >= n) return;
    if (COUNT) counts[i] = walk.count;
    if (VISITS) visits_out[i] = visits;
    if constexpr (CAP > 0) {
        float4* rec = out + 2ull * ((unsigned long long)i * max_k);      // n * max_k is formed in 64 bits
#pragma unroll 1
        for (uint32_t j = 0; j < max_k; j++) {
            // the next record is entry 0; the rest move down one, so that no index depends on j
            const int kslot = L.slot[0];
            const uint32_t kprim = L.prim[0];
#pragma unroll
            for (int k = 0; k + 1 < CAP; k++) { L.d2[k] = L.d2[k + 1]; L.slot[k] = L.slot[k + 1]; L.prim[k] = L.prim[k + 1]; }
            L.d2[CAP - 1] = INFINITY; L.slot[CAP - 1] = -1; L.prim[CAP - 1] = 0xFFFFFFFFu;
            float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
            if (kslot >= 0) {
                // k_query_nearest's epilogue: the kept triangle once more, the same function on the same inputs, the same bits
                const TriRecord* tp = sc.tris + kslot;
                const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
                const ClosestPoint c = closest_on_triangle(p.q, r0, r1, r2_);
                const float4 sr = sc.shade[kslot];
                o0 = make_float4(sqrtf(c.d2), __uint_as_float(kprim), c.v, c.w);
                o1 = make_float4(c.c.x, c.c.y, c.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
            }
            rec[2u * j] = o0;
            rec[2u * j + 1u] = o1;
        }
    }
}

template <int FMT, bool VISITS>
__global__ void __launch_bounds__(256)
k_query_within_any(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ points, uint32_t n, uint8_t* __restrict__ hit,
                   uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack st = lane_stack(stack_entries);
    const NearKQuery p = load_near_k_point(points, i, n);
    WithinWalk walk(sc, p.q, p.r2, abs_term);
    uint2 visits = make_uint2(0u, 0u);
    bvh_walk<FMT, VISITS>(sc, st, p.ok, walk, visits);
    if (i >= n) return;
    hit[i] = walk.found ? 1u : 0u;
    if (VISITS) visits_out[i] = visits;
}

template <int FMT, int CAP, bool COUNT, bool VISITS>
static hipError_t launch_near_k(const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint32_t max_k, float4* out,
                                uint32_t* counts, uint2* visits, hipStream_t stream)
{
    return launch_lane_stack(k_query_nearest_k<FMT, CAP, COUNT, VISITS>, stack_entries, n, stream, sc, stack_entries, abs_term, points, n, max_k, out, counts, visits);
}

template <int FMT, bool VISITS>
static hipError_t launch_near_k_fmt(const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint32_t max_k, float4* out,
                                    uint32_t* counts, uint2* visits, hipStream_t stream)
{
    if (max_k > kNearestMaxK || (max_k == 0u && !counts) || ((max_k != 0u) != (out != nullptr))) return hipErrorInvalidValue;
    if (max_k == 0u) return launch_near_k<FMT, 0, true, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
    if (counts) {
        if (max_k == 1u) return launch_near_k<FMT, 1, true, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
        if (max_k == 2u) return launch_near_k<FMT, 2, true, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
        if (max_k <= 4u) return launch_near_k<FMT, 4, true, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
        return launch_near_k<FMT, 8, true, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
    }
    if (max_k == 1u) return launch_near_k<FMT, 1, false, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
    if (max_k == 2u) return launch_near_k<FMT, 2, false, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
    if (max_k <= 4u) return launch_near_k<FMT, 4, false, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
    return launch_near_k<FMT, 8, false, VISITS>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
}

template <int FMT, bool VISITS>
static hipError_t launch_within(const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint8_t* hit, uint2* visits,
                                hipStream_t stream)
{
    return launch_lane_stack(k_query_within_any<FMT, VISITS>, stack_entries, n, stream, sc, stack_entries, abs_term, points, n, hit, visits);
}

hipError_t launch_query_nearest_k(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint32_t max_k,
                                  float4* out, uint32_t* counts, hipStream_t stream)
{
    if (fmt == 11) return launch_near_k_fmt<11, false>(sc, stack_entries, abs_term, points, n, max_k, out, counts, nullptr, stream);
    return launch_near_k_fmt<0, false>(sc, stack_entries, abs_term, points, n, max_k, out, counts, nullptr, stream);
}

hipError_t launch_query_within_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint8_t* hit,
                                   hipStream_t stream)
{
    if (fmt == 11) return launch_within<11, false>(sc, stack_entries, abs_term, points, n, hit, nullptr, stream);
    return launch_within<0, false>(sc, stack_entries, abs_term, points, n, hit, nullptr, stream);
}

hipError_t launch_nearest_k_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint32_t max_k,
                                   float4* out, uint32_t* counts, uint8_t* hit, uint2* visits, uint32_t mode, hipStream_t stream)
{
    if (!visits || mode > 1u) return hipErrorInvalidValue;
    if (mode == 1u) {
        if (!hit) return hipErrorInvalidValue;
        if (fmt == 11) return launch_within<11, true>(sc, stack_entries, abs_term, points, n, hit, visits, stream);
        return launch_within<0, true>(sc, stack_entries, abs_term, points, n, hit, visits, stream);
    }
    if (fmt == 11) return launch_near_k_fmt<11, true>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
    return launch_near_k_fmt<0, true>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits, stream);
}

}  // namespace ptd
