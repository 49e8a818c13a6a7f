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
// traverse_nearest's (nearest.hip), statement for statement: the nearer child first, at most one push per visit, one-word entries,
// the same two box bounds.  256-lane workgroups over a one-dimensional grid, the LDS lane stack of query.hip (stack_entries * 64
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

namespace ptd {

extern __shared__ uint32_t nearest_k_lds[];

struct NearKPoint { float d2, v, w; f3 c; };

// nearest.hip's closest_on_triangle, restated: Ericson, Real-Time Collision Detection 5.1.5, on the record's own edge vectors, the
// regions as compares applied as selects in reverse order of priority, one division.  The same statements in the same order under
// the same flags: the same bits as pt_query_nearest's.  A NaN anywhere ends in a NaN d2, which is no candidate.
__device__ __forceinline__ NearKPoint point_to_triangle(const f3& q, const f3& v0, const f3& ab, const f3& ac)
{
    const f3 ap = q - v0;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const f3 bp = ap - ab;
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const f3 cp = ap - ac;
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const bool at_a = d1 <= 0.0f && d2 <= 0.0f;
    const bool at_b = d3 >= 0.0f && d4 <= d3;
    const bool on_ab = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool at_c = d6 >= 0.0f && d5 <= d6;
    const bool on_ac = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool on_bc = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
    float num = 1.0f, den = (va + vb) + vc;
    if (on_bc) { num = e43; den = e43 + e56; }
    if (on_ac) { num = d2; den = d2 - d6; }
    if (on_ab) { num = d1; den = d1 - d3; }
    const float t = num / den;
    float v = vb * t, w = vc * t;
    if (on_bc) { v = 1.0f - t; w = t; }
    if (on_ac) { v = 0.0f; w = t; }
    if (at_c) { v = 0.0f; w = 1.0f; }
    if (on_ab) { v = t; w = 0.0f; }
    if (at_b) { v = 1.0f; w = 0.0f; }
    if (at_a) { v = 0.0f; w = 0.0f; }
    NearKPoint r;
    r.v = v; r.w = w;
    r.c = mk((v0.x + ab.x * v) + ac.x * w, (v0.y + ab.y * v) + ac.y * w, (v0.z + ab.z * v) + ac.z * w);
    const f3 s = q - r.c;
    r.d2 = dot(s, s);
    return r;
}

// nearest.hip's two lower bounds of the squared distance from the point to one child box, restated; a NaN for an empty child, which
// no threshold admits.
__device__ __forceinline__ float near_k_bound_hc(uint32_t px, uint32_t py, uint32_t pz, const f3& qc, const HSpace& hs)
{
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const float tx = __builtin_fmaf((float)hx.x, hs.isx, -qc.x), ty = __builtin_fmaf((float)hy.x, hs.isy, -qc.y), tz = __builtin_fmaf((float)hz.x, hs.isz, -qc.z);
    const float ex = fmaxf(__builtin_fmaf((float)hx.y, -hs.isx, fabsf(tx)), 0.0f);
    const float ey = fmaxf(__builtin_fmaf((float)hy.y, -hs.isy, fabsf(ty)), 0.0f);
    const float ez = fmaxf(__builtin_fmaf((float)hz.y, -hs.isz, fabsf(tz)), 0.0f);
    const float b = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    return (float)hx.y < 0.0f ? __builtin_nanf("") : b;
}
__device__ __forceinline__ float near_k_bound_f32(const f3& q, float lx, float ly, float lz, float hx, float hy, float hz)
{
    const float ex = fmaxf(fmaxf(lx - q.x, q.x - hx), 0.0f), ey = fmaxf(fmaxf(ly - q.y, q.y - hy), 0.0f), ez = fmaxf(fmaxf(lz - q.z, q.z - hz), 0.0f);
    const float b = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    return lx <= hx ? b : __builtin_nanf("");
}

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

// The children of one inner node: their bounds and references.
template <int FMT>
__device__ __forceinline__ void near_k_children(const DeviceScene& sc, int node, const f3& q, const f3& qc, float& b0, float& b1, int& c0, int& c1)
{
    if (FMT == 11) {
        // child references of inner nodes are byte offsets into hcnodes; a leaf is ~slot
        const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
        const uint4 qa = np[0], qb = np[1];
        b0 = near_k_bound_hc(qa.x, qa.y, qa.z, qc, sc.hspace);
        b1 = near_k_bound_hc(qb.x, qb.y, qb.z, qc, sc.hspace);
        c0 = (int)qa.w; c1 = (int)qb.w;
    } else {
        // child 0: lo (a.x a.y a.z) hi (a.w b.x b.y); child 1: lo (b.z b.w c.x) hi (c.y c.z c.w)
        const BvhNode* np = sc.nodes + node;
        const float4 a = np->a, b = np->b, c = np->c;
        const int4 ch = np->d;
        b0 = near_k_bound_f32(q, a.x, a.y, a.z, a.w, b.x, b.y);
        b1 = near_k_bound_f32(q, b.z, b.w, c.x, c.y, c.z, c.w);
        c0 = ch.x; c1 = ch.y;
    }
}

// One point per lane through the two-child BVH: traverse_nearest with a list for its one best.  thr is the cut widened (nearest_k.h):
// r2 under COUNT, min(d2 of entry max_k - 1, r2) otherwise.  Every triangle sits in one leaf, so each is counted once; an empty
// child's bound is a NaN, so the single-triangle scene's second reference to its triangle is never followed.
template <int FMT, int CAP, bool COUNT, bool VISITS>
__device__ __forceinline__ void traverse_nearest_k(const DeviceScene& sc, const LaneStack& st, bool active, const f3& q, float r2, float abs_term,
                                                   uint32_t max_k, NearList<CAP>& L, uint32_t& count, uint2& visits)
{
#pragma unroll
    for (int j = 0; j < CAP; j++) { L.d2[j] = INFINITY; L.slot[j] = -1; L.prim[j] = 0xFFFFFFFFu; }
    count = 0u;
    float thr = r2 * kNearRel + abs_term;
    const f3 qc = mk(q.x - sc.hspace.cx, q.y - sc.hspace.cy, q.z - sc.hspace.cz);
    int sp = 0;
    int node = (active && sc.n_tris != 0u) ? 0 : kSentinel;
    while (node != kSentinel) {
        if (node >= 0) {
            float b0, b1;
            int c0, c1;
            near_k_children<FMT>(sc, node, q, qc, b0, b1, c0, c1);
            if (VISITS) visits.x++;
            const bool h0 = b0 <= thr, h1 = b1 <= thr;          // false for an empty child's NaN
            if (h0 && h1) {
                const bool first0 = b0 <= b1;
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
            const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
            const NearKPoint p = point_to_triangle(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
            if (VISITS) visits.y++;
            if (p.d2 <= r2) {
                if (COUNT) count++;
                if constexpr (CAP > 0) {
                    const float last = near_list_insert(L, max_k, p.d2, slot, __float_as_uint(r2_.y));
                    // +inf while entry max_k - 1 is empty: the cut stays at r2
                    if (!COUNT) thr = fminf(last, r2) * kNearRel + abs_term;
                }
            }
            if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
}

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
    LaneStack st;
    st.base = nearest_k_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    const NearKQuery p = load_near_k_point(points, i, n);
    // a list of 1 or 2 is chosen for max_k = 1 or 2 alone: there max_k is the compiler's, and the list of 1 is k_query_nearest's best
    if (CAP == 1 || CAP == 2) max_k = (uint32_t)CAP;
    NearList<CAP> L;
    uint32_t count;
    uint2 visits = make_uint2(0u, 0u);
    traverse_nearest_k<FMT, CAP, COUNT, VISITS>(sc, st, p.ok, p.q, p.r2, abs_term, max_k, L, count, visits);
    if (i >= n) return;
    if (COUNT) counts[i] = count;
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
                const NearKPoint c = point_to_triangle(p.q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
                const float4 sr = sc.shade[kslot];
                o0 = make_float4(sqrtf(c.d2), __uint_as_float(kprim), c.v, c.w);
                o1 = make_float4(c.c.x, c.c.y, c.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
            }
            rec[2u * j] = o0;
            rec[2u * j + 1u] = o1;
        }
    }
}

// The within-radius walk: the same order of visits under the threshold of r2, one flag instead of a list; the first candidate sets it
// and clears the lane's node.
template <int FMT, bool VISITS>
__global__ void __launch_bounds__(256)
k_query_within_any(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ points, uint32_t n, uint8_t* __restrict__ hit,
                   uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    LaneStack st;
    st.base = nearest_k_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    const NearKQuery p = load_near_k_point(points, i, n);
    const f3 q = p.q;
    const float r2 = p.r2;
    const float thr = r2 * kNearRel + abs_term;
    const f3 qc = mk(q.x - sc.hspace.cx, q.y - sc.hspace.cy, q.z - sc.hspace.cz);
    uint2 visits = make_uint2(0u, 0u);
    bool found = false;
    int sp = 0;
    int node = (p.ok && sc.n_tris != 0u) ? 0 : kSentinel;
    while (node != kSentinel) {
        if (node >= 0) {
            float b0, b1;
            int c0, c1;
            near_k_children<FMT>(sc, node, q, qc, b0, b1, c0, c1);
            if (VISITS) visits.x++;
            const bool h0 = b0 <= thr, h1 = b1 <= thr;          // false for an empty child's NaN
            if (h0 && h1) {
                const bool first0 = b0 <= b1;
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
            const TriRecord* tp = sc.tris + ~node;
            const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
            const NearKPoint c = point_to_triangle(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
            if (VISITS) visits.y++;
            found = c.d2 <= r2;
            if (found || sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
    if (i >= n) return;
    hit[i] = found ? 1u : 0u;
    if (VISITS) visits_out[i] = visits;
}

static size_t near_k_lds_bytes(uint32_t stack_entries) { return (size_t)(256 / 64) * stack_entries * 64u * sizeof(uint32_t); }

template <int FMT, int CAP, bool COUNT, bool VISITS>
static hipError_t launch_near_k(const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, uint32_t max_k, float4* out,
                                uint32_t* counts, uint2* visits, hipStream_t stream)
{
    const size_t lds = near_k_lds_bytes(stack_entries);
    auto kernel = k_query_nearest_k<FMT, CAP, COUNT, VISITS>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<(n + 255u) / 256u, 256, lds, stream>>>(sc, stack_entries, abs_term, points, n, max_k, out, counts, visits);
    return hipGetLastError();
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
    const size_t lds = near_k_lds_bytes(stack_entries);
    auto kernel = k_query_within_any<FMT, VISITS>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<(n + 255u) / 256u, 256, lds, stream>>>(sc, stack_entries, abs_term, points, n, hit, visits);
    return hipGetLastError();
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
