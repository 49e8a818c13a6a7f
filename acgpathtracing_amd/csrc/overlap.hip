// overlap.hip — the kernels behind pt_query_overlap and pt_query_overlap_any (include/acgpt.h).
//
//   k_query_overlap<FMT, CAP, MODE>   one axis-aligned box per lane from a device array: every triangle the separating-axis test
//                                     accepts.  MODE kList keeps the lowest max_prims indices among them, ascending, in a sorted list
//                                     of CAP = 1, 4 or 8 entries (the smallest that holds max_prims; CAP = 0 carries no list) and
//                                     counts them; kAny leaves at the first accepted triangle and writes one byte; kVisits is the
//                                     counting walk that also writes how many inner nodes the lane visited and how many triangles
//                                     it tested (the test hook's instantiation).
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk prunes by the
// per-axis gap between the query box's centre and each child box, the leaves run the triangle-box test.  256-lane workgroups over a
// one-dimensional grid, the LDS lane stack of query.hip (stack_entries * 64 words per wave).  A box is two 16-byte loads per lane.
// Lanes past n and lanes whose box is a miss before any traversal stay in the wave, inactive.  No atomics: two calls give the same
// bits.
//
// The list lives in registers, as multihit.hip keeps its list: the insertion is a chain of CAP compare-and-swaps, the epilogue
// takes entry 0 and shifts the rest down once per word, so every access has an index the compiler knows.
// Built with -ffp-contract=off: the triangle-box test is evaluated as written, and tests/overlap_ref.py mirrors it operation for
// operation.  The child boxes are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "overlap.h"

namespace ptd {

extern __shared__ uint32_t overlap_lds[];

enum { kList = 0, kAny = 1, kVisits = 2 };

__device__ __forceinline__ float fmin3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float fmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// One of the nine edge axes, cross(unit i, f) with (j, k) the two axes after i: the three vertices projected, against the box's radius.
// A NaN radius, or three NaN projections, separates.
__device__ __forceinline__ bool edge_axis_keeps(float p0j, float p0k, float p1j, float p1k, float p2j, float p2k, float fj, float fk, float hj, float hk)
{
    const float s0 = p0k * fj - p0j * fk, s1 = p1k * fj - p1j * fk, s2 = p2k * fj - p2j * fk;
    const float r = hj * fabsf(fk) + hk * fabsf(fj);
    return fmin3(s0, s1, s2) <= r && fmax3(s0, s1, s2) >= -r;
}
__device__ __forceinline__ bool edge_keeps(const f3& p0, const f3& p1, const f3& p2, const f3& f, const f3& h)
{
    const bool x = edge_axis_keeps(p0.y, p0.z, p1.y, p1.z, p2.y, p2.z, f.y, f.z, h.y, h.z);
    const bool y = edge_axis_keeps(p0.z, p0.x, p1.z, p1.x, p2.z, p2.x, f.z, f.x, h.z, h.x);
    const bool z = edge_axis_keeps(p0.x, p0.y, p1.x, p1.y, p2.x, p2.y, f.x, f.y, h.x, h.y);
    return x & y & z;
}

// Does the triangle {v0, v0 + e1, v0 + e2} overlap the box of centre c and half extent h: the separating-axis test of Akenine-Moeller
// (Fast 3D Triangle-Box Overlap Testing) in keep form, the three box faces, the triangle's plane and the nine edge axes, on the
// record's own vectors.  The 13 conditions are closed (touching overlaps) and combined without a branch, so a wave's lanes run one
// instruction stream.
__device__ __forceinline__ bool tri_box_overlap(const f3& c, const f3& h, const f3& v0, const f3& e1, const f3& e2)
{
    const f3 p0 = v0 - c, p1 = p0 + e1, p2 = p0 + e2;
    const bool faces = (fmin3(p0.x, p1.x, p2.x) <= h.x) & (fmax3(p0.x, p1.x, p2.x) >= -h.x) &
                       (fmin3(p0.y, p1.y, p2.y) <= h.y) & (fmax3(p0.y, p1.y, p2.y) >= -h.y) &
                       (fmin3(p0.z, p1.z, p2.z) <= h.z) & (fmax3(p0.z, p1.z, p2.z) >= -h.z);
    const f3 nrm = cross(e1, e2);
    const float d = dot(nrm, p0);
    const float r = (h.x * fabsf(nrm.x) + h.y * fabsf(nrm.y)) + h.z * fabsf(nrm.z);
    const bool plane = (d <= r) & (d >= -r);
    const f3 f1 = e2 - e1;
    return faces & plane & edge_keeps(p0, p1, p2, e1, h) & edge_keeps(p0, p1, p2, f1, h) & edge_keeps(p0, p1, p2, e2, h);
}

// The per-axis gap between the query centre and one child box, e_k = max(|centre_k - c_k| - half_k, 0); NaNs for an empty child, which
// no compare admits.
//   FMT 11: qc = c - centre of HSpace, once per lane; per axis t = g_c * is - qc (g_c, g_h the fp16 centre and half extent: world =
//           g * is + centre), e = max(|t| - g_h * is, 0): two v_fma_mix_f32 and a max, box_bound_hc's decode.  An empty child has g_h < 0.
//   FMT 0:  e = max(lo - c, c - hi, 0) from the fp32 planes.  An empty child has lo = +inf.
__device__ __forceinline__ bool child_admitted_hc(uint32_t px, uint32_t py, uint32_t pz, const f3& qc, const HSpace& hs, const f3& thr)
{
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const float tx = __builtin_fmaf((float)hx.x, hs.isx, -qc.x), ty = __builtin_fmaf((float)hy.x, hs.isy, -qc.y), tz = __builtin_fmaf((float)hz.x, hs.isz, -qc.z);
    float ex = fmaxf(__builtin_fmaf((float)hx.y, -hs.isx, fabsf(tx)), 0.0f);
    const float ey = fmaxf(__builtin_fmaf((float)hy.y, -hs.isy, fabsf(ty)), 0.0f);
    const float ez = fmaxf(__builtin_fmaf((float)hz.y, -hs.isz, fabsf(tz)), 0.0f);
    ex = (float)hx.y < 0.0f ? __builtin_nanf("") : ex;
    return (ex <= thr.x) & (ey <= thr.y) & (ez <= thr.z);
}
__device__ __forceinline__ bool child_admitted_f32(const f3& c, float lx, float ly, float lz, float hx, float hy, float hz, const f3& thr)
{
    float ex = fmaxf(fmaxf(lx - c.x, c.x - hx), 0.0f);
    const float ey = fmaxf(fmaxf(ly - c.y, c.y - hy), 0.0f), ez = fmaxf(fmaxf(lz - c.z, c.z - hz), 0.0f);
    ex = lx <= hx ? ex : __builtin_nanf("");
    return (ex <= thr.x) & (ey <= thr.y) & (ez <= thr.z);
}

// The lane's lowest triangle indices so far, ascending.  An empty entry is 0xFFFFFFFF, which is no triangle's index (n_tris < 2^32 - 1)
// and sorts behind every one.  N = 0 leaves nothing behind.
template <int N>
struct PrimList { uint32_t prim[N ? N : 1]; };

// Insert prim among the first max_prims entries; what falls off the end is dropped.  The candidate is carried down the list: at each
// entry it sorts before, the two change places.  Every triangle sits in one leaf, so no index comes twice.
template <int N>
__device__ __forceinline__ void list_insert(PrimList<N>& L, uint32_t max_prims, uint32_t prim)
{
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint32_t lp = L.prim[j];
        const bool sw = (uint32_t)j < max_prims && prim < lp;
        L.prim[j] = sw ? prim : lp;
        prim = sw ? lp : prim;
    }
}

// One box per lane through the two-child BVH.  thr = h + margin per axis (overlap.h): a child is entered iff its gap is at most thr on
// all three axes; of two such children the first is entered and the second pushed.  A visit pushes at most one reference and descends
// one level, so the references on the stack belong to siblings of nodes on the current root-to-node path, at most one per level: the
// depth the ray walks need (size_stack, capi.hip: max_depth + 1) holds here too.  A popped reference is entered without a second look
// at its own box.  The boxes only prune: which triangles overlap is decided by tri_box_overlap alone, whatever order the walk reaches
// them in.
template <int FMT, int CAP, int MODE>
__device__ __forceinline__ void traverse_overlap(const DeviceScene& sc, const LaneStack& st, bool active, const f3& c, const f3& h, float scene_term,
                                                 uint32_t max_prims, PrimList<CAP>& L, uint32_t& count, uint2& visits)
{
#pragma unroll
    for (int j = 0; j < CAP; j++) L.prim[j] = 0xFFFFFFFFu;
    count = 0u;
    const f3 thr = mk(h.x + (scene_term + (fabsf(c.x) + h.x) * kOverlapQuery), h.y + (scene_term + (fabsf(c.y) + h.y) * kOverlapQuery),
                      h.z + (scene_term + (fabsf(c.z) + h.z) * kOverlapQuery));
    const f3 qc = mk(c.x - sc.hspace.cx, c.y - sc.hspace.cy, c.z - sc.hspace.cz);
    int sp = 0;
    int node = (active && sc.n_tris != 0u) ? 0 : kSentinel;
    while (node != kSentinel) {
        if (node >= 0) {
            bool h0, h1;
            int c0, c1;
            if (FMT == 11) {
                // child references of inner nodes are byte offsets into hcnodes; a leaf is ~slot
                const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
                const uint4 qa = np[0], qb = np[1];
                h0 = child_admitted_hc(qa.x, qa.y, qa.z, qc, sc.hspace, thr);
                h1 = child_admitted_hc(qb.x, qb.y, qb.z, qc, sc.hspace, thr);
                c0 = (int)qa.w; c1 = (int)qb.w;
            } else {
                // child 0: lo (a.x a.y a.z) hi (a.w b.x b.y); child 1: lo (b.z b.w c.x) hi (c.y c.z c.w)
                const BvhNode* np = sc.nodes + node;
                const float4 a = np->a, b = np->b, cc = np->c;
                const int4 ch = np->d;
                h0 = child_admitted_f32(c, a.x, a.y, a.z, a.w, b.x, b.y, thr);
                h1 = child_admitted_f32(c, b.z, b.w, cc.x, cc.y, cc.z, cc.w, thr);
                c0 = ch.x; c1 = ch.y;
            }
            if (MODE == kVisits) visits.x++;
            if (h0 && h1) {
                st.push(sp, c1);
                sp++;
                node = c0;
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
            const bool ok = tri_box_overlap(c, h, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x));
            if (MODE == kVisits) visits.y++;
            if (ok) {
                count++;
                if (MODE == kAny) { node = kSentinel; continue; }
                if constexpr (CAP > 0) list_insert(L, max_prims, __float_as_uint(r2.y));
            }
            if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
}

// out8: the any byte per box (kAny).  prims / counts: the list and the number (kList; either may be null), counts alone (kVisits).
template <int FMT, int CAP, int MODE>
__global__ void __launch_bounds__(256)
k_query_overlap(const DeviceScene sc, uint32_t stack_entries, float scene_term, const float4* __restrict__ boxes, uint32_t n, uint32_t max_prims,
                uint32_t* __restrict__ prims, uint32_t* __restrict__ counts, uint8_t* __restrict__ out8, uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    LaneStack st;
    st.base = overlap_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    // box i of the array, or an inert one for a lane past n.  ok: the lane has a box and the box can overlap something — centre and
    // half extent finite, no half extent negative or NaN (include/acgpt.h: "a miss before any traversal").  -0 is a zero.
    f3 c = mk(0.0f), h = mk(0.0f);
    bool ok = false;
    if (i < n) {
        const float4 a = boxes[2ull * i], b = boxes[2ull * i + 1ull];
        c = mk(a.x, a.y, a.z);
        h = mk(a.w, b.x, b.y);
        ok = __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z) && __builtin_isfinite(a.w) && __builtin_isfinite(b.x) &&
             __builtin_isfinite(b.y) && a.w >= 0.0f && b.x >= 0.0f && b.y >= 0.0f;
    }
    PrimList<CAP> L;
    uint32_t count;
    uint2 visits = make_uint2(0u, 0u);
    traverse_overlap<FMT, CAP, MODE>(sc, st, ok, c, h, scene_term, max_prims, L, count, visits);
    if (i >= n) return;
    if (MODE == kAny) { out8[i] = count != 0u ? 1 : 0; return; }
    if (counts) counts[i] = count;
    if (MODE == kVisits) visits_out[i] = visits;
    if constexpr (CAP > 0) {
        uint32_t* out = prims + (unsigned long long)i * max_prims;      // n * max_prims is formed in 64 bits
#pragma unroll 1
        for (uint32_t j = 0; j < max_prims; j++) {
            // the next word is entry 0; the rest move down one, so that no index depends on j
            out[j] = L.prim[0];
#pragma unroll
            for (int k = 0; k + 1 < CAP; k++) L.prim[k] = L.prim[k + 1];
            L.prim[CAP - 1] = 0xFFFFFFFFu;
        }
    }
}

template <int FMT, int CAP, int MODE>
static hipError_t launch_overlap(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                 uint32_t* prims, uint32_t* counts, uint8_t* out8, uint2* visits, hipStream_t stream)
{
    const size_t lds = (size_t)(256 / 64) * stack_entries * 64u * sizeof(uint32_t);
    auto kernel = k_query_overlap<FMT, CAP, MODE>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<(n + 255u) / 256u, 256, lds, stream>>>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, out8, visits);
    return hipGetLastError();
}

template <int FMT>
static hipError_t launch_overlap_fmt(const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                     uint32_t* prims, uint32_t* counts, hipStream_t stream)
{
    if (max_prims == 0u) return launch_overlap<FMT, 0, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    if (max_prims == 1u) return launch_overlap<FMT, 1, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    if (max_prims <= 4u) return launch_overlap<FMT, 4, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
    return launch_overlap<FMT, 8, kList>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, nullptr, nullptr, stream);
}

float overlap_scene_term(const float scene_lo[3], const float scene_hi[3])
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) {
        const double a = fabs((double)scene_lo[k]), b = fabs((double)scene_hi[k]);
        if (a > s && a < (double)INFINITY) s = a;
        if (b > s && b < (double)INFINITY) s = b;
    }
    const double t = s * (double)kOverlapScene;
    float f = (float)t;
    if ((double)f < t) f = nextafterf(f, INFINITY);
    return f;
}

hipError_t launch_query_overlap(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t max_prims,
                                uint32_t* prims, uint32_t* counts, hipStream_t stream)
{
    if (max_prims > kOverlapMaxPrims || (max_prims == 0u && !counts) || ((max_prims != 0u) != (prims != nullptr))) return hipErrorInvalidValue;
    if (fmt == 11) return launch_overlap_fmt<11>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, stream);
    return launch_overlap_fmt<0>(sc, stack_entries, scene_term, boxes, n, max_prims, prims, counts, stream);
}

hipError_t launch_query_overlap_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint8_t* hit,
                                    hipStream_t stream)
{
    if (fmt == 11) return launch_overlap<11, 0, kAny>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, nullptr, hit, nullptr, stream);
    return launch_overlap<0, 0, kAny>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, nullptr, hit, nullptr, stream);
}

hipError_t launch_overlap_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, uint32_t* counts,
                                 uint2* visits, hipStream_t stream)
{
    if (fmt == 11) return launch_overlap<11, 0, kVisits>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, counts, nullptr, visits, stream);
    return launch_overlap<0, 0, kVisits>(sc, stack_entries, scene_term, boxes, n, 0u, nullptr, counts, nullptr, visits, stream);
}

}  // namespace ptd
