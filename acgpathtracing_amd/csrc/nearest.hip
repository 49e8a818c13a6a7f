// nearest.hip — the kernels behind pt_query_nearest (include/acgpt.h).
//
//   k_query_nearest<FMT, COUNT>   one point per lane from a device array: the closest triangle within max_radius, then the record
//                                 (distance, triangle, weights of v1 and v2, closest point, material).  COUNT also writes how many
//                                 inner nodes the lane visited and how many triangles it tested (the test hook's instantiation).
//
// FMT 11 walks the fp16 centre / half-extent nodes, FMT 0 the fp32 nodes: the node array the scene holds.  The walk is ordered by a
// lower bound of the squared distance from the point to each child box instead of a ray's slab interval, and the leaves run a
// point-to-triangle test.  256-lane workgroups over a one-dimensional grid, the LDS lane stack of query.hip (stack_entries * 64
// words per wave).  A point is one 16-byte load and a record two 16-byte stores per lane.  Lanes past n and lanes whose point is a
// miss before any traversal stay in the wave, inactive.  No atomics: two calls give the same bits.
// Built with -ffp-contract=off: the triangle test is evaluated as written, and tests/nearest_ref.py mirrors it operation for
// operation.  The box bounds are outside that contract (they only prune) and use explicit fused multiply-adds.
#include "nearest.h"

namespace ptd {

extern __shared__ uint32_t nearest_lds[];

struct NearPoint { float d2, v, w; f3 c; };

// Closest point of the triangle {v0, v0 + ab, v0 + ac} to q: Ericson, Real-Time Collision Detection 5.1.5, on the record's own edge
// vectors.  The regions are decided by compares on d1..d6 and va, vb, vc and applied as selects in reverse order of priority (vertex
// A, vertex B, edge AB, vertex C, edge AC, edge BC, face), so a wave's lanes run one instruction stream; the one division of the
// region that wins is selected before it is taken.  (v, w): the weights of v1 and v2.  A NaN anywhere ends in a NaN d2, which is no
// candidate.
__device__ __forceinline__ NearPoint closest_on_triangle(const f3& q, const f3& v0, const f3& ab, const f3& ac)
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
    NearPoint r;
    r.v = v; r.w = w;
    r.c = mk((v0.x + ab.x * v) + ac.x * w, (v0.y + ab.y * v) + ac.y * w, (v0.z + ab.z * v) + ac.z * w);
    const f3 s = q - r.c;
    r.d2 = dot(s, s);
    return r;
}

struct NearBest { float d2; int slot; uint32_t prim; };

// Lower bound of the squared distance from the point to one child box; a NaN for an empty child, which no threshold admits (+inf
// would pass under max_radius = +inf, where the threshold is +inf too).
//   FMT 11: qc = q - centre of HSpace, once per lane; per axis t = c * is - qc (c, h the fp16 centre and half extent: world = g * is +
//           centre), e = max(|t| - h * is, 0): two v_fma_mix_f32 and a max.  An empty child has h < 0.
//   FMT 0:  e = max(lo - q, q - hi, 0) from the fp32 planes.  An empty child has lo = +inf.
__device__ __forceinline__ float box_bound_hc(uint32_t px, uint32_t py, uint32_t pz, const f3& qc, const HSpace& hs)
{
    const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
    const float tx = __builtin_fmaf((float)hx.x, hs.isx, -qc.x), ty = __builtin_fmaf((float)hy.x, hs.isy, -qc.y), tz = __builtin_fmaf((float)hz.x, hs.isz, -qc.z);
    const float ex = fmaxf(__builtin_fmaf((float)hx.y, -hs.isx, fabsf(tx)), 0.0f);
    const float ey = fmaxf(__builtin_fmaf((float)hy.y, -hs.isy, fabsf(ty)), 0.0f);
    const float ez = fmaxf(__builtin_fmaf((float)hz.y, -hs.isz, fabsf(tz)), 0.0f);
    const float b = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    return (float)hx.y < 0.0f ? __builtin_nanf("") : b;
}
__device__ __forceinline__ float box_bound_f32(const f3& q, float lx, float ly, float lz, float hx, float hy, float hz)
{
    const float ex = fmaxf(fmaxf(lx - q.x, q.x - hx), 0.0f), ey = fmaxf(fmaxf(ly - q.y, q.y - hy), 0.0f), ez = fmaxf(fmaxf(lz - q.z, q.z - hz), 0.0f);
    const float b = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    return lx <= hx ? b : __builtin_nanf("");
}

// One point per lane through the two-child BVH.  thr is min(best d2, r2) widened (nearest.h): a child is entered iff its bound is at
// most thr and it is not empty; of two such children the nearer is entered and the other pushed.  A visit pushes at most one
// reference and descends one level, so the references on the stack belong to siblings of nodes on the current root-to-node path, at
// most one per level: the depth the ray walks need (size_stack, capi.hip: max_depth + 1) holds here too.  A popped reference is
// entered without a second look at its own box — its children are tested against the threshold of that moment, a popped leaf is
// tested —, so an entry is one word.  The boxes only prune: the winner is decided by the triangle test, d2 <= r2, smallest d2, ties
// to the lowest triangle index, whatever order the walk reaches the triangles in.
template <int FMT, bool COUNT>
__device__ __forceinline__ void traverse_nearest(const DeviceScene& sc, const LaneStack& st, bool active, const f3& q, float r2, float abs_term,
                                                 NearBest& best, uint2& visits)
{
    best.d2 = INFINITY; best.slot = -1; best.prim = 0xFFFFFFFFu;
    float thr = r2 * kNearRel + abs_term;
    const f3 qc = mk(q.x - sc.hspace.cx, q.y - sc.hspace.cy, q.z - sc.hspace.cz);
    int sp = 0;
    int node = (active && sc.n_tris != 0u) ? 0 : kSentinel;
    while (node != kSentinel) {
        if (node >= 0) {
            float b0, b1;
            int c0, c1;
            if (FMT == 11) {
                // child references of inner nodes are byte offsets into hcnodes; a leaf is ~slot
                const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
                const uint4 qa = np[0], qb = np[1];
                b0 = box_bound_hc(qa.x, qa.y, qa.z, qc, sc.hspace);
                b1 = box_bound_hc(qb.x, qb.y, qb.z, qc, sc.hspace);
                c0 = (int)qa.w; c1 = (int)qb.w;
            } else {
                // child 0: lo (a.x a.y a.z) hi (a.w b.x b.y); child 1: lo (b.z b.w c.x) hi (c.y c.z c.w)
                const BvhNode* np = sc.nodes + node;
                const float4 a = np->a, b = np->b, c = np->c;
                const int4 ch = np->d;
                b0 = box_bound_f32(q, a.x, a.y, a.z, a.w, b.x, b.y);
                b1 = box_bound_f32(q, b.z, b.w, c.x, c.y, c.z, c.w);
                c0 = ch.x; c1 = ch.y;
            }
            if (COUNT) visits.x++;
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
            const NearPoint p = closest_on_triangle(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
            const uint32_t prim = __float_as_uint(r2_.y);
            if (COUNT) visits.y++;
            if (p.d2 <= r2 && (p.d2 < best.d2 || (p.d2 == best.d2 && prim < best.prim))) {
                best.d2 = p.d2; best.slot = slot; best.prim = prim;
                thr = p.d2 * kNearRel + abs_term;
            }
            if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
}

template <int FMT, bool COUNT>
__global__ void __launch_bounds__(256)
k_query_nearest(const DeviceScene sc, uint32_t stack_entries, float abs_term, const float4* __restrict__ points, uint32_t n, float4* __restrict__ out,
                uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    LaneStack st;
    st.base = nearest_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    // point i of the array, or an inert one for a lane past n.  ok: the lane has a point and the point can find something — every
    // coordinate finite, max_radius >= 0 and no NaN (include/acgpt.h: "a miss before any traversal")
    f3 q = mk(0.0f);
    float r2 = 0.0f;
    bool ok = false;
    if (i < n) {
        const float4 p = points[i];
        q = mk(p.x, p.y, p.z);
        r2 = p.w * p.w;
        ok = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z) && p.w >= 0.0f;      // false when max_radius is a NaN
    }
    NearBest best;
    uint2 visits = make_uint2(0u, 0u);
    traverse_nearest<FMT, COUNT>(sc, st, ok, q, r2, abs_term, best, visits);
    if (i >= n) return;
    float4 o0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    if (ok && best.slot >= 0) {
        // the winner's triangle once more: the same function on the same inputs gives the same bits, and the walk carries three
        // registers for its best candidate instead of eight
        const TriRecord* tp = sc.tris + best.slot;
        const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
        const NearPoint p = closest_on_triangle(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
        const float4 sr = sc.shade[best.slot];
        o0 = make_float4(sqrtf(p.d2), __uint_as_float(best.prim), p.v, p.w);
        o1 = make_float4(p.c.x, p.c.y, p.c.z, __uint_as_float(__float_as_uint(sr.w) & kShadeMatMask));
    }
    out[2ull * i] = o0;
    out[2ull * i + 1ull] = o1;
    if (COUNT) visits_out[i] = visits;
}

template <typename K>
static hipError_t launch_nearest(K kernel, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, float4* out,
                                 uint2* visits, hipStream_t stream)
{
    const size_t lds = (size_t)(256 / 64) * stack_entries * 64u * sizeof(uint32_t);
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<(n + 255u) / 256u, 256, lds, stream>>>(sc, stack_entries, abs_term, points, n, out, visits);
    return hipGetLastError();
}

float nearest_abs_term(const float scene_lo[3], const float scene_hi[3])
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) {
        const double a = fabs((double)scene_lo[k]), b = fabs((double)scene_hi[k]);
        if (a > s && a < (double)INFINITY) s = a;
        if (b > s && b < (double)INFINITY) s = b;
    }
    const double t = s * s * (double)kNearAbs;
    float f = (float)t;
    if ((double)f < t) f = nextafterf(f, INFINITY);
    return f;
}

hipError_t launch_query_nearest(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, float4* out,
                                hipStream_t stream)
{
    if (fmt == 11) return launch_nearest(k_query_nearest<11, false>, sc, stack_entries, abs_term, points, n, out, nullptr, stream);
    return launch_nearest(k_query_nearest<0, false>, sc, stack_entries, abs_term, points, n, out, nullptr, stream);
}

hipError_t launch_nearest_visits(int fmt, const DeviceScene& sc, uint32_t stack_entries, float abs_term, const float4* points, uint32_t n, float4* out,
                                 uint2* visits, hipStream_t stream)
{
    if (fmt == 11) return launch_nearest(k_query_nearest<11, true>, sc, stack_entries, abs_term, points, n, out, visits, stream);
    return launch_nearest(k_query_nearest<0, true>, sc, stack_entries, abs_term, points, n, out, visits, stream);
}

}  // namespace ptd
