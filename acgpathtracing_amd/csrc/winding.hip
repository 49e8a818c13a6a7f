// winding.hip — the kernels behind pt_query_winding (include/acgpt.h).
//
//   k_wd_parents   parent of every node and leaf slot, from whichever node array holds the topology
//   k_wd_moments   bottom-up, one thread per leaf slot; the second thread to reach a node combines its two children's stored sums,
//                  child 0 first (arrive twice; agent-scope acq_rel counters carry the children's sums between CUs).  The counters
//                  decide who combines, never what: every sum has one order
//   k_wd_single    the one node of a single-triangle scene, whose second child is marked empty
//   k_wd_pack      per inner node the 64-byte record the walk reads: both children's moments and references
//   k_query_winding<VISITS>  one point per lane: the sum of the solid angles of the triangles and of the dipoles of the subtrees
//                  that are far enough away.  VISITS also writes how many dipoles the lane took and how many triangles it evaluated
//                  (the test hook's instantiation).
//
// The parent pass and the visit counter restate refit.hip's pattern (k_rf_parents, k_rf_refit) under this file's names.  The walk
// reads the packed records and the triangle records only, so it is the same code for a scene that holds fp16 or fp32 nodes: the node
// format matters to the build alone (Topo).  256-lane workgroups over a one-dimensional grid, the lane stack of query_launch.h
// (stack_entries * 64 words per wave); at most one push per visit, no box test, no ordering, no atomics: two calls give the same bits.
// Built with -ffp-contract=off: the accept rule d2 > beta2 * r2 is evaluated in fp32 as written.
#include "winding.h"
#include "query_launch.h"
#include <vector>

namespace ptd {

namespace {

// Where a node array keeps its child references: 32-bit words at `o0` / `o1` of a `stride`-word node; inner references >= 0
// (shifted left by `shift`: the byte offsets of the centre / half-extent nodes), leaf slots as ~slot.
struct WdTopo { const uint32_t* words; uint32_t stride, o0, o1; int shift; };
__device__ __forceinline__ int wd_child(const WdTopo& t, uint32_t node, uint32_t o)
{
    const int c = (int)t.words[(size_t)node * t.stride + o];
    return c >= 0 ? c >> t.shift : c;
}

__device__ __forceinline__ WindSums wd_leaf(const TriRecord& r)
{
    const float v0[3] = {r.r0.x, r.r0.y, r.r0.z}, e1[3] = {r.r0.w, r.r1.x, r.r1.y}, e2[3] = {r.r1.z, r.r1.w, r.r2.x};
    return wind_triangle(v0, e1, e2);
}

// the sums of a node as the pass stores them: four float4 per node
__device__ __forceinline__ void wd_store(float4* acc, int node, const WindSums& t)
{
    float4* p = acc + 4 * (size_t)node;
    p[0] = make_float4(t.n[0], t.n[1], t.n[2], t.area);
    p[1] = make_float4(t.s[0], t.s[1], t.s[2], 0.0f);
    p[2] = make_float4(t.lo[0], t.lo[1], t.lo[2], 0.0f);
    p[3] = make_float4(t.hi[0], t.hi[1], t.hi[2], 0.0f);
}
__device__ __forceinline__ WindSums wd_load(const float4* acc, int node)
{
    const float4* p = acc + 4 * (size_t)node;
    const float4 a = p[0], b = p[1], c = p[2], d = p[3];
    WindSums t;
    t.n[0] = a.x; t.n[1] = a.y; t.n[2] = a.z; t.area = a.w;
    t.s[0] = b.x; t.s[1] = b.y; t.s[2] = b.z;
    t.lo[0] = c.x; t.lo[1] = c.y; t.lo[2] = c.z;
    t.hi[0] = d.x; t.hi[1] = d.y; t.hi[2] = d.z;
    return t;
}

__device__ __forceinline__ WindChild wd_child_record(const WindMoment& m, int ref)
{
    return WindChild{m.px, m.py, m.pz, m.r2, m.nx, m.ny, m.nz, ref};
}

}  // namespace

__global__ void __launch_bounds__(256)
k_wd_parents(WdTopo t, uint32_t n_nodes, int* __restrict__ node_parent, int* __restrict__ leaf_parent)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const int c0 = wd_child(t, i, t.o0), c1 = wd_child(t, i, t.o1);
    if (c0 >= 0) node_parent[c0] = (int)i; else leaf_parent[~c0] = (int)i;
    if (c1 >= 0) node_parent[c1] = (int)i; else leaf_parent[~c1] = (int)i;
    if (i == 0u) node_parent[0] = -1;
}

// acc is written and read inside this launch by different CUs: no __restrict__, no const — its loads stay on the vector path behind
// the counter's acquire
__global__ void __launch_bounds__(256)
k_wd_moments(uint32_t n, const TriRecord* __restrict__ tris, WdTopo t, const int* __restrict__ node_parent, const int* __restrict__ leaf_parent,
             uint32_t* visit, float4* acc, WindMoment* __restrict__ moments)
{
    const uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x;
    if (leaf >= n) return;
    int cur = leaf_parent[leaf];
    while (cur >= 0) {
        // release this subtree's sums, acquire the sibling's: the second arrival proceeds
        const uint32_t prev = __hip_atomic_fetch_add(&visit[cur], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == 0) return;
        const int c0 = wd_child(t, (uint32_t)cur, t.o0), c1 = wd_child(t, (uint32_t)cur, t.o1);
        const WindSums s0 = c0 < 0 ? wd_leaf(tris[~c0]) : wd_load(acc, c0);
        const WindSums s1 = c1 < 0 ? wd_leaf(tris[~c1]) : wd_load(acc, c1);
        const WindSums s = wind_combine(s0, s1);
        wd_store(acc, cur, s);
        moments[cur] = wind_moment(s);
        cur = node_parent[cur];
    }
}

// single-triangle scene: the build's one node holds the triangle twice; its moment is the triangle's, its second child is empty
__global__ void k_wd_single(const TriRecord* __restrict__ tris, WindMoment* __restrict__ moments, WindNode* __restrict__ walk)
{
    const WindMoment m = wind_moment(wd_leaf(tris[0]));
    const WindMoment zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    moments[0] = m;
    WindNode nd;
    nd.c[0] = wd_child_record(zero, ~0);
    nd.c[1] = wd_child_record(zero, kWindEmpty);
    walk[0] = nd;
}

__global__ void __launch_bounds__(256)
k_wd_pack(WdTopo t, uint32_t n_nodes, const WindMoment* __restrict__ moments, WindNode* __restrict__ walk)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const WindMoment zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int c0 = wd_child(t, i, t.o0), c1 = wd_child(t, i, t.o1);
    WindNode nd;
    nd.c[0] = wd_child_record(c0 >= 0 ? moments[c0] : zero, c0);
    nd.c[1] = wd_child_record(c1 >= 0 ? moments[c1] : zero, c1);
    walk[i] = nd;
}

// The signed solid angle of the triangle {v0, v0 + e1, v0 + e2} at q (van Oosterom and Strackee): with a, b, c the vertices minus q,
// 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|).  At a vertex both arguments are 0 and atan2f answers 0.
__device__ __forceinline__ float wd_solid_angle(const f3& q, const f3& v0, const f3& e1, const f3& e2)
{
    const f3 a = v0 - q, b = (v0 + e1) - q, c = (v0 + e2) - q;
    const float la = sqrtf(dot(a, a)), lb = sqrtf(dot(b, b)), lc = sqrtf(dot(c, c));
    const float det = dot(a, cross(b, c));
    const float den = ((la * lb) * lc + dot(a, b) * lc) + (dot(b, c) * la + dot(c, a) * lb);
    return 2.0f * atan2f(det, den);
}

// A subtree seen from q: taken as its dipole iff d2 > beta2 * r2, in fp32 exactly as written (beta2 = +inf and r2 = 0 give a NaN
// product and a false compare: the exact sum).  omega: N . (p - q) / (d2 sqrt(d2)).
__device__ __forceinline__ bool wd_accept(const f3& q, float px, float py, float pz, float r2, float nx, float ny, float nz, float beta2, float& omega)
{
    const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const bool far = d2 > beta2 * r2;
    omega = ((nx * dx + ny * dy) + nz * dz) / (d2 * sqrtf(d2));
    return far;
}

template <bool VISITS>
__global__ void __launch_bounds__(256)
k_query_winding(const TriRecord* __restrict__ tris, const WindNode* __restrict__ walk, const WindMoment root, uint32_t n_tris, uint32_t stack_entries,
                float beta2, const float4* __restrict__ points, uint32_t n, float* __restrict__ out, uint2* __restrict__ visits_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      // n <= 2^31 - 1: the grid's last lane is below 2^31 + 255
    const LaneStack st = lane_stack(stack_entries);
    f3 q = mk(0.0f);
    bool ok = false;
    if (i < n) {
        const float4 p = points[i];
        q = mk(p.x, p.y, p.z);
        ok = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z);
    }
    float sum = 0.0f;
    uint2 visits = make_uint2(0u, 0u);
    int sp = 0;
    int node = (ok && n_tris != 0u) ? 0 : kSentinel;
    if (node == 0) {      // the root first
        float omega;
        if (wd_accept(q, root.px, root.py, root.pz, root.r2, root.nx, root.ny, root.nz, beta2, omega)) {
            sum = omega;
            if (VISITS) visits.x++;
            node = kSentinel;
        }
    }
    // A visit reads one record, adds the dipoles of the inner children it accepts, enters one of the others and pushes the second: at
    // most one push per level of the current path, the depth the other walks' stacks are sized for (capi.hip size_stack).
    while (node != kSentinel) {
        if (node >= 0) {
            const float4* np = (const float4*)(walk + node);
            const float4 a0 = np[0], a1 = np[1], b0 = np[2], b1 = np[3];
            const int c0 = __float_as_int(a1.w), c1 = __float_as_int(b1.w);
            bool enter0 = c0 != kWindEmpty, enter1 = c1 != kWindEmpty;
            if (c0 >= 0) {
                float omega;
                if (wd_accept(q, a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, beta2, omega)) { sum += omega; enter0 = false; if (VISITS) visits.x++; }
            }
            if (c1 >= 0) {
                float omega;
                if (wd_accept(q, b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, beta2, omega)) { sum += omega; enter1 = false; if (VISITS) visits.x++; }
            }
            if (enter0 && enter1) {
                st.push(sp, c1);
                sp++;
                node = c0;
            } else if (enter0) {
                node = c0;
            } else if (enter1) {
                node = c1;
            } else {
                if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
            }
        } else {
            const TriRecord* tp = tris + ~node;
            const float4 r0 = tp->r0, r1 = tp->r1, r2_ = tp->r2;
            sum += wd_solid_angle(q, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2_.x));
            if (VISITS) visits.y++;
            if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
    if (i >= n) return;
    out[i] = ok ? sum * (0.25f / kPIf) : __builtin_nanf("");
    if (VISITS) visits_out[i] = visits;
}

namespace {

// scratch of one build, released on every exit path
struct WdScratch {
    std::vector<void*> ptrs;
    template <typename T> hipError_t alloc(T** p, size_t bytes)
    {
        hipError_t e = hipMalloc((void**)p, bytes ? bytes : 4);
        if (e == hipSuccess) ptrs.push_back((void*)*p);
        return e;
    }
    ~WdScratch() { for (void* p : ptrs) (void)hipFree(p); }
};

WdTopo topology_of(const LbvhResult& r)
{
    // the fp32 nodes when present (d.x, d.y: words 12, 13 of 16), else either fp16 array (a.w, b.w: words 3, 7 of 8)
    if (r.nodes) return WdTopo{(const uint32_t*)r.nodes, 16u, 12u, 13u, 0};
    if (r.hnodes) return WdTopo{(const uint32_t*)r.hnodes, 8u, 3u, 7u, 0};
    return WdTopo{(const uint32_t*)r.hcnodes, 8u, 3u, 7u, 5};
}

template <typename K>
hipError_t launch_winding(K kernel, const WindingTree& w, const TriRecord* tris, uint32_t n_tris, uint32_t stack_entries, float beta2, const float4* points,
                          uint32_t n, float* out, uint2* visits, hipStream_t stream)
{
    return launch_lane_stack(kernel, stack_entries, n, stream, tris, w.walk, w.root, w.built ? n_tris : 0u, stack_entries, beta2, points, n, out, visits);
}

}  // namespace

#define WDCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string("winding: ") + #x + ": " + hipGetErrorString(e_); return false; } } while (0)

bool build_winding(const LbvhResult& r, hipStream_t stream, WindingTree& out, std::string& err)
{
    if (r.n_tris == 0 || !r.tris || (!r.nodes && !r.hnodes && !r.hcnodes)) { err = "winding: the scene holds no node array"; return false; }
    const uint32_t n = r.n_tris, n_nodes = r.n_nodes;
    WdScratch sc;      // the two arrays the scene keeps are allocated here too, and taken out of the scratch list only on success
    WindMoment* d_mom; WindNode* d_walk;
    WDCK(sc.alloc(&d_mom, (size_t)n_nodes * sizeof(WindMoment)));
    WDCK(sc.alloc(&d_walk, (size_t)n_nodes * sizeof(WindNode)));
    const uint32_t node_blocks = (n_nodes + 255u) / 256u;
    if (n == 1) {
        k_wd_single<<<1, 1, 0, stream>>>(r.tris, d_mom, d_walk);
    } else {
        const WdTopo t = topology_of(r);
        int *d_np, *d_lp; uint32_t* d_visit; float4* d_acc;
        WDCK(sc.alloc(&d_np, (size_t)n_nodes * 4));
        WDCK(sc.alloc(&d_lp, (size_t)n * 4));
        WDCK(sc.alloc(&d_visit, (size_t)n_nodes * 4));
        WDCK(sc.alloc(&d_acc, (size_t)n_nodes * 64));
        WDCK(hipMemsetAsync(d_visit, 0, (size_t)n_nodes * 4, stream));
        k_wd_parents<<<node_blocks, 256, 0, stream>>>(t, n_nodes, d_np, d_lp);
        k_wd_moments<<<(n + 255u) / 256u, 256, 0, stream>>>(n, r.tris, t, d_np, d_lp, d_visit, d_acc, d_mom);
        k_wd_pack<<<node_blocks, 256, 0, stream>>>(t, n_nodes, d_mom, d_walk);
    }
    WDCK(hipGetLastError());
    WindMoment root;
    WDCK(hipMemcpyAsync(&root, d_mom, sizeof(root), hipMemcpyDeviceToHost, stream));
    WDCK(hipStreamSynchronize(stream));
    sc.ptrs.erase(sc.ptrs.begin(), sc.ptrs.begin() + 2);      // d_mom, d_walk: the scene's from here on
    free_winding(out);
    out.moments = d_mom; out.walk = d_walk; out.root = root; out.n_nodes = n_nodes; out.built = true;
    return true;
}

void free_winding(WindingTree& w)
{
    if (w.moments) (void)hipFree(w.moments);
    if (w.walk) (void)hipFree(w.walk);
    w = WindingTree();
}

hipError_t launch_query_winding(const WindingTree& w, const TriRecord* tris, uint32_t n_tris, uint32_t stack_entries, float beta2, const float4* points,
                                uint32_t n, float* out, hipStream_t stream)
{
    return launch_winding(k_query_winding<false>, w, tris, n_tris, stack_entries, beta2, points, n, out, nullptr, stream);
}

hipError_t launch_winding_visits(const WindingTree& w, const TriRecord* tris, uint32_t n_tris, uint32_t stack_entries, float beta2, const float4* points,
                                 uint32_t n, float* out, uint2* visits, hipStream_t stream)
{
    return launch_winding(k_query_winding<true>, w, tris, n_tris, stack_entries, beta2, points, n, out, visits, stream);
}

}  // namespace ptd
