// refit.hip — the kernels behind pt_update_vertices (include/acgpt.h): new vertices into a built tree of fixed topology.
//
//   k_rf_leaves   per leaf slot (grid-stride): gathers its triangle's three vertices through the device index buffer, writes the
//                 48-byte record and the shade record's normal (material word kept), folds the padded box into the scene box
//                 (wave reduction, then across the block, one ordered-uint atomic per block and component)
//   k_rf_parents  parent of every node and leaf slot, from whichever node array holds the topology
//   k_rf_refit    bottom-up, one thread per leaf slot; the second thread to reach a node writes it (arrive twice, agent-scope
//                 acq_rel counters carry the child boxes between CUs, as the build's k_refit_records)
//   k_rf_stats    per node: its own box area (area_ratio) and the fp16 planes' areas (half_area_ratio, half_box_inflation), summed
//                 per block in a fixed order; the host adds the block partials in block order
//
// The expressions for records, padded boxes and normals are the build's own (lbvh_build.hip k_prepare, record_aabb,
// k_gather_leaves); lbvh_build.hip keeps them file-local, so the few lines are restated here.  tests/test_gpu_update.py pins every
// answer and image bit against a fresh build; the node bits themselves — every box the exact union of the records below it — are
// pinned by tests/test_gpu_tree.py (test_refit).  Unions are exact, so the boxes do not depend on the order the threads arrive in.
#include "refit.h"
#include "pt_device.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace ptd {

namespace {

__device__ __forceinline__ uint32_t rf_f2ord(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float rf_ord2f(uint32_t u)
{
    const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f; memcpy(&f, &b, 4); return f;
}

// lbvh_build.hip record_aabb: the padded box of a triangle from its record
__device__ __forceinline__ void rf_record_aabb(const TriRecord& r, float pad_abs, float lo[3], float hi[3])
{
    const float pa[3] = {r.r0.x, r.r0.y, r.r0.z};
    const float pb[3] = {pa[0] + r.r0.w, pa[1] + r.r1.x, pa[2] + r.r1.y};
    const float pc[3] = {pa[0] + r.r1.z, pa[1] + r.r1.w, pa[2] + r.r2.x};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float l = fminf(pa[k], fminf(pb[k], pc[k])), h = fmaxf(pa[k], fmaxf(pb[k], pc[k]));
        const float pad = fmaxf(1e-5f * fmaxf(1.0f, fmaxf(fabsf(l), fabsf(h))), pad_abs);
        lo[k] = l - pad; hi[k] = h + pad;
    }
}

// Where a node array keeps its child references: 32-bit words at `o0` / `o1` of a `stride`-word node; inner references >= 0
// (shifted left by `shift`: the byte offsets of the centre / half-extent nodes), leaf slots as ~slot.
struct Topo { const uint32_t* words; uint32_t stride, o0, o1; int shift; };
__device__ __forceinline__ int rf_child(const Topo& t, uint32_t node, uint32_t o)
{
    const int c = (int)t.words[(size_t)node * t.stride + o];
    return c >= 0 ? c >> t.shift : c;
}

}  // namespace

__global__ void __launch_bounds__(256)
k_rf_leaves(const float4* __restrict__ verts, const uint32_t* __restrict__ idx, uint32_t n, TriRecord* __restrict__ tris,
            float4* __restrict__ shade, float pad_abs, uint32_t* __restrict__ scene_bounds /* 6 ordered uints: lo xyz, hi xyz */)
{
    // grid-stride: a few slots per thread, so that the scene box costs one atomic per BLOCK and component (k_prepare's one per wave
    // puts ~20 000 waves on the same six words at 1.31 M triangles: 1.4 ms of serialised atomics); min / max do not depend on the order
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const TriRecord old = tris[i];
        const uint32_t prim = __float_as_uint(old.r2.y);
        const float4 a = verts[idx[3 * prim]], b = verts[idx[3 * prim + 1]], c = verts[idx[3 * prim + 2]];
        TriRecord r;      // k_prepare's record; triangle index and material id stay
        r.r0 = make_float4(a.x, a.y, a.z, b.x - a.x);
        r.r1 = make_float4(b.y - a.y, b.z - a.z, c.x - a.x, c.y - a.y);
        r.r2 = make_float4(c.z - a.z, old.r2.y, old.r2.z, 0.0f);
        tris[i] = r;
        // k_gather_leaves' normal; the material word keeps its bsdf and emission tags
        const f3 n0 = normalize(cross(mk(r.r0.w, r.r1.x, r.r1.y), mk(r.r1.z, r.r1.w, r.r2.x)));
        shade[i] = make_float4(n0.x, n0.y, n0.z, shade[i].w);
        float l[3], h[3];
        rf_record_aabb(r, pad_abs, l, h);
#pragma unroll
        for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], l[k]); hi[k] = fmaxf(hi[k], h[k]); }
    }
    __shared__ float wave_box[4][6];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float l = lo[k], h = hi[k];
        for (int off = 32; off > 0; off >>= 1) {
            l = fminf(l, __shfl_xor(l, off));
            h = fmaxf(h, __shfl_xor(h, off));
        }
        if ((threadIdx.x & 63) == 0) { wave_box[threadIdx.x >> 6][k] = l; wave_box[threadIdx.x >> 6][3 + k] = h; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const float l = fminf(fminf(wave_box[0][k], wave_box[1][k]), fminf(wave_box[2][k], wave_box[3][k]));
        const float h = fmaxf(fmaxf(wave_box[0][3 + k], wave_box[1][3 + k]), fmaxf(wave_box[2][3 + k], wave_box[3][3 + k]));
        if (l <= h) {
            atomicMin(&scene_bounds[k], rf_f2ord(l));
            atomicMax(&scene_bounds[3 + k], rf_f2ord(h));
        }
    }
}

__global__ void __launch_bounds__(256)
k_rf_parents(Topo t, uint32_t n_nodes, int* __restrict__ node_parent, int* __restrict__ leaf_parent)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const int c0 = rf_child(t, i, t.o0), c1 = rf_child(t, i, t.o1);
    if (c0 >= 0) node_parent[c0] = (int)i; else leaf_parent[~c0] = (int)i;
    if (c1 >= 0) node_parent[c1] = (int)i; else leaf_parent[~c1] = (int)i;
    if (i == 0u) node_parent[0] = -1;
}

// nodes may be null (only the boxes are wanted); it may also be the array `t` reads: a node's child references are read and
// written back by the one thread that writes it
__global__ void __launch_bounds__(256)
k_rf_refit(uint32_t n, const TriRecord* __restrict__ tris, float pad_abs, Topo t, const int* __restrict__ node_parent,
           const int* __restrict__ leaf_parent, uint32_t* __restrict__ visit, float4* __restrict__ node_lo, float4* __restrict__ node_hi,
           BvhNode* nodes)
{
    const uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x;
    if (leaf >= n) return;
    int cur = leaf_parent[leaf];
    while (cur >= 0) {
        // release this subtree's box, acquire the sibling's: the second arrival proceeds
        const uint32_t prev = __hip_atomic_fetch_add(&visit[cur], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == 0) return;
        const int c0 = rf_child(t, (uint32_t)cur, t.o0), c1 = rf_child(t, (uint32_t)cur, t.o1);
        float l0[3], h0[3], l1[3], h1[3];
        if (c0 < 0) rf_record_aabb(tris[~c0], pad_abs, l0, h0);
        else { const float4 a = node_lo[c0], b = node_hi[c0]; l0[0] = a.x; l0[1] = a.y; l0[2] = a.z; h0[0] = b.x; h0[1] = b.y; h0[2] = b.z; }
        if (c1 < 0) rf_record_aabb(tris[~c1], pad_abs, l1, h1);
        else { const float4 a = node_lo[c1], b = node_hi[c1]; l1[0] = a.x; l1[1] = a.y; l1[2] = a.z; h1[0] = b.x; h1[1] = b.y; h1[2] = b.z; }
        if (nodes) {
            BvhNode nd;
            nd.a = make_float4(l0[0], l0[1], l0[2], h0[0]);
            nd.b = make_float4(h0[1], h0[2], l1[0], l1[1]);
            nd.c = make_float4(l1[2], h1[0], h1[1], h1[2]);
            nd.d = make_int4(c0, c1, 0, 0);
            nodes[cur] = nd;
        }
        node_lo[cur] = make_float4(fminf(l0[0], l1[0]), fminf(l0[1], l1[1]), fminf(l0[2], l1[2]), 0.0f);
        node_hi[cur] = make_float4(fmaxf(h0[0], h1[0]), fmaxf(h0[1], h1[1]), fmaxf(h0[2], h1[2]), 0.0f);
        cur = node_parent[cur];
    }
}

// single-triangle scene: the build's one node, whose second child is an empty box
__global__ void k_rf_single(const TriRecord* __restrict__ tris, float pad_abs, float4* __restrict__ node_lo, float4* __restrict__ node_hi,
                            BvhNode* __restrict__ nodes)
{
    float l[3], h[3];
    rf_record_aabb(tris[0], pad_abs, l, h);
    if (nodes) {
        BvhNode nd;
        nd.a = make_float4(l[0], l[1], l[2], h[0]);
        nd.b = make_float4(h[1], h[2], INFINITY, INFINITY);
        nd.c = make_float4(INFINITY, -INFINITY, -INFINITY, -INFINITY);
        nd.d = make_int4(~0, ~0, 0, 0);
        nodes[0] = nd;
    }
    node_lo[0] = make_float4(l[0], l[1], l[2], 0.0f);
    node_hi[0] = make_float4(h[0], h[1], h[2], 0.0f);
}

constexpr int kStatTerms = 5;      // own-box area, then k_half_nodes' four: child area before / after fp16 rounding, boxes, inflation

__device__ __forceinline__ float rf_area(float ex, float ey, float ez) { return ex * ey + ey * ez + ez * ex; }

// nodes may be null: then only the own-box areas (the refit_tree_area of the tree as it stands)
__global__ void __launch_bounds__(256)
k_rf_stats(const float4* __restrict__ node_lo, const float4* __restrict__ node_hi, const BvhNode* __restrict__ nodes, uint32_t n, HSpace sp,
           float* __restrict__ partial /* kStatTerms per block */)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float v[kStatTerms] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (i < n) {
        const float4 lo = node_lo[i], hi = node_hi[i];
        v[0] = rf_area(hi.x - lo.x, hi.y - lo.y, hi.z - lo.z);
        if (nodes) {      // lbvh_build.hip k_half_nodes, term for term
            const BvhNode nd = nodes[i];
            const float scale = 1.0f / sp.inv_scale;
            float l[6], h[6];
            // child 0: lo (a.x a.y a.z) hi (a.w b.x b.y); child 1: lo (b.z b.w c.x) hi (c.y c.z c.w)
            (void)pack_planes(nd.a.x, nd.a.w, sp.cx, scale, l[0], h[0]); (void)pack_planes(nd.a.y, nd.b.x, sp.cy, scale, l[1], h[1]);
            (void)pack_planes(nd.a.z, nd.b.y, sp.cz, scale, l[2], h[2]); (void)pack_planes(nd.b.z, nd.c.y, sp.cx, scale, l[3], h[3]);
            (void)pack_planes(nd.b.w, nd.c.z, sp.cy, scale, l[4], h[4]); (void)pack_planes(nd.c.x, nd.c.w, sp.cz, scale, l[5], h[5]);
            const float e0[3] = {nd.a.w - nd.a.x, nd.b.x - nd.a.y, nd.b.y - nd.a.z}, e1[3] = {nd.c.y - nd.b.z, nd.c.z - nd.b.w, nd.c.w - nd.c.x};
            const float b0 = e0[0] * e0[1] + e0[1] * e0[2] + e0[2] * e0[0], b1 = e1[0] * e1[1] + e1[1] * e1[2] + e1[2] * e1[0];
            if (e0[0] >= 0.0f) v[1] += b0;
            if (e1[0] >= 0.0f) v[1] += b1;
            const float g0[3] = {(h[0] - l[0]) * sp.inv_scale, (h[1] - l[1]) * sp.inv_scale, (h[2] - l[2]) * sp.inv_scale};
            const float g1[3] = {(h[3] - l[3]) * sp.inv_scale, (h[4] - l[4]) * sp.inv_scale, (h[5] - l[5]) * sp.inv_scale};
            const float a0 = g0[0] * g0[1] + g0[1] * g0[2] + g0[2] * g0[0], a1 = g1[0] * g1[1] + g1[1] * g1[2] + g1[2] * g1[0];
            if (e0[0] >= 0.0f) v[2] += a0;
            if (e1[0] >= 0.0f) v[2] += a1;
            if (e0[0] >= 0.0f && b0 > 0.0f) { v[3] += 1.0f; v[4] += fminf(a0 / b0, 1e4f); }
            if (e1[0] >= 0.0f && b1 > 0.0f) { v[3] += 1.0f; v[4] += fminf(a1 / b1, 1e4f); }
        }
    }
    __shared__ float wave_sum[4][kStatTerms];
#pragma unroll
    for (int k = 0; k < kStatTerms; k++) {
        float s = v[k];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kStatTerms)
        partial[(size_t)blockIdx.x * kStatTerms + threadIdx.x] =
            ((wave_sum[0][threadIdx.x] + wave_sum[1][threadIdx.x]) + wave_sum[2][threadIdx.x]) + wave_sum[3][threadIdx.x];
}

#define RFCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string("refit: ") + #x + ": " + hipGetErrorString(e_); return false; } } while (0)

namespace {

// scratch of one call, released on every exit path
struct RfScratch {
    std::vector<void*> ptrs;
    template <typename T> hipError_t alloc(T** p, size_t bytes)
    {
        hipError_t e = hipMalloc((void**)p, bytes ? bytes : 4);
        if (e == hipSuccess) ptrs.push_back((void*)*p);
        return e;
    }
    ~RfScratch() { for (void* p : ptrs) (void)hipFree(p); }
};

Topo topology_of(const LbvhResult& r)
{
    // the fp32 nodes when present (d.x, d.y: words 12, 13 of 16), else either fp16 array (a.w, b.w: words 3, 7 of 8)
    if (r.nodes) return Topo{(const uint32_t*)r.nodes, 16u, 12u, 13u, 0};
    if (r.hnodes) return Topo{(const uint32_t*)r.hnodes, 8u, 3u, 7u, 0};
    return Topo{(const uint32_t*)r.hcnodes, 8u, 3u, 7u, 5};
}

// the boxes of every node of r's tree over its current records into node_lo / node_hi (and the fp32 nodes into `nodes` if not
// null), then the stats; sums[kStatTerms] in block order
bool refit_pass(const LbvhResult& r, const Topo& t, BvhNode* nodes, const HSpace& sp, hipStream_t stream, double sums[kStatTerms],
                std::string& err)
{
    RfScratch sc;
    const uint32_t n = r.n_tris, n_nodes = r.n_nodes;
    float4 *d_lo, *d_hi; float* d_part;
    const uint32_t stat_blocks = (n_nodes + 255u) / 256u;
    RFCK(sc.alloc(&d_lo, (size_t)n_nodes * 16));
    RFCK(sc.alloc(&d_hi, (size_t)n_nodes * 16));
    RFCK(sc.alloc(&d_part, (size_t)stat_blocks * kStatTerms * 4));
    if (n == 1) {
        k_rf_single<<<1, 1, 0, stream>>>(r.tris, r.pad_abs, d_lo, d_hi, nodes);
    } else {
        int *d_np, *d_lp; uint32_t* d_visit;
        RFCK(sc.alloc(&d_np, (size_t)n_nodes * 4));
        RFCK(sc.alloc(&d_lp, (size_t)n * 4));
        RFCK(sc.alloc(&d_visit, (size_t)n_nodes * 4));
        RFCK(hipMemsetAsync(d_visit, 0, (size_t)n_nodes * 4, stream));
        k_rf_parents<<<stat_blocks, 256, 0, stream>>>(t, n_nodes, d_np, d_lp);
        k_rf_refit<<<(n + 255u) / 256u, 256, 0, stream>>>(n, r.tris, r.pad_abs, t, d_np, d_lp, d_visit, d_lo, d_hi, nodes);
    }
    k_rf_stats<<<stat_blocks, 256, 0, stream>>>(d_lo, d_hi, nodes, n_nodes, sp, d_part);
    RFCK(hipGetLastError());
    std::vector<float> h_part((size_t)stat_blocks * kStatTerms);
    RFCK(hipMemcpyAsync(h_part.data(), d_part, h_part.size() * 4, hipMemcpyDeviceToHost, stream));
    RFCK(hipStreamSynchronize(stream));
    for (int k = 0; k < kStatTerms; k++) sums[k] = 0.0;
    for (uint32_t b = 0; b < stat_blocks; b++)
        for (int k = 0; k < kStatTerms; k++) sums[k] += (double)h_part[(size_t)b * kStatTerms + k];
    // own-box area of the root (node 0), for the ratio
    float4 root_lo, root_hi;
    RFCK(hipMemcpy(&root_lo, d_lo, 16, hipMemcpyDeviceToHost));
    RFCK(hipMemcpy(&root_hi, d_hi, 16, hipMemcpyDeviceToHost));
    const double root = (double)(root_hi.x - root_lo.x) * (root_hi.y - root_lo.y) + (double)(root_hi.y - root_lo.y) * (root_hi.z - root_lo.z) +
                        (double)(root_hi.z - root_lo.z) * (root_hi.x - root_lo.x);
    sums[0] = root > 0.0 ? sums[0] / root : 1.0;
    return true;
}

template <typename T> void release(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

}  // namespace

bool refit_tree_area(const LbvhResult& r, hipStream_t stream, double& area, std::string& err)
{
    area = 1.0;
    if (r.n_tris == 0) return true;
    if (!r.tris || (!r.nodes && !r.hnodes && !r.hcnodes)) { err = "refit: the scene holds no node array"; return false; }
    double sums[kStatTerms];
    if (!refit_pass(r, topology_of(r), nullptr, r.hspace, stream, sums, err)) return false;
    area = sums[0];
    return true;
}

bool refit_lbvh(LbvhResult& r, const float* h_verts_xyzw, size_t n_verts, const uint32_t* d_idx, hipStream_t stream, double& area_out,
                std::string& err)
{
    area_out = 1.0;
    if (r.n_tris == 0) return true;
    if (!r.tris || !r.shade || (!r.nodes && !r.hnodes && !r.hcnodes)) { err = "refit: the scene holds no node array"; return false; }
    const uint32_t n = r.n_tris, n_nodes = r.n_nodes;

    // pad_abs: lbvh_build.hip build_impl, 2^-19 of the largest finite |coordinate| of every vertex (referenced or not), at least 2^-19
    float coord_max = 1.0f;
    for (size_t i = 0; i < n_verts; i++)
        for (int k = 0; k < 3; k++) { const float a = fabsf(h_verts_xyzw[4 * i + k]); if (a > coord_max && a < INFINITY) coord_max = a; }
    const float pad_abs = coord_max * (1.0f / 524288.0f);

    RfScratch sc;
    float4* d_verts; uint32_t* d_bounds;
    const uint32_t init_bounds[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    uint32_t h_bounds[6];
    RFCK(sc.alloc(&d_verts, n_verts * 16));
    RFCK(sc.alloc(&d_bounds, 24));
    RFCK(hipMemcpyAsync(d_verts, h_verts_xyzw, n_verts * 16, hipMemcpyHostToDevice, stream));
    RFCK(hipMemcpyAsync(d_bounds, init_bounds, 24, hipMemcpyHostToDevice, stream));
    k_rf_leaves<<<std::min((n + 255u) / 256u, 1024u), 256, 0, stream>>>(d_verts, d_idx, n, r.tris, r.shade, pad_abs, d_bounds);
    RFCK(hipGetLastError());
    RFCK(hipMemcpyAsync(h_bounds, d_bounds, 24, hipMemcpyDeviceToHost, stream));
    RFCK(hipStreamSynchronize(stream));
    r.pad_abs = pad_abs;
    for (int k = 0; k < 3; k++) { r.scene_lo[k] = rf_ord2f(h_bounds[k]); r.scene_hi[k] = rf_ord2f(h_bounds[3 + k]); }

    // the fp16 space of the new scene box: lbvh_build.hip build_impl, line for line
    HSpace sp;
    {
        float half_ext = 0.0f;
        float* cc = &sp.cx;
        for (int k = 0; k < 3; k++) { cc[k] = 0.5f * r.scene_lo[k] + 0.5f * r.scene_hi[k]; half_ext = fmaxf(half_ext, fmaxf(r.scene_hi[k] - cc[k], cc[k] - r.scene_lo[k])); }
        sp.inv_scale = (half_ext > 0.0f && half_ext < INFINITY ? half_ext : 1.0f) / 1023.0f;
        float* is = &sp.isx;
        for (int k = 0; k < 3; k++) {
            const float hk = fmaxf(r.scene_hi[k] - cc[k], cc[k] - r.scene_lo[k]);
            is[k] = (hk > half_ext * 0x1p-20f && hk < INFINITY && !getenv("ACGPT_HC_UNIFORM") ? hk : (half_ext > 0.0f && half_ext < INFINITY ? half_ext : 1.0f)) / 1023.0f;
        }
        sp.pad_ = 0.0f;
    }

    // the fp32 nodes: rewritten in place when the scene holds them (the topology is read from them, node by node, by the thread that
    // writes the node), else into a new array while an fp16 array still supplies the topology
    const Topo t = topology_of(r);
    BvhNode* nodes = r.nodes;
    if (!nodes) RFCK(hipMalloc((void**)&nodes, (size_t)n_nodes * sizeof(BvhNode)));
    double sums[kStatTerms];
    if (!refit_pass(r, t, nodes, sp, stream, sums, err)) {
        if (nodes != r.nodes) (void)hipFree(nodes);
        return false;
    }
    r.nodes = nodes;
    // every array derived from the old boxes goes; each comes back on first use (lbvh_build.h ensure_*)
    release(r.hnodes); release(r.hcnodes); release(r.qnodes); release(r.cnodes); release(r.top_nodes); release(r.wrecs); release(r.srecs);
    release(r.hcnodes_alt);
    r.n_top = 0; r.n_wrecs = 0; r.n_wnodes = 0; r.wide_depth = 0; r.wide_ms = 0.0f; r.n_srecs = 0; r.hcnodes_alt_bytes = 0;
    r.hspace = sp;
    r.half_area_ratio = sums[1] > 0.0 ? (float)(sums[2] / sums[1]) : 1.0f;
    r.half_box_inflation = sums[3] > 0.0 ? (float)(sums[4] / sums[3]) : 1.0f;
    {   // lbvh_build.hip make_qgrid_f: the experiment grid nodes' transform over the new scene box
        float c[3], o[3];
        for (int k = 0; k < 3; k++) {
            const float ext = r.scene_hi[k] - r.scene_lo[k];
            c[k] = (ext * 1.0001f + 1e-30f) / 65531.0f;
            o[k] = r.scene_lo[k] - 2.0f * c[k];
        }
        r.grid.ox = o[0]; r.grid.oy = o[1]; r.grid.oz = o[2];
        r.grid.cx = c[0]; r.grid.cy = c[1]; r.grid.cz = c[2];
        r.grid.icx = 1.0f / c[0]; r.grid.icy = 1.0f / c[1]; r.grid.icz = 1.0f / c[2];
    }
    area_out = sums[0];
    return true;
}

}  // namespace ptd
