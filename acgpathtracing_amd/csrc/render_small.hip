// render_small.hip — the persistent path-trace kernel specialised for small scenes (Cornell class): BVH nodes from LDS at five
// waves per SIMD.
//
// The default kernel (k_render_pw variant 7, render_megakernel.hip) keeps both per-CU limits near full on such scenes: vector issue
// 0.82 busy, texture-address path 0.77.  Reading the 40 KB of fp16 nodes from LDS takes the node gathers off the texture path
// (profiles/r04_ab_lds_nodes.txt: 5.7 % at four waves per SIMD), but a copy of the tree is per workgroup, and five waves per SIMD
// are 20 waves a CU — more than one workgroup.  So a CU runs TWO workgroups of this kernel, from two launches that share one
// RenderArgs and pull from the same queue: 1024 threads (four waves per SIMD) and 256 threads (the fifth), each with its own copy
// of the nodes.  Neither waits for the other; any subset of resident workgroups drains the queue.
//
// What makes both fit: 16-bit stack entries (small_ref.h) halve the lane stacks.
//
// Stack layout: entry-major, lane-minor, two lanes to a dword — entry e of lane l of a wave at byte e * 128 + 2 * l of the wave's
// region.  A wave-wide ds_read_i16 touches 32 consecutive dwords, 16 per 32-lane group, every dword by the two lanes that share
// it: one bank each, and the two lanes of a pair ask for the same dword, which the LDS serves as one access.  A ds_write_b16 of
// the pair writes the two halves of one dword; even if the array took that as two accesses to one bank, a 2-way conflict on a
// 4-byte-or-narrower store is hidden behind the cycles the store spends moving its address and data registers (4 against 2 in
// the array).  The alternative stack[entry][lane / 2] with sub-dword writes is this very layout; two half-wave planes would buy
// nothing on top.
//
// LDS budget of a CU (small_eligible): with S = stack_entries and N = nodes,
//   1024-thread workgroup: 16 x S x 128  +  N x 32  +  256  +  16 x 320
//    256-thread workgroup:  4 x S x 128  +  N x 32  +  256  +   4 x 320
//   together: 2 x N x 32  +  20 waves x 64 lanes x S x 2 B  +  20 books of 320 B  +  2 LCG tables of 256 B.
// Cornell boxes (N = 1263, S = 24): 94 944 + 54 240 = 149 184 B of the CU's 163 840: one of each fits, and a second 256-thread
// workgroup (54 240 B more) does not, so a CU never holds two small workgroups in the place of the large one.
//
// That is the fp16 shape (kSmallShapeHalf), which decides whether a scene takes the path at all.  Inside the path a launch takes the
// fp32 shape (kSmallShapeFloat, render_small.h) where its budget fits (small_float_budget):
//   1024-thread workgroup: 16 x (S x 128 + 320)  +  N x 64  +  256      nodes as fp32: the visit's fp16 -> fp32 conversions done once, at staging
//    256-thread workgroup:  4 x (S x 128 + 320)  +  256                 no copy: the fp16 nodes from global memory, as variant 7 reads them
// Cornell boxes: 135 360 + 13 824 = 149 184 B, the same sum.  The 256-thread launch asks for more than it lays out — just over half
// of what the large workgroup leaves free — so that a second one never fits beside the first.
#include "render_common.h"
#include "render_small.h"
#include "small_ref.h"
#include "small_slab.h"

namespace ptd {

struct SmallArgsBox { RenderArgs a[1]; uint32_t wave0; };      // RenderArgs at the offsets of RenderArgsBox, the grid's first wave number behind it

// One stack per lane, 16-bit entries in the local form of small_ref.h: a pop sign-extends.
struct SmallStack {
    uint16_t* base;   // &lds16[wave_region + lane]
    __device__ __forceinline__ void push(int sp, int v) const { base[sp * 64] = (uint16_t)v; }
    __device__ __forceinline__ int pop(int sp) const { return (int)(int16_t)base[sp * 64]; }
};

// Both 16-byte halves of a staged node, as two ds_read_b128 (8 LDS-array cycles a wave).  Read as two uint4 through a generic
// pointer, the compiler takes {x, y, z} of each half with a ds_read_b96 and the two child words with a ds_read2_b32: 20 cycles.
typedef uint32_t small_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void small_node(const char* p, uint4& a, uint4& b)
{
    const __attribute__((address_space(3))) small_v4u* q = (const __attribute__((address_space(3))) small_v4u*)p;
    const small_v4u va = q[0], vb = q[1];
    a = make_uint4(va.x, va.y, va.z, va.w); b = make_uint4(vb.x, vb.y, vb.z, vb.w);
}


// ---- kSmallNodesFloatLds: the nodes as fp32 ----
// Each 16-byte half of an HNode {cx | hx << 16, cy | hy << 16, cz | hz << 16, child} becomes two 16-byte records,
// {(float)cx, (float)cy, (float)cz, child in the local form of small_ref.h} and {(float)hx, (float)hy, (float)hz, 0}: a node is 64
// bytes, at node << 2 from the same 16-bit reference.  The conversion is exact, so a v_fma_f32 on the staged float gives the bits
// of the v_fma_mix_f32 on the half (slab_hcf_f32 / slab_hcf, small_slab.h).  The one staging code of the kernel and of pt_debug_small_staged.
__device__ __forceinline__ void small_stage_f32(uint4* dst, const uint4* src, uint32_t n_halves, uint32_t first, uint32_t stride)
{
    for (uint32_t i = first; i < n_halves; i += stride) {
        const uint4 v = src[i];
        const half2_t hx = __builtin_bit_cast(half2_t, v.x), hy = __builtin_bit_cast(half2_t, v.y), hz = __builtin_bit_cast(half2_t, v.z);
        dst[2u * i] = make_uint4(__float_as_uint((float)hx.x), __float_as_uint((float)hy.x), __float_as_uint((float)hz.x), (uint32_t)small_ref_local((int)v.w));
        dst[2u * i + 1u] = make_uint4(__float_as_uint((float)hx.y), __float_as_uint((float)hy.y), __float_as_uint((float)hz.y), 0u);
    }
}
// the four records of a staged node as four ds_read_b128 (small_node's reason for the LDS-typed pointer holds here too)
__device__ __forceinline__ void small_node_f32(const char* p, uint4& ca, uint4& ha, uint4& cb, uint4& hb)
{
    const __attribute__((address_space(3))) small_v4u* q = (const __attribute__((address_space(3))) small_v4u*)p;
    const small_v4u v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
    ca = make_uint4(v0.x, v0.y, v0.z, v0.w); ha = make_uint4(v1.x, v1.y, v1.z, v1.w);
    cb = make_uint4(v2.x, v2.y, v2.z, v2.w); hb = make_uint4(v3.x, v3.y, v3.z, v3.w);
}
// the box test on these records is slab_hcf_f32 (small_slab.h)

#include "render_small.inc"

__global__ void __launch_bounds__(256) k_small_stage_f32(const uint4* src, uint32_t n_halves, uint4* dst)
{
    small_stage_f32(dst, src, n_halves, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

constexpr size_t kSmallFixedPerWave = (size_t)kBookDwords * 4u, kSmallFixedPerGroup = 256u;
constexpr size_t kSmallWaves = (size_t)(kSmallBigThreads + kSmallLittleThreads) / 64u;
// the parts of the budget that are constants: 20 books and two LCG tables are a twentieth of a CU's LDS, whatever the scene
static_assert(kSmallWaves == 20u, "1024 + 256 threads are five waves per SIMD");
static_assert(kSmallWaves * kSmallFixedPerWave + 2u * kSmallFixedPerGroup <= 8u * 1024u, "books and LCG tables of both workgroups");
// the largest tree the 16-bit references reach cannot be staged twice beside any stack: the LDS budget, not the encoding, is the limit
static_assert(2u * (size_t)kSmallMaxNodes * sizeof(HNode) >= 128u * 1024u, "2048 nodes are 64 KB a copy");

size_t small_lds_bytes(int threads, uint32_t stack_entries, uint32_t n_nodes)
{
    const size_t waves = (size_t)threads / 64u;
    return waves * ((size_t)stack_entries * 64u * sizeof(uint16_t) + kSmallFixedPerWave) + (size_t)n_nodes * sizeof(HNode) + kSmallFixedPerGroup;
}

bool small_eligible(uint32_t n_nodes, uint32_t n_tris, uint32_t stack_entries, size_t cu_lds_bytes)
{
    if (n_nodes < 1u || n_nodes > kSmallMaxNodes || n_tris < 2u || n_tris > kSmallMaxTris) return false;      // references in 16 bits
    if (stack_entries < 4u || (stack_entries & 3u) != 0u) return false;                                        // the nodes behind the stacks stay 16-byte aligned
    // a workgroup's LDS is handed out in granules; counting each workgroup up to the next KB errs on the side of "does not fit"
    const auto kb = [](size_t b) { return (b + 1023u) & ~(size_t)1023u; };
    const size_t big = small_lds_bytes(kSmallBigThreads, stack_entries, n_nodes), little = small_lds_bytes(kSmallLittleThreads, stack_entries, n_nodes);
    if (kb(big) + kb(little) > cu_lds_bytes) return false;           // one of each must fit ...
    return big + 2u * little > cu_lds_bytes;                         // ... and a second 256-thread workgroup beside them must not
}

SmallFloatBudget small_float_budget(uint32_t stack_entries, uint32_t n_nodes, size_t cu_lds_bytes)
{
    const auto kb = [](size_t b) { return (b + 1023u) & ~(size_t)1023u; };
    const auto bare = [&](int threads) { return (size_t)threads / 64u * ((size_t)stack_entries * 64u * sizeof(uint16_t) + kSmallFixedPerWave) + kSmallFixedPerGroup; };
    SmallFloatBudget b;
    b.big = bare(kSmallBigThreads) + (size_t)n_nodes * kSmallFloatNodeBytes;
    b.little = bare(kSmallLittleThreads);
    b.fits = kb(b.big) + kb(b.little) <= cu_lds_bytes;
    // just over half of what the 1024-thread workgroup leaves free, in 16-byte steps: two of them are more than is left
    const size_t half_free = b.big < cu_lds_bytes ? (((cu_lds_bytes - b.big) / 2u + 16u) & ~(size_t)15u) : 0u;
    b.little_request = b.little > half_free ? b.little : half_free;
    return b;
}

typedef void (*SmallKernel)(const SmallArgsBox);
static SmallKernel small_kernel(int threads, int math, int nodes)
{
    if (threads == kSmallBigThreads) {
        if (nodes == kSmallNodesFloatLds) return math != 0 ? k_render_small<kSmallBigThreads, 1, kSmallNodesFloatLds> : k_render_small<kSmallBigThreads, 0, kSmallNodesFloatLds>;
        if (nodes == kSmallNodesHalfLds) return math != 0 ? k_render_small<kSmallBigThreads, 1, kSmallNodesHalfLds> : k_render_small<kSmallBigThreads, 0, kSmallNodesHalfLds>;
        return nullptr;
    }
    if (nodes == kSmallNodesHalfGlobal) return math != 0 ? k_render_small<kSmallLittleThreads, 1, kSmallNodesHalfGlobal> : k_render_small<kSmallLittleThreads, 0, kSmallNodesHalfGlobal>;
    if (nodes == kSmallNodesHalfLds) return math != 0 ? k_render_small<kSmallLittleThreads, 1, kSmallNodesHalfLds> : k_render_small<kSmallLittleThreads, 0, kSmallNodesHalfLds>;
    return nullptr;
}
const char* small_kernel_name(int threads, int math, int nodes)
{
    static const char* const names[2][2][3] = {
        {{"k_render_small<1024, 0, 0>", "k_render_small<1024, 0, 1>", ""}, {"k_render_small<1024, 1, 0>", "k_render_small<1024, 1, 1>", ""}},
        {{"k_render_small<256, 0, 0>", "", "k_render_small<256, 0, 2>"}, {"k_render_small<256, 1, 0>", "", "k_render_small<256, 1, 2>"}}};
    if (nodes < 0 || nodes > 2) return "";
    return names[threads == kSmallBigThreads ? 0 : 1][math != 0 ? 1 : 0][nodes];
}

hipError_t launch_render_small(int threads, int math, int nodes, size_t lds, const RenderArgs& args, uint32_t wave0, uint32_t grid_blocks, hipStream_t stream)
{
    if ((threads != kSmallBigThreads && threads != kSmallLittleThreads) || grid_blocks == 0u) return hipErrorInvalidValue;
    if (args.n_lds_nodes < 1u || args.n_lds_nodes > kSmallMaxNodes || args.scene.n_tris > kSmallMaxTris || args.scene.hcnodes == nullptr) return hipErrorInvalidValue;
    const SmallKernel k = small_kernel(threads, math, nodes);
    if (k == nullptr) return hipErrorInvalidValue;
    // never less LDS than the kernel lays out: stacks, books and LCG table, and the copy of the nodes in the form it stages
    const size_t node_bytes = nodes == kSmallNodesHalfLds ? sizeof(HNode) : nodes == kSmallNodesFloatLds ? kSmallFloatNodeBytes : 0u;
    if (lds < small_lds_bytes(threads, args.stack_entries, 0u) + (size_t)args.n_lds_nodes * node_bytes) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    SmallArgsBox box;
    box.a[0] = args;
    box.wave0 = wave0;
    hipLaunchKernelGGL(k, dim3(grid_blocks), dim3(threads), lds, stream, box);
    return hipGetLastError();
}

hipError_t launch_small_stage_f32(const HNode* hcnodes, uint32_t n_nodes, void* out, hipStream_t stream)
{
    if (hcnodes == nullptr || out == nullptr || n_nodes < 1u || n_nodes > kSmallMaxNodes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_small_stage_f32, dim3((n_nodes * 2u + 255u) / 256u), dim3(256), 0, stream, (const uint4*)hcnodes, n_nodes * 2u, (uint4*)out);
    return hipGetLastError();
}

}  // namespace ptd
