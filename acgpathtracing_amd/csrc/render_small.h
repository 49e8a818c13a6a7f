// render_small.h — launch interface of the small-scene render kernel (render_small.hip): the default kernel's loop for scenes
// whose fp16 nodes fit a CU's LDS twice, as one 1024-thread and one 256-thread workgroup per CU (20 waves, five per SIMD).
#pragma once
#include "render_megakernel.h"

namespace ptd {

constexpr int kSmallBigThreads = 1024, kSmallLittleThreads = 256;

// Where a workgroup of k_render_small finds the nodes.  A launch has one of two shapes:
//   kSmallShapeHalf   both workgroups stage the fp16 nodes into their own LDS (kSmallNodesHalfLds): the fallback;
//   kSmallShapeFloat  the 1024-thread workgroup stages them as fp32 (kSmallNodesFloatLds: 64 bytes a node, the fp16 -> fp32 conversion
//                     done once per workgroup instead of once per visit), the 256-thread workgroup holds no copy and reads the fp16
//                     nodes from global memory (kSmallNodesHalfGlobal).
constexpr int kSmallNodesHalfLds = 0, kSmallNodesFloatLds = 1, kSmallNodesHalfGlobal = 2;
constexpr int kSmallShapeNone = 0, kSmallShapeHalf = 1, kSmallShapeFloat = 2;      // pt_debug_small_shape
constexpr size_t kSmallFloatNodeBytes = 64u;

// dynamic LDS of one workgroup of `threads` threads: lane stacks (2 bytes an entry), its copy of the nodes, LCG table, fold books
size_t small_lds_bytes(int threads, uint32_t stack_entries, uint32_t n_nodes);
// May a scene take the small-scene path on a CU with cu_lds_bytes of LDS?  Its references fit 16 bits (small_ref.h), one workgroup
// of each kind fits the CU together, and a second 256-thread workgroup beside them does not.
bool small_eligible(uint32_t n_nodes, uint32_t n_tris, uint32_t stack_entries, size_t cu_lds_bytes);

// The budget of kSmallShapeFloat.  big: stacks, books, LCG table and the fp32 nodes; little: stacks, books and LCG table alone.  fits:
// each counted up to a whole KB, both fit the CU together.  little_request is what the 256-thread launch asks for: `little` padded to
// just over half of what the 1024-thread workgroup leaves free (big + 2 x little_request > cu_lds_bytes), so that a second 256-thread
// workgroup never fits beside the first — the registers (20 waves a CU at 96) say the same today, but the LDS must not depend on them.
// Where `fits`, the padded request fits too: little is at least 3.5 KB, so the free space is at least 4 KB and half of it plus a KB
// of rounding stays inside it.
struct SmallFloatBudget { size_t big, little, little_request; bool fits; };
SmallFloatBudget small_float_budget(uint32_t stack_entries, uint32_t n_nodes, size_t cu_lds_bytes);

// one of the two grids; wave0: the number of its first wave among the waves of both (fold-slot scratch of RenderArgs::wave_scratch);
// nodes: kSmallNodes*, lds_bytes: the dynamic LDS to ask for (small_lds_bytes, or a SmallFloatBudget's big / little_request)
hipError_t launch_render_small(int threads, int math, int nodes, size_t lds_bytes, const RenderArgs& args, uint32_t wave0, uint32_t grid_blocks, hipStream_t stream);
const char* small_kernel_name(int threads, int math, int nodes);      // the instantiation as a kernel trace prints it
// pt_debug_small_staged: the staging function of kSmallNodesFloatLds over n_nodes fp16 nodes (device) into out (device, 64 bytes a node)
hipError_t launch_small_stage_f32(const HNode* hcnodes, uint32_t n_nodes, void* out, hipStream_t stream);

}  // namespace ptd
