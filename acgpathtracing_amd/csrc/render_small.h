// render_small.h — launch interface of the small-scene render kernel (render_small.hip): the default kernel's loop for scenes
// whose fp16 nodes fit a CU's LDS twice, as one 1024-thread and one 256-thread workgroup per CU (20 waves, five per SIMD).
#pragma once
#include "render_megakernel.h"

namespace ptd {

constexpr int kSmallBigThreads = 1024, kSmallLittleThreads = 256;

// dynamic LDS of one workgroup of `threads` threads: lane stacks (2 bytes an entry), its copy of the nodes, LCG table, fold books
size_t small_lds_bytes(int threads, uint32_t stack_entries, uint32_t n_nodes);
// May a scene take the small-scene path on a CU with cu_lds_bytes of LDS?  Its references fit 16 bits (small_ref.h), one workgroup
// of each kind fits the CU together, and a second 256-thread workgroup beside them does not.
bool small_eligible(uint32_t n_nodes, uint32_t n_tris, uint32_t stack_entries, size_t cu_lds_bytes);
// one of the two grids; wave0: the number of its first wave among the waves of both (fold-slot scratch of RenderArgs::wave_scratch)
hipError_t launch_render_small(int threads, int math, const RenderArgs& args, uint32_t wave0, uint32_t grid_blocks, hipStream_t stream);
const char* small_kernel_name(int threads, int math);      // the instantiation as a kernel trace prints it

}  // namespace ptd
