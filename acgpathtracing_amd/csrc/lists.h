// lists.h — variable-length results in compressed-sparse-row form: pt_list_offsets, pt_query_overlap_lists, pt_query_triangles_lists
// (include/acgpt.h states the contracts; tests/lists_ref.py is the NumPy statement).  Three steps: the capped calls count, the scan
// turns counts into offsets, the fill walks again and writes every accepted index into the query's slice, ascending.  Kernels in
// lists.hip; the leaf tests and the child-box admissions are overlap_device.h's and tritri_device.h's, shared with the capped kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// ---- the cuts (tests/test_gpu_lists.py puts list lengths one below, at and one above each) ----
constexpr uint32_t kListRegister = 8u;         // a slice of at most this many words is kept as the sorted register list of the capped kernels
                                               // and written once, ascending; a longer one is stored as the walk finds it and sorted afterwards
constexpr uint32_t kListSortLds = 4096u;       // a slice of at most this many words is sorted in LDS (16 KB), a longer one in global memory
constexpr uint32_t kListScanTile = 2048u;      // counts per workgroup of the scan: 256 lanes of 8
constexpr uint32_t kListScanRuns = 256u;       // lanes of the one workgroup that scans the tile sums: more than kListScanTile * kListScanRuns
                                               // counts give every lane a run of two tile sums or more

// Words of scratch the calls need, in 8-byte words: word 0 holds the mismatch flag of the fill, words 1 .. tiles + 1 the tile sums of
// the scan and behind them the total.
inline size_t list_scratch_words(size_t n) { return 2u + (n + kListScanTile - 1u) / kListScanTile; }

// offsets[0] = 0, offsets[i + 1] = offsets[i] + counts[i] (the low 32 bits; the sums are 64-bit), and the total in scratch[1 + tiles].
// counts: n DEVICE words, offsets: n + 1, disjoint; 1 <= n <= 2^31 - 1.  Three launches: a sum per tile, an exclusive scan of the tile
// sums in one workgroup (lane t takes the t-th run of consecutive tiles, the 256 run sums are scanned in LDS), the scan of each tile
// with its prefix added.  Integer arithmetic throughout: any schedule gives the same bits.  No look-back, no waiting across workgroups.
hipError_t launch_list_offsets(const uint32_t* counts, uint32_t n, uint32_t* offsets, unsigned long long* scratch, hipStream_t stream);

// The fill and the sort behind it.  fmt: 11 = fp16 centre / half-extent nodes, 0 = fp32 nodes.  boxes / tris: the records of
// launch_query_overlap / launch_query_triangles.  offsets: n + 1 words; prims: capacity words (null with capacity == 0); found: n words
// or null; flag: one word, zero before the launch, set to 1 by every lane whose slice does not hold what it found.  A lane writes
// prims[offsets[i] .. offsets[i + 1]) only, and only if offsets[i] <= offsets[i + 1] <= capacity.
// phases: kListPhaseAll for the product; the test hook pt_debug_list_phases (tools/lists_timing.py) runs the fill or the sort alone, or
// both without the register list.
constexpr uint32_t kListPhaseFill = 1u, kListPhaseSort = 2u, kListPhaseNoRegisters = 4u, kListPhaseAll = kListPhaseFill | kListPhaseSort;
hipError_t launch_overlap_lists(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* boxes, uint32_t n, const uint32_t* offsets,
                                uint32_t* prims, uint32_t capacity, uint32_t* found, uint32_t* flag, uint32_t phases, hipStream_t stream);
hipError_t launch_triangles_lists(int fmt, const DeviceScene& sc, uint32_t stack_entries, float scene_term, const float4* tris, uint32_t n, const uint32_t* offsets,
                                  uint32_t* prims, uint32_t capacity, uint32_t* found, uint32_t* flag, uint32_t phases, hipStream_t stream);

}  // namespace ptd
