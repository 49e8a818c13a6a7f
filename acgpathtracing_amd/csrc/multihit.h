// multihit.h — the first hits of a ray in order, and how many there are: pt_query_multi (include/acgpt.h states the contract;
// tests/multihit_ref.py is the reference).  Kernels in multihit.hip; they read the render kernels' headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

constexpr uint32_t kMultiMaxHits = 8u;      // PT_QUERY_MULTI_MAX

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  rays: n records of two float4 (query.h).
// hits: n * max_hits records of two float4 (pt_hit), ray-major, or null with max_hits == 0; counts: n words or null; not both null.
// All DEVICE, rays and hits 16-byte aligned, 1 <= n <= 2^31 - 1, max_hits <= kMultiMaxHits.  With counts the walk is cut at the
// ray's tmax only; without, also at the last kept hit once the list is full.
hipError_t launch_query_multi(int fmt, const DeviceScene& sc, uint32_t stack_entries, const float4* rays, uint32_t n, uint32_t max_hits, float4* hits,
                              uint32_t* counts, hipStream_t stream);

}  // namespace ptd
