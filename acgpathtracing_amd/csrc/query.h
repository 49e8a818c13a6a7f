// query.h — device-resident ray queries: pt_query_closest / pt_query_any (include/acgpt.h states the contract; tests/query_ref.py is
// the NumPy statement of the hit record).  Kernels in query.hip; they read the render kernels' headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

// fmt: 11 = fp16 centre / half-extent nodes (sc.hcnodes), 0 = fp32 nodes (sc.nodes).  rays: n records of two float4 {o.xyz, d.x}
// {d.yz, tmin, tmax}; hits: n records of two float4 (pt_hit); occluded: n bytes.  All DEVICE, rays and hits 16-byte aligned, n >= 1.
hipError_t launch_query_closest(int fmt, const DeviceScene& sc, uint32_t stack_entries, const float4* rays, uint32_t n, float4* hits, hipStream_t stream);
hipError_t launch_query_any(int fmt, const DeviceScene& sc, uint32_t stack_entries, const float4* rays, uint32_t n, uint8_t* occluded, hipStream_t stream);

}  // namespace ptd
