// query_launch.h — what every query unit repeats around its kernel: the LDS lane stack (one declaration, its size, the calling lane's
// LaneStack), the launch of 256-lane workgroups with that much dynamic LDS, the dispatch on the scene's node format, and the scene's
// scale on the host.  The render kernels keep their own (pt_device.h is not touched); LaneStack and kSentinel stay there.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <type_traits>
#include "pt_device.h"

namespace ptd {

// stack_entries * 64 words per wave, four waves per workgroup: entry sp of lane l sits at word sp * 64 + l of its wave's region, so a
// push or a pop of a whole wave is one conflict-free LDS access.
extern __shared__ uint32_t lane_stack_lds[];

inline size_t lane_stack_lds_bytes(uint32_t stack_entries) { return (size_t)(256 / 64) * stack_entries * 64u * sizeof(uint32_t); }

__device__ __forceinline__ LaneStack lane_stack(uint32_t stack_entries)
{
    LaneStack st;
    st.base = lane_stack_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    return st;
}

// `blocks` workgroups of 256 lanes with the lane stack's LDS; args are the kernel's own.
template <typename K, typename... A>
static hipError_t launch_lane_stack_blocks(K kernel, uint32_t stack_entries, uint32_t blocks, hipStream_t stream, A... args)
{
    const size_t lds = lane_stack_lds_bytes(stack_entries);
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<blocks, 256, lds, stream>>>(args...);
    return hipGetLastError();
}

// One lane per query: n <= 2^31 - 1, so (n + 255) does not wrap.
template <typename K, typename... A>
static hipError_t launch_lane_stack(K kernel, uint32_t stack_entries, uint32_t n, hipStream_t stream, A... args)
{
    return launch_lane_stack_blocks(kernel, stack_entries, (n + 255u) / 256u, stream, args...);
}

// The node format the scene holds (11: the fp16 centre / half-extent nodes, else 0: the fp32 nodes) as a template argument:
// f(std::integral_constant<int, FMT>{}), so a launcher names its kernel once, as k<decltype(F)::value>.  With a bool, which goes the
// same way: f(std::integral_constant<int, FMT>{}, std::bool_constant<B>{}).
template <typename F>
static hipError_t dispatch_format(int fmt, F f)
{
    return fmt == 11 ? f(std::integral_constant<int, 11>{}) : f(std::integral_constant<int, 0>{});
}
template <typename F>
static hipError_t dispatch_format(int fmt, bool b, F f)
{
    return dispatch_format(fmt, [&](auto fmt_c) { return b ? f(fmt_c, std::true_type{}) : f(fmt_c, std::false_type{}); });
}

// The largest finite |coordinate| of the scene box the builder (or the last refit) recorded; 0 when there is none.  The absolute terms
// of the pruning thresholds (nearest.h, overlap.h, sweep.h) scale with it.  A float converts to double exactly.
inline float scene_max_abs(const float scene_lo[3], const float scene_hi[3])
{
    float s = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float a = fabsf(scene_lo[k]), b = fabsf(scene_hi[k]);
        if (a > s && a < INFINITY) s = a;
        if (b > s && b < INFINITY) s = b;
    }
    return s;
}

// x rounded to float, upward: the absolute terms must not come out smaller than their derivation's.
inline float round_up_to_float(double x)
{
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, INFINITY);
    return f;
}

}  // namespace ptd
