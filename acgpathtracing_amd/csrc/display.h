// display.h — the display transform of pt_display_transform (include/acgpt.h states the arithmetic; tests/display_ref.py is its NumPy
// reference).  Kernels in display.hip; they include the render kernels' make_color and change nothing in it.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

namespace ptd {

constexpr uint32_t kDisplayBins = PT_DISPLAY_BINS;
constexpr uint32_t kDisplayBinBase = 856u;            // bits(2^-20) >> 20: the first bin
constexpr uint32_t kDisplayThreads = 256u;            // workgroup of the histogram and apply kernels
constexpr uint32_t kDisplayHistBlocks = 1024u;        // the histogram's grid is min(ceil(n / 256), 1024): each lane strides over the rest

// What the context keeps on the device: the live counts (bins 0..319, then the unmetered pixels), all zero between two calls (the
// meter kernel clears them after it has read them), and the record the meter kernel writes, in pt_display_info's layout.
struct DisplayState {
    uint32_t live[kDisplayBins + 1u];
    pt_display_info record;
};

// src: float4[n]; out: float4[n] or null; fb: uchar4[n] as uint32 or null (not both null).  dp.exposure == 0: histogram, meter, apply;
// else apply alone with that factor (the state is neither read nor written).  `st->live` must be zero on entry.
hipError_t launch_display(const float4* src, uint64_t n, const pt_display_params& dp, DisplayState* st, float4* out, uint32_t* fb, hipStream_t stream);

}  // namespace ptd
