// small_slab.h — the box test of k_render_small (render_small.hip): one formula on two operand forms.
//
// slab_hc (pt_device.h) computes per axis c_t = fma(c, mul, add), e = fma(h, |mul|, 0), near = c_t - e, far = c_t + e: four instructions,
// the shape to have while both fma are half-rate v_fma_mix_f32 and the add / sub ride beside them.  On operands staged as fp32 every one
// of the four is full rate, and the product e is work the result does not need:
//     c_t  = fma( c, mul,   add)
//     near = fma(-h, |mul|, c_t)
//     far  = fma( h, |mul|, c_t)
// three instructions per axis and child (the negation and the absolute value are source modifiers), eighteen v_fma_f32 a visit where there
// were twelve and twelve add / sub.  Each plane has one rounding fewer: e is not rounded before it meets c_t.  So near and far are NOT the
// bits of slab_hc's; they are the correctly rounded c_t -/+ h * |mul|, where slab_hc's are that value of a rounded product.  Both lie within
// one ulp of the same real number, and the pads that make the test conservative (pack_centre_half's guard of 3.9e-6 relative, kFarWiden)
// were sized for the larger of the two errors.  pt_selftest ops 42 / 43 hold the formula to the exact box in its own right.
//
// The negation sits on h, not on the multiplier: fma(h, -|mul|, c_t) makes the compiler keep -|mul| in three more registers over the
// whole loop, which is the difference between 96 VGPRs and a spill in the 1024-thread fp32 instantiations.
//
// slab_hcf_f32 takes the staged float records of small_stage_f32, slab_hcf the packed fp16 words of an HNode half.  fp16 -> fp32 is
// exact, so for one node and one ray the two return the same bits: the grids of k_render_small walk with identical box decisions
// whichever form their nodes are in.
#pragma once
#include "pt_device.h"

namespace ptd {

// c = {cx, cy, cz, child}, h = {hx, hy, hz, 0} as floats in their bit patterns
__device__ __forceinline__ void slab_hcf_f32(const uint4& c, const uint4& h, const f3& mul, const f3& add, float rtmin, float& tn, float& tf)
{
    const float cx = __builtin_fmaf(__uint_as_float(c.x), mul.x, add.x), cy = __builtin_fmaf(__uint_as_float(c.y), mul.y, add.y), cz = __builtin_fmaf(__uint_as_float(c.z), mul.z, add.z);
    const float hx = __uint_as_float(h.x), hy = __uint_as_float(h.y), hz = __uint_as_float(h.z);
    const float ax = fabsf(mul.x), ay = fabsf(mul.y), az = fabsf(mul.z);
    tn = fmaxf(fmaxf(__builtin_fmaf(-hx, ax, cx), __builtin_fmaf(-hy, ay, cy)), fmaxf(__builtin_fmaf(-hz, az, cz), rtmin));
    tf = fminf(fminf(__builtin_fmaf(hx, ax, cx), __builtin_fmaf(hy, ay, cy)), __builtin_fmaf(hz, az, cz)) * kFarWiden;
}

// px, py, pz = {centre | half extent << 16} as pack_centre_half packs them: every fma a v_fma_mix_f32
__device__ __forceinline__ void slab_hcf(uint32_t px, uint32_t py, uint32_t pz, const f3& mul, const f3& add, float rtmin, float& tn, float& tf)
{
    const half2_t qx = __builtin_bit_cast(half2_t, px), qy = __builtin_bit_cast(half2_t, py), qz = __builtin_bit_cast(half2_t, pz);
    const float cx = __builtin_fmaf((float)qx.x, mul.x, add.x), cy = __builtin_fmaf((float)qy.x, mul.y, add.y), cz = __builtin_fmaf((float)qz.x, mul.z, add.z);
    const float hx = (float)qx.y, hy = (float)qy.y, hz = (float)qz.y;
    const float ax = fabsf(mul.x), ay = fabsf(mul.y), az = fabsf(mul.z);
    tn = fmaxf(fmaxf(__builtin_fmaf(-hx, ax, cx), __builtin_fmaf(-hy, ay, cy)), fmaxf(__builtin_fmaf(-hz, az, cz), rtmin));
    tf = fminf(fminf(__builtin_fmaf(hx, ax, cx), __builtin_fmaf(hy, ay, cy)), __builtin_fmaf(hz, az, cz)) * kFarWiden;
}

}  // namespace ptd
