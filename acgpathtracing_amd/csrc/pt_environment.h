// pt_environment.h — the environment map as the render kernels see it (pt_set_environment, include/acgpt.h): nearest-texel lookup
// of a latitude-longitude map, its importance-sampling pdf, and a sample drawn from the two CDFs environment.hip builds.
// The kernels and pt_debug_environment call the very same functions.  FM: arithmetic level of pt_device.h (divisions only).
#pragma once
#include "pt_device.h"

namespace ptd {

// texels: {r, g, b, w} with the scale applied, row 0 = the +Y pole; w = lum(rgb) * sin(pi (row + 0.5) / H), the sampling weight.
// marginal[H]: normalised inclusive scan of the row totals; conditional[H][W]: each row's normalised inclusive scan.
// pdf_scale = W H / (2 pi^2 * total weight), 0 for a black map (nothing to sample).  w == 0: no map (a black one).
struct EnvMap {
    const float4* texels;
    const float* marginal;
    const float* conditional;
    uint32_t w, h;
    float pdf_scale;
};
constexpr float kInv2PIf = 0.159154943091895336f, kInvPIf = 0.318309886183790672f;

// u = 0.5 + atan2(d.x, -d.z) / (2 pi), v = acos(d.y) / pi; the texel that holds (u, v)
__device__ __forceinline__ uint32_t env_texel(const EnvMap& E, const f3& d)
{
    const float u = 0.5f + atan2f(d.x, -d.z) * kInv2PIf;
    const float v = acosf(clampf(d.y, -1.0f, 1.0f)) * kInvPIf;
    const int col = min(max((int)(u * (float)E.w), 0), (int)E.w - 1);
    const int row = min(max((int)(v * (float)E.h), 0), (int)E.h - 1);
    return (uint32_t)row * E.w + (uint32_t)col;
}

// radiance seen along the unit direction d
__device__ __forceinline__ f3 env_eval(const EnvMap& E, const f3& d)
{
    if (E.w == 0u) return mk(0.0f);
    const float4 t = E.texels[env_texel(E, d)];
    return mk(t.x, t.y, t.z);
}

// solid-angle pdf of env_sample for the texel's weight w and the direction's sin(theta)
template <int FM>
__device__ __forceinline__ float env_pdf_weight(float w, float sin_theta, float pdf_scale)
{
    return sin_theta > 0.0f ? m_div<FM>(w * pdf_scale, sin_theta) : 0.0f;
}

// solid-angle pdf with which env_sample draws the unit direction d
template <int FM>
__device__ __forceinline__ float env_pdf(const EnvMap& E, const f3& d)
{
    if (E.w == 0u || !(E.pdf_scale > 0.0f)) return 0.0f;
    const float w = E.texels[env_texel(E, d)].w;
    return env_pdf_weight<FM>(w, m_sqrt<FM>(fmaxf(0.0f, (1.0f - d.y) * (1.0f + d.y))), E.pdf_scale);     // (1 - y)(1 + y): exact near the poles
}

// first index k of cdf[0 .. n) with cdf[k] > x (n - 1 if none): a bin of zero width is never chosen
__device__ __forceinline__ uint32_t env_search(const float* cdf, uint32_t n, float x)
{
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] > x) hi = mid; else lo = mid + 1u;
    }
    return lo;
}
// where x lies inside bin k of cdf, in [0, 1)
template <int FM>
__device__ __forceinline__ float env_offset(const float* cdf, uint32_t k, float x)
{
    const float c0 = k ? cdf[k - 1u] : 0.0f, c1 = cdf[k];
    const float f = c1 > c0 ? m_div<FM>(x - c0, c1 - c0) : 0.5f;
    return fminf(fmaxf(f, 0.0f), 0.99999994f);
}

// (u1, u2) in [0, 1)^2 -> a direction drawn from the map's distribution: the row by u1 from the marginal CDF, the column by u2 from
// that row's CDF, a linear offset inside each bin.  Out: dir, its solid-angle pdf (pdf_uv / (2 pi^2 sin theta)) and the texel's
// radiance.  Returns false for a black map.
template <int FM>
__device__ __forceinline__ bool env_sample(const EnvMap& E, float u1, float u2, f3& dir, float& pdf, f3& Le)
{
    pdf = 0.0f; Le = mk(0.0f); dir = mk(0.0f, 1.0f, 0.0f);
    if (E.w == 0u || !(E.pdf_scale > 0.0f)) return false;
    const uint32_t row = env_search(E.marginal, E.h, u1);
    const float fv = env_offset<FM>(E.marginal, row, u1);
    const float* cdf = E.conditional + (size_t)row * E.w;
    const uint32_t col = env_search(cdf, E.w, u2);
    const float fu = env_offset<FM>(cdf, col, u2);
    const float u = ((float)col + fu) / (float)E.w, v = ((float)row + fv) / (float)E.h;
    float st, ct, sp, cp;
    sincosf(kPIf * v, &st, &ct);
    sincosf(2.0f * kPIf * (u - 0.5f), &sp, &cp);
    st = fmaxf(st, 0.0f);
    dir = mk(st * sp, ct, -(st * cp));
    const float4 t = E.texels[(size_t)row * E.w + col];
    Le = mk(t.x, t.y, t.z);
    pdf = env_pdf_weight<FM>(t.w, st, E.pdf_scale);
    return pdf > 0.0f;
}

}  // namespace ptd
