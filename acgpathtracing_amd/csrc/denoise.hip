// denoise.hip — the kernels behind pt_render_features and pt_denoise (include/acgpt.h).
//
//   k_dn_features   one camera ray per pixel through the pixel centre: first-hit albedo + triangle index, unit normal + distance
//   k_dn_variance   demodulation and the 5x5 luminance variance (geometry weights only) -> scratch {c, var}
//   k_dn_atrous     one a-trous iteration (step 1, 2, 4, ...), ping-pong over the scratch; the last one remodulates into the output
//
// The filter reads 25 taps of {c, var} and {normal, depth} per pixel and iteration, 32 bytes each, plus the .w of 9 neighbours for
// the variance blur: bound by the L1 / L2, not by arithmetic.  No atomics anywhere: two calls give the same bits.
#include "denoise.h"
#include "image_common.h"
#include "traverse_hc.h"

namespace ptd {

extern __shared__ uint32_t dn_lds[];

// ---- features ---------------------------------------------------------------------------------------------------------------
// The closest-hit walk over the fp16 centre / half-extent nodes (NODE_FMT 11) is traverse_hc (traverse_hc.h): hit triangle and t equal
// pt_trace_closest's bit for bit.
template <int FMT>
__global__ void __launch_bounds__(256)
k_dn_features(const DeviceScene sc, uint32_t stack_entries, uint32_t w, uint32_t h, pt_float3 eye, pt_float3 U, pt_float3 V, pt_float3 W,
              float4* __restrict__ albedo_prim, float4* __restrict__ normal_depth)
{
    const uint32_t n = w * h;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    LaneStack st;
    st.base = dn_lds + (threadIdx.x >> 6) * (stack_entries * 64u) + (threadIdx.x & 63u);
    const bool active = i < n;
    const uint32_t x = active ? i % w : 0u, y = active ? i / w : 0u;
    const f3 dir = pixel_centre_dir(x, y, w, h, U, V, W);
    const f3 org = mk(eye);
    HitRec hit;
    if (FMT == 11) traverse_hc(sc, st, active, org, dir, 0.01f, 1e16f, hit);
    else traverse<false>(sc, st, active, org, dir, 0.01f, 1e16f, hit);
    if (!active) return;
    if (hit.slot >= 0) {
        const float4 sr = sc.shade[hit.slot];          // normalize(cross(e1, e2)) and the material id (pt_device.h)
        f3 nrm = mk(sr.x, sr.y, sr.z);
        if (dot(nrm, dir) > 0.0f) nrm = -nrm;          // towards the camera
        const float4 kd = sc.mats[__float_as_uint(sr.w) & kShadeMatMask].kd_ior;
        albedo_prim[i] = make_float4(kd.x, kd.y, kd.z, __uint_as_float(hit.prim));
        normal_depth[i] = make_float4(nrm.x, nrm.y, nrm.z, hit.t);
    } else {
        albedo_prim[i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
        normal_depth[i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    }
}

// ---- filter -----------------------------------------------------------------------------------------------------------------
// Every expression below is mirrored operation for operation by tests/denoise_ref.py (fp32, same order, taps dy-major).
__device__ __forceinline__ bool dn_hit(const float4& nd) { return nd.w >= 0.0f; }
__device__ __forceinline__ float4 dn_albedo(const float4& alb, bool hit)
{
    return hit ? make_float4(fmaxf(alb.x, kDnAlbedoFloor), fmaxf(alb.y, kDnAlbedoFloor), fmaxf(alb.z, kDnAlbedoFloor), 0.0f) : make_float4(1.0f, 1.0f, 1.0f, 0.0f);
}
// Invalid inputs (include/acgpt.h, "invalid inputs" under pt_denoise).  The rules below only add comparisons and selects: where none
// fires, every expression is the one it always was, in the same order.
// A source pixel is unusable if a demodulated channel is not finite or |l(c)| > 2^60 (NaN included): it is never a tap, and its own
// output is its accumulation rgb.  Between the passes the flag travels as var = -1 in cv.w (a usable var is >= 0 and finite).
constexpr float kDnMaxLum = 1152921504606846976.0f;      // 2^60
__device__ __forceinline__ bool dn_usable(float r, float g, float b, float l)
{
    return isfinite(r) && isfinite(g) && isfinite(b) && fabsf(l) <= kDnMaxLum;
}
// w_n and the depth term of the exponent for a tap q of p (zden = sigma_z * step * t_p, zok: it is neither zero nor not finite); false
// when exactly one of them misses, or when !zok and t_q != t_p (with t_q == t_p the depth term is then 0)
__device__ __forceinline__ bool dn_zok(float zden) { return zden != 0.0f && isfinite(zden); }
__device__ __forceinline__ bool dn_geometry(const float4& ndp, const float4& ndq, bool hp, float zden, bool zok, float& wn, float& ez)
{
    const bool hq = dn_hit(ndq);
    if (hp != hq || (hp && !zok && !(ndq.w == ndp.w))) return false;
    wn = 1.0f; ez = 0.0f;
    if (hp) {
        const float z = fabsf(ndp.w - ndq.w) / zden;
        ez = zok ? z : 0.0f;
        float c = fmaxf(ndp.x * ndq.x + ndp.y * ndq.y + ndp.z * ndq.z, 0.0f);
#pragma unroll
        for (int k = 0; k < kDnNormalSquarings; k++) c = c * c;
        wn = c;
    }
    return true;
}

__constant__ float kDnH[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
__constant__ float kDnG[3] = {0.25f, 0.5f, 0.25f};

// demodulation + variance (step 1, 5x5, geometry weights), about l_p: M1, M2 = weighted means of (l_q - l_p) and its square
__global__ void __launch_bounds__(256)
k_dn_variance(const float4* __restrict__ accum, const float4* __restrict__ albedo, const float4* __restrict__ nd, uint32_t w, uint32_t h,
              float4* __restrict__ cv)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint32_t p = y * w + x;
    const float4 ndp = nd[p];
    const bool hp = dn_hit(ndp);
    const float4 ap = dn_albedo(albedo[p], hp), cp4 = accum[p];
    const float cr = cp4.x / ap.x, cg = cp4.y / ap.y, cb = cp4.z / ap.z;
    const float lp = image_lum(cr, cg, cb);
    if (!dn_usable(cr, cg, cb, lp)) { cv[p] = make_float4(cr, cg, cb, -1.0f); return; }
    const float zden = kDnSigmaZ * 1.0f * ndp.w;
    const bool zok = dn_zok(zden);
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int yq = (int)y + dy;
        if (yq < 0 || yq >= (int)h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int xq = (int)x + dx;
            if (xq < 0 || xq >= (int)w) continue;
            const uint32_t q = (uint32_t)yq * w + (uint32_t)xq;
            const float4 ndq = nd[q];
            const float4 aq = dn_albedo(albedo[q], hp), c4 = accum[q];
            const float qr = c4.x / aq.x, qg = c4.y / aq.y, qb = c4.z / aq.z;
            const float lq = image_lum(qr, qg, qb);
            float wn, ez;
            if (!dn_geometry(ndp, ndq, hp, zden, zok, wn, ez) || !dn_usable(qr, qg, qb, lq)) continue;      // one branch per tap
            const float dl = lq - lp;
            const float wq = wn * expf(-ez);
            sw += wq; s1 += wq * dl; s2 += wq * (dl * dl);
        }
    }
    const float m1 = s1 / sw, m2 = s2 / sw;        // sw > 0: the centre tap has weight ~1, unless the normal is zero, NaN or short
    const float var = fmaxf(m2 - m1 * m1, 0.0f);
    cv[p] = make_float4(cr, cg, cb, sw > 0.0f && isfinite(var) ? var : 0.0f);
}

// one iteration at `step`; LAST: remodulate with max(albedo_p, 0.01) and write {rgb, 1}, else {c', var'}; an unusable pixel
// (cv.w < 0) stays as it is, and LAST writes its accumulation rgb
template <bool LAST>
__global__ void __launch_bounds__(256)
k_dn_atrous(const float4* __restrict__ cv, const float4* __restrict__ nd, const float4* __restrict__ albedo, const float4* __restrict__ accum,
            uint32_t w, uint32_t h, int step, float4* __restrict__ out)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint32_t p = y * w + x;
    const float4 ndp = nd[p], cvp = cv[p];
    const bool hp = dn_hit(ndp);
    if (cvp.w < 0.0f) {
        if (LAST) { const float4 c = accum[p]; out[p] = make_float4(c.x, c.y, c.z, 1.0f); }
        else out[p] = cvp;
        return;
    }
    // g(var)_p: 3x3 {1/4, 1/2, 1/4}^2 at distance 1, renormalised at the borders
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int yq = (int)y + dy;
        if (yq < 0 || yq >= (int)h) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int xq = (int)x + dx;
            if (xq < 0 || xq >= (int)w) continue;
            const float k = kDnG[dx + 1] * kDnG[dy + 1];
            const float vq = cv[(uint32_t)yq * w + (uint32_t)xq].w;
            const bool use = !(vq < 0.0f);              // selects, not a branch: an unusable neighbour adds an exact zero
            gs += use ? k * vq : 0.0f;
            gw += use ? k : 0.0f;
        }
    }
    const float lden = kDnSigmaL * sqrtf(gs / gw) + 1e-6f;
    const float lp = image_lum(cvp.x, cvp.y, cvp.z);
    const float zden = kDnSigmaZ * (float)step * ndp.w;
    const bool zok = dn_zok(zden);
    float sk = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int yq = (int)y + dy * step;
        if (yq < 0 || yq >= (int)h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int xq = (int)x + dx * step;
            if (xq < 0 || xq >= (int)w) continue;
            const uint32_t q = (uint32_t)yq * w + (uint32_t)xq;
            const float4 ndq = nd[q];
            const float4 c = cv[q];
            float wn, ez;
            if (!dn_geometry(ndp, ndq, hp, zden, zok, wn, ez) || c.w < 0.0f) continue;       // one branch per tap
            const float el = fabsf(lp - image_lum(c.x, c.y, c.z)) / lden;
            const float k = kDnH[dx + 2] * kDnH[dy + 2] * wn * expf(-(ez + el));
            sk += k;
            sr += k * c.x; sg += k * c.y; sb += k * c.z;
            sv += (k * k) * c.w;
        }
    }
    float r = sr / sk, g = sg / sk, b = sb / sk;            // sk > 0: the centre tap's k is 9/64 * n_p.n_p^128
    float var = sv / (sk * sk);
    // no weight at all (a zero, NaN or short normal) or a sum that left fp32: the pixel keeps c_p and var_p for this pass
    if (!(sk > 0.0f && isfinite(r) && isfinite(g) && isfinite(b) && isfinite(var))) { r = cvp.x; g = cvp.y; b = cvp.z; var = cvp.w; }
    if (LAST) {
        const float4 ap = dn_albedo(albedo[p], hp);
        out[p] = make_float4(r * ap.x, g * ap.y, b * ap.z, 1.0f);
    } else {
        out[p] = make_float4(r, g, b, var);
    }
}

hipError_t launch_features(int fmt, const DeviceScene& sc, uint32_t stack_entries, uint32_t w, uint32_t h, pt_float3 eye, pt_float3 U, pt_float3 V,
                           pt_float3 W, float4* albedo_prim, float4* normal_depth, hipStream_t stream)
{
    const uint32_t n = w * h;
    const size_t lds = (size_t)(256 / 64) * stack_entries * 64u * sizeof(uint32_t);
    const void* fn = fmt == 11 ? (const void*)k_dn_features<11> : (const void*)k_dn_features<0>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (fmt == 11) k_dn_features<11><<<(n + 255) / 256, 256, lds, stream>>>(sc, stack_entries, w, h, eye, U, V, W, albedo_prim, normal_depth);
    else k_dn_features<0><<<(n + 255) / 256, 256, lds, stream>>>(sc, stack_entries, w, h, eye, U, V, W, albedo_prim, normal_depth);
    return hipGetLastError();
}

hipError_t launch_denoise(const float4* accum, const float4* albedo_prim, const float4* normal_depth, uint32_t w, uint32_t h, uint32_t iterations,
                          float4* scratch0, float4* scratch1, float4* out, hipStream_t stream)
{
    const PixelLaunch pl = pixel_launch(w, h);
    k_dn_variance<<<pl.grid, pl.block, 0, stream>>>(accum, albedo_prim, normal_depth, w, h, scratch0);
    hipError_t e = hipGetLastError();
    float4* src = scratch0;
    float4* dst = scratch1;
    for (uint32_t i = 0; i < iterations && e == hipSuccess; i++) {
        const int step = 1 << i;
        if (i + 1 == iterations) k_dn_atrous<true><<<pl.grid, pl.block, 0, stream>>>(src, normal_depth, albedo_prim, accum, w, h, step, out);
        else k_dn_atrous<false><<<pl.grid, pl.block, 0, stream>>>(src, normal_depth, albedo_prim, accum, w, h, step, dst);
        e = hipGetLastError();
        float4* t = src; src = dst; dst = t;
    }
    return e;
}

}  // namespace ptd
