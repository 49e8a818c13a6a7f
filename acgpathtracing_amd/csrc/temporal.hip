// temporal.hip — the kernels behind pt_temporal_blend (include/acgpt.h).
//
//   k_tp_tri_bsdf   once per scene, on first use: bsdfType per triangle in the caller's index order (a scatter over the leaf slots)
//   k_tp_blend      one thread per pixel of the current view: reproject its first hit into the previous camera, take the bilinear
//                   footprint's consistent taps of the previous history, blend them with the accumulation by sample count.
//                   k_tp_blend<true> (pt_temporal_blend_motion) adds the hit point's motion between the two views' vertex positions
//                   and the variance clip of the history mean
//
// k_tp_blend reads 48 B of the current view and up to four taps x 48 B of the previous one per pixel and writes 16 B: a gather
// bound by the caches and HBM, not by arithmetic.  The motion adds 12 B of indices and six scattered 16-B vertex loads per diffuse hit,
// the clip nine 16-B accumulation taps shared with the neighbours.  No atomics, no transcendental: two calls
// give the same bits.
#include "temporal.h"
#include "image_common.h"

namespace ptd {

__global__ void __launch_bounds__(256)
k_tp_tri_bsdf(const TriRecord* __restrict__ tris, const float4* __restrict__ shade, uint32_t n, uint8_t* __restrict__ bsdf)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t prim = __float_as_uint(tris[i].r2.y);
    if (prim < n) bsdf[prim] = (uint8_t)((__float_as_uint(shade[i].w) >> kShadeBsdfShift) & 3u);
}

// Every expression below is mirrored operation for operation by tests/temporal_ref.py (fp32, same order, taps ty-major), and with
// kMotion by tests/motion_ref.py.  This file is built with -ffp-contract=off: no contraction.  kMotion = false is pt_temporal_blend:
// the motion and clip steps are compiled out, and what remains is the expressions it always had.
template <bool kMotion>
__global__ void __launch_bounds__(256)
k_tp_blend(const float4* __restrict__ accum, const float4* __restrict__ albedo_prim, const float4* __restrict__ normal_depth, uint32_t w,
           uint32_t h, pt_float3 eye, pt_float3 U, pt_float3 V, pt_float3 W, float N, const TpPrev prev, const uint8_t* __restrict__ bsdf,
           uint32_t n_tris, float cap, const TpMotion mo, float4* __restrict__ out)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint32_t p = y * w + x;
    const float4 c = accum[p], ndp = normal_depth[p];
    const uint32_t prim = __float_as_uint(albedo_prim[p].w);
    float4 o = make_float4(c.x, c.y, c.z, N);                          // the pass-through
    // Invalid inputs (include/acgpt.h): a non-finite accumulation pixel passes through, a non-finite history tap is not accepted,
    // the clip leaves non-finite neighbours out, a blend that left fp32 passes through.  Comparisons and selects only: where none
    // fires, every expression below is the one it always was.
    if (prev.hist && isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && ndp.w >= 0.0f && prim < n_tris && bsdf[prim] == (uint8_t)PT_BSDF_DIFFUSE) {
        const f3 dir = pixel_centre_dir(x, y, w, h, U, V, W);      // the ray k_dn_features traced (denoise.hip)
        f3 hit = mk(eye) + ndp.w * dir;
        bool moved_ok = true;
        if (kMotion && mo.verts) {
            // motion: the hit point's displacement from this view's positions to the previous view's, by its barycentrics on the
            // current triangle (Moller-Trumbore on the feature ray); a triangle that did not move adds nothing, not even a zero
            const uint32_t i0 = mo.idx[3u * prim], i1 = mo.idx[3u * prim + 1u], i2 = mo.idx[3u * prim + 2u];
            const float4 a0 = mo.verts[i0], a1 = mo.verts[i1], a2 = mo.verts[i2];
            const float4 q0 = mo.prev_verts[i0], q1 = mo.prev_verts[i1], q2 = mo.prev_verts[i2];
            const f3 v0 = mk(a0.x, a0.y, a0.z), v1 = mk(a1.x, a1.y, a1.z), v2 = mk(a2.x, a2.y, a2.z);
            const f3 D0 = mk(q0.x, q0.y, q0.z) - v0, D1 = mk(q1.x, q1.y, q1.z) - v1, D2 = mk(q2.x, q2.y, q2.z) - v2;
            if (D0.x != 0.0f || D0.y != 0.0f || D0.z != 0.0f || D1.x != 0.0f || D1.y != 0.0f || D1.z != 0.0f ||
                D2.x != 0.0f || D2.y != 0.0f || D2.z != 0.0f) {
                const f3 e1 = v1 - v0, e2 = v2 - v0;
                const f3 pv = cross(dir, e2);
                const float det = dot(e1, pv);
                const f3 tv = mk(eye) - v0;
                const float b1 = dot(tv, pv) / det;
                const f3 qv = cross(tv, e1);
                const float b2 = dot(dir, qv) / det;
                const f3 m = (D0 + b1 * (D1 - D0)) + b2 * (D2 - D0);
                moved_ok = isfinite(m.x) && isfinite(m.y) && isfinite(m.z);
                hit = hit + m;
            }
        }
        const f3 v = hit - mk(prev.eye);
        const f3 Up = mk(prev.U), Vp = mk(prev.V), Wp = mk(prev.W);
        const float s = dot(v, Wp) / dot(Wp, Wp);
        if (moved_ok && s > 0.0f) {
            const float du = dot(v, Up) / (s * dot(Up, Up));
            const float dv = dot(v, Vp) / (s * dot(Vp, Vp));
            const float fx = (du + 1.0f) * 0.5f * (float)prev.w - 0.5f;
            const float fy = (dv + 1.0f) * 0.5f * (float)prev.h - 0.5f;
            // a footprint with a tap inside the previous image has fx in [-1, w'), fy in [-1, h'); NaN fails here too
            if (fx >= -1.0f && fx < (float)prev.w && fy >= -1.0f && fy < (float)prev.h) {
                const float x0f = floorf(fx), y0f = floorf(fy);
                const float ax = fx - x0f, ay = fy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;
                float a = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f;
#pragma unroll
                for (int ty = 0; ty < 2; ty++) {
                    const int yq = y0 + ty;
                    if (yq < 0 || yq >= (int)prev.h) continue;
                    const float wy = ty ? ay : 1.0f - ay;
#pragma unroll
                    for (int tx = 0; tx < 2; tx++) {
                        const int xq = x0 + tx;
                        if (xq < 0 || xq >= (int)prev.w) continue;
                        const uint32_t q = (uint32_t)yq * prev.w + (uint32_t)xq;
                        if (__float_as_uint(prev.albedo_prim[q].w) != prim) continue;          // another triangle (or a miss)
                        const float4 nq = prev.normal_depth[q];
                        if (!(nq.x * ndp.x + nq.y * ndp.y + nq.z * ndp.z > 0.0f)) continue;    // the other side of the plane
                        const float wq = (tx ? ax : 1.0f - ax) * wy;
                        const float4 hq = prev.hist[q];
                        if (!(isfinite(hq.x) && isfinite(hq.y) && isfinite(hq.z) && isfinite(hq.w))) continue;   // a poisoned tap
                        a += wq;
                        hr += wq * hq.x; hg += wq * hq.y; hb += wq * hq.z;
                        hn += wq * hq.w;
                    }
                }
                const float n = hn < cap ? hn : cap;
                if (a > 0.0f && n > 0.0f) {
                    float h0 = hr / a, h1 = hg / a, h2 = hb / a;
                    if (kMotion && mo.gamma > 0.0f) {
                        // clip: the history mean into mu +- gamma sigma of the accumulation's 3 x 3 neighbourhood (taps inside the
                        // image, dy outer); neighbouring pixels read the same taps, so they come from L1/L2
                        float s1r = 0.0f, s1g = 0.0f, s1b = 0.0f, s2r = 0.0f, s2g = 0.0f, s2b = 0.0f, k = 0.0f;
#pragma unroll
                        for (int ny = -1; ny <= 1; ny++) {
                            const int yq = (int)y + ny;
                            if (yq < 0 || yq >= (int)h) continue;
#pragma unroll
                            for (int nx = -1; nx <= 1; nx++) {
                                const int xq = (int)x + nx;
                                if (xq < 0 || xq >= (int)w) continue;
                                const float4 cq = accum[(uint32_t)yq * w + (uint32_t)xq];
                                if (!(isfinite(cq.x) && isfinite(cq.y) && isfinite(cq.z))) continue;
                                s1r += cq.x; s1g += cq.y; s1b += cq.z;
                                s2r += cq.x * cq.x; s2g += cq.y * cq.y; s2b += cq.z * cq.z;
                                k += 1.0f;
                            }
                        }
                        const float g = mo.gamma;
                        const float mr = s1r / k, mg = s1g / k, mb = s1b / k;
                        const float vr = s2r / k - mr * mr, vg = s2g / k - mg * mg, vb = s2b / k - mb * mb;
                        const float sr = isfinite(vr) ? sqrtf(fmaxf(0.0f, vr)) : 0.0f, sg = isfinite(vg) ? sqrtf(fmaxf(0.0f, vg)) : 0.0f,
                                    sb = isfinite(vb) ? sqrtf(fmaxf(0.0f, vb)) : 0.0f;
                        h0 = fminf(fmaxf(h0, mr - g * sr), mr + g * sr);
                        h1 = fminf(fmaxf(h1, mg - g * sg), mg + g * sg);
                        h2 = fminf(fmaxf(h2, mb - g * sb), mb + g * sb);
                    }
                    const float den = n + N;
                    const float4 b = make_float4((n * h0 + N * c.x) / den, (n * h1 + N * c.y) / den, (n * h2 + N * c.z) / den, den);
                    if (isfinite(b.x) && isfinite(b.y) && isfinite(b.z)) o = b;
                }
            }
        }
    }
    out[p] = o;
}

hipError_t launch_tri_bsdf(const DeviceScene& sc, uint8_t* bsdf, hipStream_t stream)
{
    if (sc.n_tris == 0u) return hipSuccess;
    hipError_t e = hipMemsetAsync(bsdf, 0xFF, sc.n_tris, stream);      // a triangle no slot names stays "not diffuse"
    if (e != hipSuccess) return e;
    k_tp_tri_bsdf<<<(sc.n_tris + 255u) / 256u, 256, 0, stream>>>(sc.tris, sc.shade, sc.n_tris, bsdf);
    return hipGetLastError();
}

hipError_t launch_temporal(const float4* accum, const float4* albedo_prim, const float4* normal_depth, uint32_t w, uint32_t h, pt_float3 eye,
                           pt_float3 U, pt_float3 V, pt_float3 W, float n_samples, const TpPrev& prev, const uint8_t* bsdf, uint32_t n_tris,
                           float cap, const TpMotion* motion, float4* out, hipStream_t stream)
{
    const PixelLaunch pl = pixel_launch(w, h);
    if (!motion) k_tp_blend<false><<<pl.grid, pl.block, 0, stream>>>(accum, albedo_prim, normal_depth, w, h, eye, U, V, W, n_samples, prev, bsdf, n_tris,
                                                                     cap, TpMotion{}, out);
    else k_tp_blend<true><<<pl.grid, pl.block, 0, stream>>>(accum, albedo_prim, normal_depth, w, h, eye, U, V, W, n_samples, prev, bsdf, n_tris, cap,
                                                            *motion, out);
    return hipGetLastError();
}

}  // namespace ptd
