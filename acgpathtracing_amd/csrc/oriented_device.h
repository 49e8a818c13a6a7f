// oriented_device.h — the query record of the oriented-box overlap queries, OBoxQuery, with BoxQuery's interface (overlap_device.h):
// PrimListWalk<OBoxQuery, CAP, ANY> (oriented.hip) and FillWalk<OBoxQuery> (lists.hip) walk it through bvh_walk.h as they walk a box or
// a triangle.  Include only from a unit built with -ffp-contract=off: the local coordinates are evaluated as written, and
// tests/oriented_ref.py mirrors them operation for operation.  The admission is outside that contract (it only prunes) and uses
// explicit fused multiply-adds.
#pragma once
#include "oriented.h"
#include "overlap_device.h"

namespace ptd {

__device__ __forceinline__ float comp(const f3& a, int k) { return k == 0 ? a.x : k == 1 ? a.y : a.z; }

// CROSS: the admission also tests the nine axes cross(world axis, box axis).  The product's record is OBoxQuery = OBoxQueryT<false>;
// the other arm exists for the measurement behind that choice alone (pt_debug_overlap_oriented_visits_cross).
template <bool CROSS>
struct OBoxQueryT {
    f3 c, h;              // centre and half extent
    f3 u, v, w;           // the box's axes in world coordinates: the columns of the 3 x 3 part
    f3 thrw, thrb, qc;    // thresholds of the world axes and of the box axes (oriented.h), c in the fp16 nodes' space
    float mc;             // CROSS: the margin of the cross axes
    __device__ __forceinline__ bool load(const float4* __restrict__ boxes, uint32_t i, uint32_t n)
    {
        c = mk(0.0f); h = mk(0.0f); u = mk(0.0f); v = mk(0.0f); w = mk(0.0f);
        if (i >= n) return false;
        const float4 r0 = boxes[4ull * i], r1 = boxes[4ull * i + 1ull], r2 = boxes[4ull * i + 2ull], r3 = boxes[4ull * i + 3ull];
        u = mk(r0.x, r1.x, r2.x);
        v = mk(r0.y, r1.y, r2.y);
        w = mk(r0.z, r1.z, r2.z);
        c = mk(r0.w, r1.w, r2.w);
        h = mk(r3.x, r3.y, r3.z);
        const bool finite = __builtin_isfinite(r0.x) && __builtin_isfinite(r0.y) && __builtin_isfinite(r0.z) && __builtin_isfinite(r0.w) &&
                            __builtin_isfinite(r1.x) && __builtin_isfinite(r1.y) && __builtin_isfinite(r1.z) && __builtin_isfinite(r1.w) &&
                            __builtin_isfinite(r2.x) && __builtin_isfinite(r2.y) && __builtin_isfinite(r2.z) && __builtin_isfinite(r2.w) &&
                            __builtin_isfinite(r3.x) && __builtin_isfinite(r3.y) && __builtin_isfinite(r3.z);
        // orthonormal to kOBoxOrthoTol: a dot product that overflows fails its compare like a NaN
        const bool ortho = fabsf(dot(u, u) - 1.0f) <= kOBoxOrthoTol && fabsf(dot(v, v) - 1.0f) <= kOBoxOrthoTol && fabsf(dot(w, w) - 1.0f) <= kOBoxOrthoTol &&
                           fabsf(dot(u, v)) <= kOBoxOrthoTol && fabsf(dot(v, w)) <= kOBoxOrthoTol && fabsf(dot(w, u)) <= kOBoxOrthoTol;
        return finite && ortho && r3.x >= 0.0f && r3.y >= 0.0f && r3.z >= 0.0f;
    }
    __device__ __forceinline__ void prepare(const DeviceScene& sc, float scene_term)
    {
        const float hsum = (h.x + h.y) + h.z;
        const float m = scene_term + (fmax3(fabsf(c.x), fabsf(c.y), fabsf(c.z)) + hsum) * kOBoxQuery;
        const float mw = m + hsum * kOBoxOrtho;
        // H_k = sum_j |A_kj| h_j: row k of the 3 x 3 part is (u_k, v_k, w_k)
        thrw = mk(((fabsf(u.x) * h.x + fabsf(v.x) * h.y) + fabsf(w.x) * h.z) + mw, ((fabsf(u.y) * h.x + fabsf(v.y) * h.y) + fabsf(w.y) * h.z) + mw,
                  ((fabsf(u.z) * h.x + fabsf(v.z) * h.y) + fabsf(w.z) * h.z) + mw);
        thrb = mk(h.x + m, h.y + m, h.z + m);
        mc = m + hsum * kOBoxOrthoCross;
        qc = mk(c.x - sc.hspace.cx, c.y - sc.hspace.cy, c.z - sc.hspace.cz);
    }
    // t: the child box's centre minus c; g: its half extent.  |a . t| <= thrb + sum_k |a_k| g_k on the three box axes.
    __device__ __forceinline__ bool box_axes_keep(float tx, float ty, float tz, float gx, float gy, float gz) const
    {
        const float pu = __builtin_fmaf(tz, u.z, __builtin_fmaf(ty, u.y, tx * u.x)), ru = __builtin_fmaf(gz, fabsf(u.z), __builtin_fmaf(gy, fabsf(u.y), gx * fabsf(u.x)));
        const float pv = __builtin_fmaf(tz, v.z, __builtin_fmaf(ty, v.y, tx * v.x)), rv = __builtin_fmaf(gz, fabsf(v.z), __builtin_fmaf(gy, fabsf(v.y), gx * fabsf(v.x)));
        const float pw = __builtin_fmaf(tz, w.z, __builtin_fmaf(ty, w.y, tx * w.x)), rw = __builtin_fmaf(gz, fabsf(w.z), __builtin_fmaf(gy, fabsf(w.y), gx * fabsf(w.x)));
        bool keep = (fabsf(pu) <= thrb.x + ru) & (fabsf(pv) <= thrb.y + rv) & (fabsf(pw) <= thrb.z + rw);
        if (CROSS) keep &= cross_axes_keep(mk(tx, ty, tz), mk(gx, gy, gz));
        return keep;
    }
    // The nine axes L = cross(e_k, a_j), world axis k and box axis j, with (k1, k2) and (j1, j2) the indices after k and j:
    //   |t . L| = |t[k2] a_j[k1] - t[k1] a_j[k2]|,  the child's radius g[k1] |a_j[k2]| + g[k2] |a_j[k1]|,
    //   the box's radius h[j1] |a_j2[k]| + h[j2] |a_j1[k]|  (a_i . L = e_k . cross(a_j, a_i), and cross(a_j, a_j1) = +-a_j2 for orthonormal axes).
    // L is no longer than 1.001, so the absolute margin is the other axes' m; axes orthonormal to 2^-10 move each |a_i . L| by at most
    // 5.4 * 2^-10 (oriented.h), taken as 2^-7.  An L near zero, a box axis along a world axis, separates nothing.
    __device__ __forceinline__ bool cross_axes_keep(const f3& t, const f3& g) const
    {
        const f3 ax[3] = {u, v, w};
        bool keep = true;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
                const float r1 = comp(ax[j], k1), r2 = comp(ax[j], k2);
                const float s = comp(t, k2) * r1 - comp(t, k1) * r2;
                const float rc = comp(g, k1) * fabsf(r2) + comp(g, k2) * fabsf(r1);
                const float rb = comp(h, j1) * fabsf(comp(ax[j2], k)) + comp(h, j2) * fabsf(comp(ax[j1], k));
                keep &= fabsf(s) <= (rc + rb) + mc;
            }
        }
        return keep;
    }
    // child_admitted_hc's decode (overlap_device.h): t = g_c * is - qc, g = g_h * is; an empty child has g_h < 0 and is admitted by no
    // compare of the world axes.
    __device__ __forceinline__ bool admit_hc(uint32_t px, uint32_t py, uint32_t pz, const HSpace& hs) const
    {
        const half2_t hx = __builtin_bit_cast(half2_t, px), hy = __builtin_bit_cast(half2_t, py), hz = __builtin_bit_cast(half2_t, pz);
        const float tx = __builtin_fmaf((float)hx.x, hs.isx, -qc.x), ty = __builtin_fmaf((float)hy.x, hs.isy, -qc.y), tz = __builtin_fmaf((float)hz.x, hs.isz, -qc.z);
        const float gx = (float)hx.y * hs.isx, gy = (float)hy.y * hs.isy, gz = (float)hz.y * hs.isz;
        float ex = fmaxf(fabsf(tx) - gx, 0.0f);
        const float ey = fmaxf(fabsf(ty) - gy, 0.0f), ez = fmaxf(fabsf(tz) - gz, 0.0f);
        ex = (float)hx.y < 0.0f ? __builtin_nanf("") : ex;
        return (ex <= thrw.x) & (ey <= thrw.y) & (ez <= thrw.z) & box_axes_keep(tx, ty, tz, gx, gy, gz);
    }
    // An empty child has lo = +inf: the world axes refuse it, whatever the box axes make of its infinities.
    __device__ __forceinline__ bool admit_f32(float lx, float ly, float lz, float hx, float hy, float hz) const
    {
        const bool world = child_admitted_f32(c, lx, ly, lz, hx, hy, hz, thrw);
        return world & box_axes_keep((0.5f * lx + 0.5f * hx) - c.x, (0.5f * ly + 0.5f * hy) - c.y, (0.5f * lz + 0.5f * hz) - c.z,
                                     0.5f * hx - 0.5f * lx, 0.5f * hy - 0.5f * ly, 0.5f * hz - 0.5f * lz);
    }
    // The statement: the triangle's stored vectors in the box's frame, then the 13 conditions of the axis-aligned test about the origin.
    // L(p) = ((m0 p.x + m4 p.y) + m8 p.z, ...) is dot(u, p), dot(v, p), dot(w, p) as pt_device.h writes dot.  The edges are rotated, not
    // formed again from rotated points.
    __device__ __forceinline__ f3 local(const f3& p) const { return mk(dot(u, p), dot(v, p), dot(w, p)); }
    __device__ __forceinline__ bool accept(const f3& v0, const f3& e1, const f3& e2) const
    {
        return tri_box_overlap(mk(0.0f), h, local(v0 - c), local(e1), local(e2));
    }
};
typedef OBoxQueryT<false> OBoxQuery;

}  // namespace ptd
