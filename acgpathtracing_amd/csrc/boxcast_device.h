// boxcast_device.h — the leaf test and the record of the swept oriented-box casts (include/acgpt.h pt_query_box_cast states them to
// the last operation; tests/boxcast_ref.py is the NumPy twin).  Include only from a unit built with -ffp-contract=off: every operation
// is evaluated as written, IEEE division and square root.
//
// In the box's own frame (OBoxQuery::local, oriented_device.h) the box is the cube |q_j| <= h_j about the origin and the triangle
// {P0, P0 + E1, P0 + E2} translates by nD t, nD = -L(d).  On each of tri_box_overlap's 13 axes the triangle's projection [lo, hi]
// moves with the speed s = the projection of nD and meets [-r, r] between (-r - hi) / s and (r - lo) / s; the time of impact is the
// largest entry, valid iff it is no later than the smallest exit.
#pragma once
#include "oriented_device.h"

namespace ptd {

// What the 13 axes leave behind: te = the largest entry so far (ties keep the lower axis), tx = the smallest exit, and of the axis of
// te its number, its speed and the axis itself in the box's frame (the last two feed the record alone: the walk's copies are dead code).
struct OBoxClip { float te, tx, sw; int ax; f3 a; };

// One axis: entry and exit, folded into c.  The two divisions run on every lane, by 1 where s == 0; the selects behind them keep a wave on one instruction
// stream.  s == 0: the axis rules the pair out (entry +inf, exit -inf) iff lo > r or hi < -r, and constrains nothing otherwise.
__device__ __forceinline__ void obox_axis(int k, float lo, float hi, float r, float s, const f3& axis, OBoxClip& c)
{
    const bool still = s == 0.0f;
    const float sd = still ? 1.0f : s;
    const float a = (-r - hi) / sd, b = (r - lo) / sd;
    const bool swap = b < a;
    float en = swap ? b : a, ex = swap ? a : b;
    const bool out = lo > r || hi < -r;
    en = still ? (out ? INFINITY : -INFINITY) : en;
    ex = still ? (out ? -INFINITY : INFINITY) : ex;
    if (en > c.te) { c.te = en; c.ax = k; c.sw = s; c.a = axis; }
    if (ex < c.tx) c.tx = ex;
}

// One of the nine edge axes, cross(unit i, f) with (j, k) the two axes after i: edge_axis_keeps' projections and radius
// (overlap_device.h), the speed by the same expression.  axis: that cross product, a[i] = 0, a[j] = -f[k], a[k] = f[j].
__device__ __forceinline__ void obox_edge_axis(int n, float p0j, float p0k, float p1j, float p1k, float p2j, float p2k, float vj, float vk, float fj, float fk, float hj,
                                               float hk, const f3& axis, OBoxClip& c)
{
    const float s0 = p0k * fj - p0j * fk, s1 = p1k * fj - p1j * fk, s2 = p2k * fj - p2j * fk;
    const float r = hj * fabsf(fk) + hk * fabsf(fj);
    const float s = vk * fj - vj * fk;
    obox_axis(n, fmin3(s0, s1, s2), fmax3(s0, s1, s2), r, s, axis, c);
}
__device__ __forceinline__ void obox_edge(int n, const f3& p0, const f3& p1, const f3& p2, const f3& v, const f3& f, const f3& h, OBoxClip& c)
{
    obox_edge_axis(n, p0.y, p0.z, p1.y, p1.z, p2.y, p2.z, v.y, v.z, f.y, f.z, h.y, h.z, mk(0.0f, -f.z, f.y), c);
    obox_edge_axis(n + 1, p0.z, p0.x, p1.z, p1.x, p2.z, p2.x, v.z, v.x, f.z, f.x, h.z, h.x, mk(f.z, 0.0f, -f.x), c);
    obox_edge_axis(n + 2, p0.x, p0.y, p1.x, p1.y, p2.x, p2.y, v.x, v.y, f.x, f.y, h.x, h.y, mk(-f.y, f.x, 0.0f), c);
}

// The time of impact of the cube of half extent h about the origin with the triangle {P0, P0 + E1, P0 + E2} translating by nD t:
// 0 on a start overlap (c.ax = 13), else max(te, 0) when te <= tx and tx >= 0 (c.ax = the axis of te, c.sw its speed, c.a the axis),
// +inf when the pair is no candidate.  The caller compares with tmax.
__device__ __forceinline__ float obox_triangle(const f3& h, const f3& P0, const f3& E1, const f3& E2, const f3& nD, OBoxClip& c)
{
    const f3 p0 = P0, p1 = p0 + E1, p2 = p0 + E2;
    c.te = -INFINITY; c.tx = INFINITY; c.ax = 0; c.sw = 0.0f; c.a = mk(0.0f);
    obox_axis(0, fmin3(p0.x, p1.x, p2.x), fmax3(p0.x, p1.x, p2.x), h.x, nD.x, mk(1.0f, 0.0f, 0.0f), c);
    obox_axis(1, fmin3(p0.y, p1.y, p2.y), fmax3(p0.y, p1.y, p2.y), h.y, nD.y, mk(0.0f, 1.0f, 0.0f), c);
    obox_axis(2, fmin3(p0.z, p1.z, p2.z), fmax3(p0.z, p1.z, p2.z), h.z, nD.z, mk(0.0f, 0.0f, 1.0f), c);
    const f3 nrm = cross(E1, E2);
    const float dn = dot(nrm, p0);
    const float rn = (h.x * fabsf(nrm.x) + h.y * fabsf(nrm.y)) + h.z * fabsf(nrm.z);
    obox_axis(3, dn, dn, rn, dot(nrm, nD), nrm, c);
    const f3 f1 = E2 - E1;
    obox_edge(4, p0, p1, p2, nD, E1, h, c);
    obox_edge(7, p0, p1, p2, nD, f1, h, c);
    obox_edge(10, p0, p1, p2, nD, E2, h, c);
    float t = (c.te <= c.tx && c.tx >= 0.0f) ? (c.te > 0.0f ? c.te : 0.0f) : INFINITY;
    // the start overlap is section 38's own call on the same local vectors, not the entry times
    if (tri_box_overlap(mk(0.0f), h, P0, E1, E2)) { t = 0.0f; c.ax = 13; }
    return t;
}

// The record's normal and point for the winner (w: what obox_triangle left, w.ax in 0..12; t the time): q the box, d the direction,
// v0 e1 e2 the triangle's stored vectors, P0 E1 E2 nD as above.
__device__ __forceinline__ void obox_contact(const OBoxQuery& q, const f3& d, const f3& v0, const f3& e1, const f3& e2, const f3& P0, const f3& E1, const f3& E2,
                                             const f3& nD, const OBoxClip& w, float t, f3& nrm_out, f3& pt_out)
{
    const int ax = w.ax;
    const float sw = w.sw;
    const f3 h = q.h;
    const f3 p0 = P0, p1 = p0 + E1, p2 = p0 + E2;
    const f3 F1 = E2 - E1;
    // features 4..12 are 4 + 3 g + i: the edge g in ((v0, e1), (v0 + e1, e2 - e1), (v0, e2)) and the box axis i, both read off ax by compares
    const bool g0 = ax < 7, g1 = !g0 && ax < 10;
    const bool i0 = ax == 4 || ax == 7 || ax == 10, i1 = ax == 5 || ax == 8 || ax == 11;
    const f3 f = g0 ? E1 : g1 ? F1 : E2;
    // the axis in local coordinates, signed from the triangle to the box: the triangle moves along +axis when sw > 0, so the box lies on that side
    const f3 a = w.a;
    const f3 g = sw > 0.0f ? a : mk(-a.x, -a.y, -a.z);
    const f3 W = mk((g.x * q.u.x + g.y * q.v.x) + g.z * q.w.x, (g.x * q.u.y + g.y * q.v.y) + g.z * q.w.y, (g.x * q.u.z + g.y * q.v.z) + g.z * q.w.z);
    const float len = sqrtf(dot(W, W));
    nrm_out = len > 0.0f ? mk(W.x / len, W.y / len, W.z / len) : mk(0.0f);
    // the box's support corner towards the triangle, in local coordinates
    const f3 sc = mk(g.x > 0.0f ? -h.x : h.x, g.y > 0.0f ? -h.y : h.y, g.z > 0.0f ? -h.z : h.z);
    if (ax < 3) {
        const float c0 = comp(p0, ax), c1 = comp(p1, ax), c2 = comp(p2, ax);
        const float ext = sw > 0.0f ? fmax3(c0, c1, c2) : fmin3(c0, c1, c2);
        pt_out = c0 == ext ? v0 : c1 == ext ? v0 + e1 : v0 + e2;
    } else if (ax == 3) {
        const f3 cen = mk(q.c.x + d.x * t, q.c.y + d.y * t, q.c.z + d.z * t);
        pt_out = mk(cen.x + ((sc.x * q.u.x + sc.y * q.v.x) + sc.z * q.w.x), cen.y + ((sc.x * q.u.y + sc.y * q.v.y) + sc.z * q.w.y),
                    cen.z + ((sc.x * q.u.z + sc.y * q.v.z) + sc.z * q.w.z));
    } else {
        const f3 pa = g1 ? p1 : p0;
        const f3 al = mk(pa.x + nD.x * t, pa.y + nD.y * t, pa.z + nD.z * t);
        // (j, k) the two axes after i
        const float fj = i0 ? f.y : i1 ? f.z : f.x, fk = i0 ? f.z : i1 ? f.x : f.y;
        const float dj = (i0 ? sc.y : i1 ? sc.z : sc.x) - (i0 ? al.y : i1 ? al.z : al.x), dk = (i0 ? sc.z : i1 ? sc.x : sc.y) - (i0 ? al.z : i1 ? al.x : al.y);
        const float ff = fj * fj + fk * fk;
        float s = (dj * fj + dk * fk) / ff;
        s = s < 0.0f ? 0.0f : s;
        s = s > 1.0f ? 1.0f : s;
        s = ff > 0.0f ? s : 0.0f;
        const f3 A = g1 ? v0 + e1 : v0;
        const f3 E = g0 ? e1 : g1 ? e2 - e1 : e2;
        pt_out = mk(A.x + E.x * s, A.y + E.y * s, A.z + E.z * s);
    }
}

}  // namespace ptd
