"""NumPy statement of pt_query_segments' record (include/acgpt.h states the same definition), the brute force over all triangles it is
held to, and the segment sets its tests use.

Every operation is fp32 in the order of csrc/segment.hip segment_triangle — plain multiplies and adds, nine IEEE divisions per
triangle, every clamp and case a mask — so the GPU's record equals this one bit for bit.  The triangle is what the build stores in a
TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0, one fp32 subtraction per component.  Float64 arrays run the same algorithm in double."""
import numpy as np

import nearest_ref as nr
from nearest_ref import MISS_PRIM, SHADE_MAT_MASK, closest_on_triangle, miss_records, records_of_scene, scene_box      # noqa: F401

F = np.float32


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _clamp01(q):
    zero, one = q.dtype.type(0.0), q.dtype.type(1.0)
    q = np.where(q < zero, zero, q)
    return np.where(q > one, one, q)


def segment_edge(p0, d, a, A, E):
    """(d2, s, c) of segments {p0, d} (a = dot(d, d)) against edges {A, E}: Ericson 5.1.9 as selects, two divisions"""
    zero, one = p0.dtype.type(0.0), p0.dtype.type(1.0)
    r = p0 - A
    e = _dot(E, E)
    b = _dot(d, E)
    c = _dot(d, r)
    f = _dot(E, r)
    a, e, b, c, f = np.broadcast_arrays(a, e, b, c, f)
    a_ok, e_ok = a > zero, e > zero
    den = a * e - b * b
    both = a_ok & e_ok & (den > zero)
    only_a = a_ok & ~e_ok
    num1 = np.where(both, b * f - c * e, np.where(only_a, -c, zero))
    den1 = np.where(both, den, np.where(only_a, a, one))
    s0 = _clamp01(num1 / den1)
    tnom = b * s0 + f
    lo = e_ok & (tnom < zero)
    hi = e_ok & (tnom > e)
    out = lo | hi
    num2 = np.where(e_ok, tnom, zero)
    den2 = np.where(e_ok, e, one)
    num2 = np.where(lo, -c, num2)
    num2 = np.where(hi, b - c, num2)
    den2 = np.where(out, a, den2)
    num2 = np.where(out & ~a_ok, zero, num2)
    den2 = np.where(out & ~a_ok, one, den2)
    q2 = _clamp01(num2 / den2)
    s = np.where(out, q2, s0)
    t = np.where(lo, zero, np.where(hi, one, q2))
    ps = p0 + d * s[..., None]
    cs = A + E * t[..., None]
    w = ps - cs
    return _dot(w, w), s, cs


def crossing(p0, d, v0, e1, e2):
    """(accepted, s, c): the two-sided Moeller-Trumbore test of the segment against the triangle in plain multiplies and adds"""
    zero = p0.dtype.type(0.0)
    pv = _cross(d, e2)
    det = _dot(e1, pv)
    tv = p0 - v0
    U = _dot(tv, pv)
    qv = _cross(tv, e1)
    V = _dot(d, qv)
    T = _dot(e2, qv)
    neg = det < zero
    det, U, V, T = np.where(neg, -det, det), np.where(neg, -U, U), np.where(neg, -V, V), np.where(neg, -T, T)
    acc = (det > zero) & (U >= zero) & (V >= zero) & (U + V <= det) & (T >= zero) & (T <= det)
    s = T / det
    return acc, s, p0 + d * s[..., None]


def segment_triangle(p0, p1, v0, e1, e2):
    """(d2, s, feature, c) of segments {p0, p1} against triangles {v0, v0 + e1, v0 + e2}; the arrays broadcast against each other, last
    axis xyz.  feature is an integer array."""
    p0, p1, v0, e1, e2 = np.broadcast_arrays(p0, p1, v0, e1, e2)
    zero, one = p0.dtype.type(0.0), p0.dtype.type(1.0)
    with np.errstate(all="ignore"):
        d = p1 - p0
        a = _dot(d, d)
        d2, _, _, c = closest_on_triangle(p0, v0, e1, e2)
        s = np.zeros_like(d2)
        feat = np.zeros(d2.shape, np.int32)
        d1, _, _, c1 = closest_on_triangle(p1, v0, e1, e2)
        cands = [(d1, np.full_like(d1, one), c1), segment_edge(p0, d, a, v0, e1), segment_edge(p0, d, a, v0, e2), segment_edge(p0, d, a, v0 + e1, e2 - e1)]
        for k, (dk, sk, ck) in enumerate(cands):
            take = (dk < d2) | (np.isnan(d2) & ~np.isnan(dk))           # the smaller d2, ties to the lower feature; a NaN is no candidate
            d2, s, feat, c = np.where(take, dk, d2), np.where(take, sk, s), np.where(take, k + 1, feat), np.where(take[..., None], ck, c)
        acc, sx, cx = crossing(p0, d, v0, e1, e2)
        d2, s, feat, c = np.where(acc, zero, d2), np.where(acc, sx, s), np.where(acc, 5, feat), np.where(acc[..., None], cx, c)
    return d2, s, feat, c


def searchable(segments):
    """False where a segment is a miss before any traversal: a non-finite coordinate, a non-finite component of p1 - p0, a NaN or
    negative max_radius.  The eighth float is not looked at."""
    g = np.asarray(segments, np.float32).reshape(-1, 8)
    with np.errstate(all="ignore"):
        return np.isfinite(g[:, 0:3]).all(axis=1) & np.isfinite(g[:, 4:7]).all(axis=1) & np.isfinite(g[:, 4:7] - g[:, 0:3]).all(axis=1) & (g[:, 3] >= F(0.0))


def segment_records(segments, verts, idx, mat_ids, chunk=1024, return_d2=False):
    """pt_segment_hit records as uint32 [n, 8] (distance, prim, s, feature, cx, cy, cz, material) by brute force: every segment against
    every triangle, candidates d2 <= max_radius * max_radius (fp32), the smallest d2, ties to the lowest triangle index.  return_d2:
    also the winning d2 per segment, float32 (NaN where nothing is found), for records_within."""
    g = np.ascontiguousarray(np.asarray(segments, np.float32).reshape(-1, 8))
    n = g.shape[0]
    rec = miss_records(n)
    win_d2 = np.full(n, np.nan, np.float32)
    v0, e1, e2 = records_of_scene(verts, idx)
    if v0.shape[0] == 0 or n == 0:
        return (rec, win_d2) if return_d2 else rec
    mats = np.asarray(mat_ids, np.uint32)
    ok = searchable(g)
    for start in range(0, n, chunk):
        sl = slice(start, min(n, start + chunk))
        with np.errstate(all="ignore"):
            r2 = g[sl, 3] * g[sl, 3]
            d2, s, feat, c = segment_triangle(g[sl, None, 0:3], g[sl, None, 4:7], v0[None], e1[None], e2[None])
            cand = (d2 <= r2[:, None]) & ok[sl, None]
        key = np.where(cand, d2, F(np.inf))
        best = key.min(axis=1)
        win = np.argmax(cand & (key == best[:, None]), axis=1)           # the first (lowest) index among the ties
        found = cand.any(axis=1)
        rows = np.arange(win.size)
        out = np.zeros((win.size, 8), np.float32)
        with np.errstate(all="ignore"):
            out[:, 0] = np.sqrt(d2[rows, win])
        out[:, 2] = s[rows, win]
        out[:, 3] = feat[rows, win].astype(np.float32)
        out[:, 4:7] = c[rows, win]
        out = out.view(np.uint32)
        out[:, 1] = win.astype(np.uint32)
        out[:, 7] = mats[win] & SHADE_MAT_MASK
        sub = rec[sl]
        sub[found] = out[found]
        win_d2[sl] = np.where(found, d2[rows, win], F(np.nan))
    return (rec, win_d2) if return_d2 else rec


def records_within(rec_inf, win_d2, radius):
    """The records at max_radius = radius from those at +inf and their winning d2: the radius only decides whether the winner is a
    candidate — a smaller radius removes candidates from the far end, and the smallest d2 is the last to go."""
    with np.errstate(all="ignore"):
        r = np.broadcast_to(np.asarray(radius, np.float32), win_d2.shape)
        keep = win_d2 <= r * r
    return np.where(keep[:, None], rec_inf, miss_records(rec_inf.shape[0]))


def segment_f64(p0, p1, v0, v1, v2):
    """(distance, s, feature, c) in float64 from the fp32 inputs: the same statement in double"""
    p0, p1, v0, v1, v2 = (np.asarray(a, np.float64) for a in (p0, p1, v0, v1, v2))
    d2, s, feat, c = segment_triangle(p0, p1, v0, v1 - v0, v2 - v0)
    return np.sqrt(d2), s, feat, c


# ---- the two box bounds of the walk, in float64 (what the kernel's bounds approximate from below) -----------------------------------
def bound_a(p0, p1, lo, hi):
    """squared distance between the segment's bounding box and the box [lo, hi]"""
    m, hd = 0.5 * (p0 + p1), 0.5 * np.abs(p1 - p0)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    e = np.maximum(np.abs(c - m) - (h + hd), 0.0)
    return (e * e).sum(axis=-1)


def bound_b(p0, p1, lo, hi):
    """the largest squared separation of the segment and the box along the three axes normalize(d x axis_i); 0 for an axis whose cross
    product has no length"""
    m, d = 0.5 * (p0 + p1), p1 - p0
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    best = np.zeros(np.broadcast(m[..., 0], c[..., 0]).shape)
    for i in range(3):
        ax = np.zeros(3); ax[i] = 1.0
        nrm = np.cross(d, ax)
        ln = np.sqrt((nrm * nrm).sum(axis=-1, keepdims=True))
        with np.errstate(all="ignore"):
            nrm = np.where(ln > 0, nrm / ln, 0.0)
        sep = np.maximum(np.abs(((c - m) * nrm).sum(axis=-1)) - (h * np.abs(nrm)).sum(axis=-1), 0.0)
        best = np.maximum(best, sep * sep)
    return best


# ---- segment sets ------------------------------------------------------------------------------------------------------------------
# Fixed seeds.  With FINITE_RADIUS (in units of the scene box's diagonal) every set finds something on at least a quarter of its
# segments and nothing on at least a tenth, on both Cornell fixtures, by the brute force alone (tests/test_segment_host.py holds that).
SEGMENT_SETS = ("short", "long", "axis", "shell", "touching")
SET_SIZE = 1000
FINITE_RADIUS = {"short": 0.03, "long": 0.004, "axis": 0.02, "shell": 9.7, "touching": 0.0}


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(np.float32)


def segment_set(name, verts, idx, n=SET_SIZE):
    """n segments (p0, p1) float32 [n, 6] of the named set"""
    lo, hi = scene_box(verts, idx)
    ext = hi - lo
    diag = F(np.sqrt(float((ext * ext).sum())))
    c = F(0.5) * (lo + hi)
    if name == "short":             # start uniform in the box, 0.02 diagonals long, any direction
        rng = np.random.default_rng(1101)
        p0 = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        return np.concatenate([p0, p0 + _unit(rng, n) * (F(0.02) * diag)], axis=1).astype(np.float32)
    if name == "long":              # both ends uniform in the box
        rng = np.random.default_rng(1102)
        return np.concatenate([lo + rng.random((n, 3)).astype(np.float32) * ext, lo + rng.random((n, 3)).astype(np.float32) * ext], axis=1).astype(np.float32)
    if name == "axis":              # parallel to a coordinate axis, up to half the extent long
        rng = np.random.default_rng(1103)
        p0 = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        p1 = p0.copy()
        k = rng.integers(0, 3, n)
        p1[np.arange(n), k] += (rng.random(n).astype(np.float32) - F(0.5)) * ext[k]
        return np.concatenate([p0, p1], axis=1).astype(np.float32)
    if name == "shell":             # ten box diagonals from the centre, give or take a twentieth, about 0.3 diagonals long
        rng = np.random.default_rng(1104)
        p0 = (c + _unit(rng, n) * (diag * rng.uniform(9.5, 10.5, (n, 1)).astype(np.float32))).astype(np.float32)
        return np.concatenate([p0, p0 + _unit(rng, n) * (diag * rng.uniform(0.25, 0.35, (n, 1)).astype(np.float32))], axis=1).astype(np.float32)
    if name == "touching":          # from vertices, edge midpoints and centroids, 0.05 diagonals long; a quarter pushed off by 0.01 diagonals
        pts = nr.feature_points(verts, idx)
        rng = np.random.default_rng(1105)
        p0 = pts[rng.integers(0, pts.shape[0], n)].copy()
        off = rng.permutation(n)[:n // 4]
        p0[off] += _unit(rng, off.size) * (F(0.01) * diag)
        return np.concatenate([p0, p0 + _unit(rng, n) * (F(0.05) * diag)], axis=1).astype(np.float32)
    raise ValueError(name)


def tangent_set(verts, idx, n=SET_SIZE, seed=1106, shells=(1.05, 1.5)):
    """Segments of about one radius of the sphere that most of the scene's triangles lie on (the median of their centroids, and the
    centroids' median distance from it: the few triangles of a shell around an icosphere do not move either), tangent at their
    midpoint to a concentric sphere of shells[0] to shells[1] radii: the set on which the edge features win (on a convex mesh the
    nearest feature to a tangent line is often an edge)"""
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    cen = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)].astype(np.float64).mean(axis=1)
    c = np.median(cen, axis=0)
    rad = F(np.median(np.linalg.norm(cen - c, axis=1)))
    c = c.astype(np.float32)
    rng = np.random.default_rng(seed)
    u = _unit(rng, n)
    t = np.cross(u, _unit(rng, n)).astype(np.float32)
    t /= np.sqrt((t * t).sum(axis=1, keepdims=True))
    m = c + u * (rad * rng.uniform(shells[0], shells[1], (n, 1)).astype(np.float32))
    half = t * (F(0.5) * rad * rng.uniform(0.8, 1.2, (n, 1)).astype(np.float32))
    return np.concatenate([m - half, m + half], axis=1).astype(np.float32)


def with_radius(segs, radius, eighth=0.0):
    """(n, 8) float32 {p0, max_radius | p1, ignored}"""
    segs = np.asarray(segs, np.float32).reshape(-1, 6)
    g = np.zeros((segs.shape[0], 8), np.float32)
    g[:, 0:3] = segs[:, 0:3]
    g[:, 3] = radius
    g[:, 4:7] = segs[:, 3:6]
    g[:, 7] = eighth
    return g


def set_radius(name, verts, idx):
    lo, hi = scene_box(verts, idx)
    ext = hi - lo
    return F(FINITE_RADIUS[name]) * F(np.sqrt(float((ext * ext).sum())))


# the bad segments of the tests: each with what makes it a miss before any traversal; `good` is the record they are made from
def bad_segments(good):
    good = np.asarray(good, np.float32).reshape(8)
    out, why = [], []
    for k in (0, 1, 2, 4, 5, 6):
        for val in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = val
            out.append(r); why.append("float %d = %s" % (k, val))
    r = good.copy(); r[0] = F(3e38); r[4] = F(-3e38)
    out.append(r); why.append("finite ends whose difference overflows")
    for val, what in ((np.nan, "NaN"), (-np.inf, "-inf"), (F(-1.0), "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        r = good.copy(); r[3] = val
        out.append(r); why.append("max_radius = %s" % what)
    return np.array(out, np.float32), why
