"""NumPy statement of pt_query_triangle_distance's record (include/acgpt.h states the same definition), the brute force over all
triangles it is held to, and the query sets its tests use.

Every operation is fp32 in the order of csrc/tridist.hip triangle_triangle: twenty-one sub-tests built from nearest_ref's
closest_on_triangle and segment_ref's segment_edge and crossing, plain multiplies and adds, every clamp and case a mask, so the GPU's
record equals this one bit for bit.  The scene triangle is what the build stores in a TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0.
Float64 arrays run the same algorithm in double."""
import numpy as np

import nearest_ref as nr
import segment_ref as sr
from nearest_ref import MISS_PRIM, SHADE_MAT_MASK, closest_on_triangle, records_of_scene, scene_box      # noqa: F401
from segment_ref import _dot, crossing, segment_edge

F = np.float32
GROUPS = ("a_vertex", "b_vertex", "edge_edge", "a_crosses", "b_crosses")


def group_of(feature):
    """index into GROUPS of feature numbers 0..20"""
    return np.searchsorted(np.array([3, 6, 15, 18]), np.asarray(feature).astype(np.int64), side="right")


def triangle_triangle(a0, a1, a2, v0, e1, e2):
    """(d2, feature, q, c) of query triangles {a0, a1, a2} against scene triangles {v0, v0 + e1, v0 + e2}; the arrays broadcast against
    each other, last axis xyz.  feature is an integer array, q the point on the query triangle, c the point on the scene triangle."""
    a0, a1, a2, v0, e1, e2 = np.broadcast_arrays(a0, a1, a2, v0, e1, e2)
    zero = a0.dtype.type(0.0)
    with np.errstate(all="ignore"):
        f1, f2, g = a1 - a0, a2 - a0, a2 - a1
        w1, w2, h = v0 + e1, v0 + e2, e2 - e1
        q_edges = ((a0, f1), (a0, f2), (a1, g))
        s_edges = ((v0, e1), (v0, e2), (w1, h))
        d2, _, _, c = closest_on_triangle(a0, v0, e1, e2)
        q = a0
        feat = np.zeros(d2.shape, np.int32)
        cands = []
        for i, a in ((1, a1), (2, a2)):
            dk, _, _, ck = closest_on_triangle(a, v0, e1, e2)
            cands.append((i, dk, a, ck))
        for j, b in enumerate((v0, w1, w2)):
            dk, _, _, qk = closest_on_triangle(b, a0, f1, f2)
            cands.append((3 + j, dk, qk, b))
        for i, (P, D) in enumerate(q_edges):
            a = _dot(D, D)
            for j, (A, E) in enumerate(s_edges):
                dk, s, ck = segment_edge(P, D, a, A, E)
                cands.append((6 + 3 * i + j, dk, P + D * s[..., None], ck))
        for k, dk, qk, ck in cands:
            take = (dk < d2) | (np.isnan(d2) & ~np.isnan(dk))           # the smaller d2, ties to the lower feature; a NaN is no candidate
            d2, feat, q, c = np.where(take, dk, d2), np.where(take, k, feat), np.where(take[..., None], qk, q), np.where(take[..., None], ck, c)
        crossed = np.zeros(d2.shape, bool)
        tests = [(15 + i, P, D, v0, e1, e2) for i, (P, D) in enumerate(q_edges)] + [(18 + j, A, E, a0, f1, f2) for j, (A, E) in enumerate(s_edges)]
        for k, P, D, t0, t1, t2 in tests:
            acc, _, x = crossing(P, D, t0, t1, t2)
            acc = acc & ~crossed                                         # of several accepted crossings the lowest feature number
            d2, feat, q, c = np.where(acc, zero, d2), np.where(acc, k, feat), np.where(acc[..., None], x, q), np.where(acc[..., None], x, c)
            crossed |= acc
    return d2, feat, q, c


def as_records(tris, radius=np.inf, eighth=0.0, twelfth=0.0):
    """(n, 12) float32 {a0, max_radius | a1, ignored | a2, ignored} from (n, 3, 3) or (n, 9) vertices"""
    t = np.asarray(tris, np.float32).reshape(-1, 9)
    g = np.zeros((t.shape[0], 12), np.float32)
    g[:, 0:3], g[:, 4:7], g[:, 8:11] = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    g[:, 3], g[:, 7], g[:, 11] = radius, eighth, twelfth
    return g


def searchable(records):
    """False where a query is a miss before any traversal: a non-finite one of the nine coordinates, a non-finite component of
    a1 - a0, a2 - a0 or a2 - a1, a NaN or negative max_radius.  The eighth and twelfth float are not looked at."""
    g = np.asarray(records, np.float32).reshape(-1, 12)
    a0, a1, a2 = g[:, 0:3], g[:, 4:7], g[:, 8:11]
    with np.errstate(all="ignore"):
        return (np.isfinite(a0).all(axis=1) & np.isfinite(a1).all(axis=1) & np.isfinite(a2).all(axis=1) & np.isfinite(a1 - a0).all(axis=1) &
                np.isfinite(a2 - a0).all(axis=1) & np.isfinite(a2 - a1).all(axis=1) & (g[:, 3] >= F(0.0)))


def miss_records(n):
    """n miss records as uint32 [n, 12]: {-1, 0xFFFFFFFF, 0, 0xFFFFFFFF | 0, 0, 0, 0 | 0, 0, 0, 0}"""
    rec = np.zeros((n, 12), np.uint32)
    rec[:, 0] = F(-1.0).view(np.uint32)
    rec[:, 1] = MISS_PRIM
    rec[:, 3] = MISS_PRIM
    return rec


def triangle_distance_records(records, verts, idx, mat_ids, chunk=32, return_d2=False):
    """pt_triangle_distance_hit records as uint32 [n, 12] (distance, prim, feature, material | qx, qy, qz, 0 | cx, cy, cz, 0) by brute
    force: every query against every distinct triangle record, candidates d2 <= max_radius * max_radius (fp32), the smallest d2, ties to the lowest
    triangle index.  return_d2: also the winning d2 per query, float32 (NaN where nothing is found), for records_within."""
    g = np.ascontiguousarray(np.asarray(records, np.float32).reshape(-1, 12))
    n = g.shape[0]
    rec = miss_records(n)
    win_d2 = np.full(n, np.nan, np.float32)
    v0, e1, e2 = records_of_scene(verts, idx)
    if v0.shape[0] == 0 or n == 0:
        return (rec, win_d2) if return_d2 else rec
    mats = np.asarray(mat_ids, np.uint32)
    ok = searchable(g)
    # Triangles whose stored vectors are the same bits give the same d2, and the tie goes to the lowest index: one evaluation per
    # distinct record, at its first index, in ascending order of those (20 000 coincident copies are one evaluation per query).
    stored = np.ascontiguousarray(np.concatenate([v0, e1, e2], axis=1)).view(np.uint32)
    first = np.sort(np.unique(stored, axis=0, return_index=True)[1])
    v0, e1, e2 = v0[first], e1[first], e2[first]
    for start in range(0, n, chunk):
        sl = slice(start, min(n, start + chunk))
        with np.errstate(all="ignore"):
            r2 = g[sl, 3] * g[sl, 3]
            d2, feat, q, c = triangle_triangle(g[sl, None, 0:3], g[sl, None, 4:7], g[sl, None, 8:11], v0[None], e1[None], e2[None])
            cand = (d2 <= r2[:, None]) & ok[sl, None]
        key = np.where(cand, d2, F(np.inf))
        best = key.min(axis=1)
        win = np.argmax(cand & (key == best[:, None]), axis=1)           # the first (lowest) index among the ties
        found = cand.any(axis=1)
        rows = np.arange(win.size)
        out = np.zeros((win.size, 12), np.float32)
        with np.errstate(all="ignore"):
            out[:, 0] = np.sqrt(d2[rows, win])
        out[:, 2] = feat[rows, win].astype(np.float32)
        out[:, 4:7] = q[rows, win]
        out[:, 8:11] = c[rows, win]
        out = out.view(np.uint32)
        out[:, 1] = first[win].astype(np.uint32)
        out[:, 3] = mats[first[win]] & SHADE_MAT_MASK
        sub = rec[sl]
        sub[found] = out[found]
        win_d2[sl] = np.where(found, d2[rows, win], F(np.nan))
    return (rec, win_d2) if return_d2 else rec


def records_within(rec_inf, win_d2, radius):
    """The records at max_radius = radius from those at +inf and their winning d2 (segment_ref.records_within's argument)"""
    with np.errstate(all="ignore"):
        r = np.broadcast_to(np.asarray(radius, np.float32), win_d2.shape)
        keep = win_d2 <= r * r
    return np.where(keep[:, None], rec_inf, miss_records(rec_inf.shape[0]))


def distance_f64(a0, a1, a2, v0, e1, e2):
    """The float64 formulation the statement is compared with: the minimum of six float64 segment_triangle calls, the three edges of
    each triangle against the other triangle.  Inputs are the fp32 values; the scene triangle is {v0, v0 + e1, v0 + e2} in double."""
    a0, a1, a2, v0, e1, e2 = (np.asarray(x, np.float64) for x in (a0, a1, a2, v0, e1, e2))
    w1, w2 = v0 + e1, v0 + e2
    best = None
    for p, q in ((a0, a1), (a0, a2), (a1, a2)):
        d2 = sr.segment_triangle(p, q, v0, e1, e2)[0]
        best = d2 if best is None else np.fmin(best, d2)
    for p, q in ((v0, w1), (v0, w2), (w1, w2)):
        best = np.fmin(best, sr.segment_triangle(p, q, a0, a1 - a0, a2 - a0)[0])
    return np.sqrt(best)


# ---- the two box bounds of the walk, in float64 (what the kernel's bounds approximate from below) -----------------------------------
def bound_a(a0, a1, a2, lo, hi):
    """squared distance between the query triangle's bounding box and the box [lo, hi]"""
    tlo, thi = np.minimum(np.minimum(a0, a1), a2), np.maximum(np.maximum(a0, a1), a2)
    m, hd = 0.5 * (tlo + thi), 0.5 * (thi - tlo)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    e = np.maximum(np.abs(c - m) - (h + hd), 0.0)
    return (e * e).sum(axis=-1)


def bound_b(a0, a1, a2, lo, hi):
    """the squared separation of the box from the query triangle's plane along its unit normal; 0 for a normal without length"""
    nrm = np.cross(a1 - a0, a2 - a0)
    ln = np.sqrt((nrm * nrm).sum(axis=-1, keepdims=True))
    with np.errstate(all="ignore"):
        nrm = np.where(ln > 0, nrm / ln, 0.0)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    sep = np.maximum(np.abs(((c - a0) * nrm).sum(axis=-1)) - (h * np.abs(nrm)).sum(axis=-1), 0.0)
    return sep * sep


# ---- query sets --------------------------------------------------------------------------------------------------------------------
# Fixed seeds.  With FINITE_RADIUS (in units of the scene box's diagonal) every set finds something on at least a quarter of its
# queries and nothing on at least a tenth, on both Cornell fixtures, by the brute force alone (tests/test_tridist_host.py holds that).
QUERY_SETS = ("small", "large", "shell", "offset", "touching")
SET_SIZE = 1000
FINITE_RADIUS = {"small": 0.03, "large": 0.004, "shell": 9.7, "offset": 0.01, "touching": 0.0}
_unit = sr._unit


def query_set(name, verts, idx, n=SET_SIZE):
    """n query triangles float32 [n, 9] (a0, a1, a2) of the named set"""
    lo, hi = scene_box(verts, idx)
    ext = hi - lo
    diag = F(np.sqrt(float((ext * ext).sum())))
    c = F(0.5) * (lo + hi)
    if name == "small":             # a0 uniform in the box, a1 and a2 at 0.02 diagonals in random directions
        rng = np.random.default_rng(1201)
        a0 = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        return np.concatenate([a0, a0 + _unit(rng, n) * (F(0.02) * diag), a0 + _unit(rng, n) * (F(0.02) * diag)], axis=1).astype(np.float32)
    if name == "large":             # three uniform vertices
        rng = np.random.default_rng(1202)
        return np.concatenate([lo + rng.random((n, 3)).astype(np.float32) * ext for _ in range(3)], axis=1).astype(np.float32)
    if name == "shell":             # ten box diagonals from the centre, give or take a twentieth, edges of about 0.3 diagonals
        rng = np.random.default_rng(1203)
        a0 = (c + _unit(rng, n) * (diag * rng.uniform(9.5, 10.5, (n, 1)).astype(np.float32))).astype(np.float32)
        a1 = a0 + _unit(rng, n) * (diag * rng.uniform(0.25, 0.35, (n, 1)).astype(np.float32))
        a2 = a0 + _unit(rng, n) * (diag * rng.uniform(0.25, 0.35, (n, 1)).astype(np.float32))
        return np.concatenate([a0, a1, a2], axis=1).astype(np.float32)
    if name == "offset":            # a scene triangle shrunk to half about its centroid and moved 0 to 0.02 diagonals along +- its normal: parallel faces
        rng = np.random.default_rng(1204)
        v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
        tri = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)]
        if tri.shape[0] == 0:
            return query_set("small", verts, idx, n)
        t = tri[rng.integers(0, tri.shape[0], n)].astype(np.float64)
        cen = t.mean(axis=1, keepdims=True)
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        ln = np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
        nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), _unit(rng, n))
        move = nrm * (rng.uniform(0.0, 0.02, (n, 1)) * float(diag) * rng.choice([-1.0, 1.0], (n, 1)))
        return (cen + 0.5 * (t - cen) + move[:, None, :]).reshape(n, 9).astype(np.float32)
    if name == "touching":          # a0 a vertex, edge midpoint or centroid, edges of 0.05 diagonals; a third pushed off by 0.03 diagonals
        pts = nr.feature_points(verts, idx)
        rng = np.random.default_rng(1205)
        a0 = pts[rng.integers(0, pts.shape[0], n)].copy()
        off = rng.permutation(n)[:n // 3]
        a0[off] += _unit(rng, off.size) * (F(0.03) * diag)
        return np.concatenate([a0, a0 + _unit(rng, n) * (F(0.05) * diag), a0 + _unit(rng, n) * (F(0.05) * diag)], axis=1).astype(np.float32)
    raise ValueError(name)


def tangent_triangles(verts, idx, n=SET_SIZE, seed=1206):
    """For sphere-like scenes: segment_ref.tangent_set's segment as one edge, the third vertex its midpoint moved by half the segment's
    length within the tangent plane.  The triangle lies in a plane tangent to a concentric sphere: the closest feature of the mesh
    is a vertex over the face's interior, or an edge against an edge."""
    segs = sr.tangent_set(verts, idx, n=n, seed=seed)
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    cen = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)].astype(np.float64).mean(axis=1)
    c = np.median(cen, axis=0)
    p0, p1 = segs[:, 0:3].astype(np.float64), segs[:, 3:6].astype(np.float64)
    m, d = 0.5 * (p0 + p1), p1 - p0
    w = np.cross(m - c, d)
    w /= np.sqrt((w * w).sum(axis=1, keepdims=True))
    a2 = m + w * (0.5 * np.sqrt((d * d).sum(axis=1, keepdims=True)))
    return np.concatenate([segs, a2.astype(np.float32)], axis=1).astype(np.float32)


def set_radius(name, verts, idx):
    lo, hi = scene_box(verts, idx)
    ext = hi - lo
    return F(FINITE_RADIUS[name]) * F(np.sqrt(float((ext * ext).sum())))


# the bad queries of the tests: each with what makes it a miss before any traversal; `good` is the record they are made from
def bad_triangles(good):
    good = np.asarray(good, np.float32).reshape(12)
    out, why = [], []
    for k in (0, 1, 2, 4, 5, 6, 8, 9, 10):
        for val in (np.nan, np.inf) + ((-np.inf,) if k in (0, 5, 10) else ()):
            r = good.copy(); r[k] = val
            out.append(r); why.append("float %d = %s" % (k, val))
    for p, q, what in ((0, 4, "a1 - a0"), (1, 9, "a2 - a0"), (6, 10, "a2 - a1")):
        r = good.copy(); r[[0, 1, 2, 4, 5, 6, 8, 9, 10]] = 0.0
        r[p] = F(3e38); r[q] = F(-3e38)
        out.append(r); why.append("finite vertices whose difference %s overflows" % what)
    for val, what in ((np.nan, "NaN"), (-np.inf, "-inf"), (F(-1.0), "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        r = good.copy(); r[3] = val
        out.append(r); why.append("max_radius = %s" % what)
    return np.array(out, np.float32), why
