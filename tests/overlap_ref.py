"""NumPy statement of pt_query_overlap's triangle-box test (include/acgpt.h states the same definition), the brute force over all
triangles it is held to, and the box sets its tests use.

Every operation is fp32 in the order of csrc/overlap.hip tri_box_overlap — plain multiplies, adds and subtractions, fmin / fmax that
ignore a NaN operand, the 13 closed conditions combined by `and` — so the GPU's counts, lists and any bytes equal these bit for bit.
The triangle is what the build stores in a TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0, one fp32 subtraction per component."""
import numpy as np

from nearest_ref import records_of_scene, scene_box

F = np.float32
NO_PRIM = np.uint32(0xFFFFFFFF)
MAX_PRIMS = 8                   # PT_QUERY_OVERLAP_MAX


def _fmin3(a, b, c):
    return np.fmin(np.fmin(a, b), c)


def _fmax3(a, b, c):
    return np.fmax(np.fmax(a, b), c)


def _faces(p0, p1, p2, h):
    keep = np.ones(p0.shape[:-1], bool)
    for k in range(3):
        keep &= (_fmin3(p0[..., k], p1[..., k], p2[..., k]) <= h[..., k]) & (_fmax3(p0[..., k], p1[..., k], p2[..., k]) >= -h[..., k])
    return keep


def _plane(p0, h, e1, e2):
    nx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
    ny = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
    nz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    d = (nx * p0[..., 0] + ny * p0[..., 1]) + nz * p0[..., 2]
    r = (h[..., 0] * np.abs(nx) + h[..., 1] * np.abs(ny)) + h[..., 2] * np.abs(nz)
    return (d <= r) & (d >= -r)


def _edges(p0, p1, p2, h, e1, e2):
    keep = np.ones(p0.shape[:-1], bool)
    for f in (e1, e2 - e1, e2):
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            s0 = p0[..., k] * f[..., j] - p0[..., j] * f[..., k]
            s1 = p1[..., k] * f[..., j] - p1[..., j] * f[..., k]
            s2 = p2[..., k] * f[..., j] - p2[..., j] * f[..., k]
            r = h[..., j] * np.abs(f[..., k]) + h[..., k] * np.abs(f[..., j])
            keep &= (_fmin3(s0, s1, s2) <= r) & (_fmax3(s0, s1, s2) >= -r)
    return keep


def conditions(c, h, v0, e1, e2):
    """(faces, plane, edges): the three groups of the 13 conditions, bool each.  The arrays broadcast against each other, last axis xyz.
    Any float dtype: float32 arrays give the GPU's bits, float64 arrays the same algorithm in double."""
    c, h, v0, e1, e2 = np.broadcast_arrays(c, h, v0, e1, e2)
    with np.errstate(all="ignore"):
        p0 = v0 - c
        p1 = p0 + e1
        p2 = p0 + e2
        return _faces(p0, p1, p2, h), _plane(p0, h, e1, e2), _edges(p0, p1, p2, h, e1, e2)


def tri_box_overlap(c, h, v0, e1, e2):
    """bool: does the triangle {v0, v0 + e1, v0 + e2} overlap the box of centre c and half extent h: all 13 conditions hold.  The plane
    and the edge axes are evaluated only on the pairs the faces keep, which changes no pair's arithmetic."""
    c, h, v0, e1, e2 = np.broadcast_arrays(c, h, v0, e1, e2)
    with np.errstate(all="ignore"):
        p0 = v0 - c
        p1 = p0 + e1
        p2 = p0 + e2
        keep = _faces(p0, p1, p2, h)
        if keep.ndim == 0 or keep.mean() > 0.25:
            return keep & _plane(p0, h, e1, e2) & _edges(p0, p1, p2, h, e1, e2)
        sel = np.nonzero(keep)
        if sel[0].size:
            q0, q1, q2, hh, f1, f2 = (a[sel] for a in (p0, p1, p2, h, e1, e2))
            keep[sel] = _plane(q0, hh, f1, f2) & _edges(q0, q1, q2, hh, f1, f2)
    return keep


def as_boxes(centres, half_extents):
    """(n, 8) float32 records {cx, cy, cz, hx, hy, hz, 0, 0}"""
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    b = np.zeros((c.shape[0], 8), np.float32)
    b[:, 0:3] = c
    b[:, 3:6] = np.broadcast_to(np.asarray(half_extents, np.float32), c.shape)
    return b


def searchable(boxes):
    """False where a box is a miss before any traversal: a non-finite centre or half extent, a negative or NaN half extent"""
    b = np.asarray(boxes, np.float32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(b[:, 0:6]).all(axis=1) & (b[:, 3:6] >= F(0.0)).all(axis=1)


def overlap_matrix(boxes, verts, idx, dtype=np.float32, chunk=1024):
    """bool [n, n_tris]: box i against triangle j, by the statement in `dtype` (the fp32 records widened for float64), with the miss
    rule applied"""
    b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 8))
    v0, e1, e2 = (a.astype(dtype) for a in records_of_scene(verts, idx))
    out = np.zeros((b.shape[0], v0.shape[0]), bool)
    if v0.shape[0] == 0 or b.shape[0] == 0:
        return out
    ok = searchable(b)
    for start in range(0, b.shape[0], chunk):
        sl = slice(start, min(b.shape[0], start + chunk))
        c, h = b[sl, None, 0:3].astype(dtype), b[sl, None, 3:6].astype(dtype)
        out[sl] = tri_box_overlap(c, h, v0[None], e1[None], e2[None]) & ok[sl, None]
    return out


def lists_of_matrix(m, max_prims):
    """(counts uint32 [n], prims uint32 [n, max_prims], any uint8 [n]) of an overlap matrix: the count not clamped, the lowest
    max_prims indices ascending, 0xFFFFFFFF past the last one"""
    n, t = m.shape
    counts = m.sum(axis=1).astype(np.uint32)
    prims = np.full((n, max_prims), NO_PRIM, np.uint32)
    if max_prims and t:
        rank = np.cumsum(m, axis=1) - 1                                        # position of a kept triangle among the box's kept ones
        rows, cols = np.nonzero(m & (rank < max_prims))
        prims[rows, rank[rows, cols]] = cols.astype(np.uint32)
    return counts, prims, (counts != 0).astype(np.uint8)


def overlap_records(boxes, verts, idx, max_prims=MAX_PRIMS, chunk=1024):
    """(counts, prims, any) by brute force: every box against every triangle"""
    return lists_of_matrix(overlap_matrix(boxes, verts, idx, np.float32, chunk), max_prims)


# ---- box sets --------------------------------------------------------------------------------------------------------------------
# Fixed seeds.  tests/test_overlap_host.py holds the shares of the mixed sets on the Cornell fixtures by the brute force alone.
BOX_SETS = ("random", "grid", "centroids", "first_hits", "wall_faces", "far", "whole", "outside")
MIXED_SETS = ("random", "grid")
SET_SIZE = 1000
GRID = (16, 16, 16)


def _diag(lo, hi):
    ext = (hi - lo).astype(np.float64)
    return float(np.sqrt((ext * ext).sum()))


def grid_boxes(resolution, lo, hi):
    """The cells of an (nz, ny, nx) grid over [lo, hi] as boxes, x fastest: bakeOccupancy's, centres as distanceFieldPoints makes them,
    the half extent half a cell computed in float64 and rounded up to float32"""
    import acgpathtracing_amd as pt
    nz, ny, nx = resolution
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    half64 = 0.5 * (hi64 - lo64) / np.array([nx, ny, nz], np.float64)
    half = half64.astype(np.float32)
    half[half.astype(np.float64) < half64] = np.nextafter(half, F(np.inf))[half.astype(np.float64) < half64]
    return as_boxes(pt.distanceFieldPoints(resolution, lo64, hi64), half)


def box_set(name, verts, idx, camera=None, first_hits=None, n=SET_SIZE):
    """n boxes (n, 8) float32 of the named set, from the scene's own box.  camera: (eye, U, V, W) and first_hits: rays -> (t, prim) for
    "first_hits" (the GPU tests pass pt_trace_closest, the host test nearest_ref's brute force)."""
    import nearest_ref as nr
    lo, hi = scene_box(verts, idx)
    ext = hi - lo
    diag = F(_diag(lo, hi)) if _diag(lo, hi) > 0 else F(1.0)
    cen = F(0.5) * (lo + hi)
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    tri = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)]
    if name == "random":            # uniform centres in the scene box, half extents log-uniform per axis in 1e-4 .. 0.2 of the diagonal
        rng = np.random.default_rng(808)
        c = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        h = (diag * F(10.0) ** rng.uniform(-4.0, np.log10(0.2), (n, 3)).astype(np.float32)).astype(np.float32)
        return as_boxes(c, h)
    if name == "grid":              # the 16^3 cell grid over the scene box, x fastest; the first n cells of a fixed permutation when n is smaller
        b = grid_boxes(GRID, lo, hi)
        if n >= b.shape[0]:
            return b
        return b[np.sort(np.random.default_rng(818).permutation(b.shape[0])[:n])]
    if name == "centroids":         # around centroids, half extents down to 1e-6 of the diagonal: every box names its own triangle
        rng = np.random.default_rng(828)
        pick = rng.integers(0, tri.shape[0], n)
        c = ((tri[pick, 0] + tri[pick, 1] + tri[pick, 2]) * F(1.0 / 3.0)).astype(np.float32)
        h = (diag * F(10.0) ** rng.uniform(-6.0, -1.5, (n, 3)).astype(np.float32)).astype(np.float32)
        return as_boxes(c, h)
    if name == "first_hits":        # flat, segment and point boxes on the first-hit points of camera rays
        rng = np.random.default_rng(838)
        pts = nr.point_set("surface", verts, idx, camera, first_hits=first_hits)[:n]
        pts = np.resize(pts, (n, 3))
        h = (diag * F(10.0) ** rng.uniform(-5.0, -1.5, (n, 3)).astype(np.float32)).astype(np.float32)
        kind = np.arange(n) % 4            # 0: point, 1: segment (two zero axes), 2: rectangle (one zero axis), 3: a thin box
        axis = rng.integers(0, 3, n)
        h[kind == 0] = 0.0
        for k in range(3):
            h[(kind == 1) & (axis != k), k] = 0.0
            h[(kind == 2) & (axis == k), k] = 0.0
        return as_boxes(pts, h)
    if name == "wall_faces":        # one face placed in a wall's plane (the scene box's) or through a vertex: lo + h or hi - h is the centre
        rng = np.random.default_rng(848)
        c = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        h = (diag * F(10.0) ** rng.uniform(-3.0, -1.0, (n, 3)).astype(np.float32)).astype(np.float32)
        axis, side, vert = rng.integers(0, 3, n), rng.integers(0, 2, n), rng.integers(0, 2, n).astype(bool)
        rows = np.arange(n)
        pv = tri[rng.integers(0, tri.shape[0], n), rng.integers(0, 3, n)]
        plane = np.where(vert, pv[rows, axis], np.where(side == 0, lo[axis], hi[axis])).astype(np.float32)
        c[vert] = pv[vert]
        # the box lies on the far side of the plane for half of them (touching from outside), on the near side for the rest
        out = rng.integers(0, 2, n).astype(bool)
        sign = np.where(out == (side == 0), F(-1.0), F(1.0)).astype(np.float32)
        c[rows, axis] = (plane + sign * h[rows, axis]).astype(np.float32)
        return as_boxes(c, h)
    if name == "far":               # centred 10 to 100 diagonals out along an axis, the near face within a few ulps of the scene box's face
        rng = np.random.default_rng(858)
        c = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        h = (diag * F(10.0) ** rng.uniform(-2.0, -0.7, (n, 3)).astype(np.float32)).astype(np.float32)
        axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
        rows = np.arange(n)
        dist = (diag * rng.uniform(10.0, 100.0, n).astype(np.float32)).astype(np.float32)
        face = np.where(side == 0, lo[axis], hi[axis]).astype(np.float32)
        ca = np.where(side == 0, face - dist, face + dist).astype(np.float32)
        ha = np.abs(face - ca).astype(np.float32)
        ulps = rng.integers(-3, 4, n)                       # the near face from three ulps short of the scene's face to three past it
        for _ in range(3):
            ha = np.where(ulps > 0, np.nextafter(ha, F(np.inf)), np.where(ulps < 0, np.nextafter(ha, F(0.0)), ha)).astype(np.float32)
            ulps = ulps - np.sign(ulps)
        c[rows, axis] = ca
        h[rows, axis] = ha
        return as_boxes(c, h)
    if name == "whole":             # boxes containing the whole scene (count == n_tris), growing
        rng = np.random.default_rng(868)
        h = (np.maximum(ext, diag * F(1e-3))[None, :] * (F(0.75) + rng.random((n, 3)).astype(np.float32) * F(10.0))).astype(np.float32)
        return as_boxes(np.broadcast_to(cen, (n, 3)), h)
    if name == "outside":           # far outside: nothing overlaps
        rng = np.random.default_rng(878)
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
        c = (cen + d * (diag * rng.uniform(3.0, 50.0, (n, 1)).astype(np.float32))).astype(np.float32)
        h = (diag * F(10.0) ** rng.uniform(-4.0, -0.5, (n, 3)).astype(np.float32)).astype(np.float32)
        return as_boxes(c, h)
    raise ValueError(name)


# the bad boxes of the tests: each with what makes it a miss before any traversal; `good` is the box they are made from
def bad_boxes(good):
    good = np.asarray(good, np.float32).reshape(8)
    out, why = [], []
    for k in range(6):
        for val in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = val
            out.append(r); why.append("float %d = %s" % (k, val))
    for k in range(3, 6):
        for val, what in ((F(-1.0), "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
            r = good.copy(); r[k] = val
            out.append(r); why.append("half extent %d = %s" % (k - 3, what))
    return np.array(out, np.float32), why


def surface_points_f64(verts, idx, n, seed=888):
    """n random points on the surface in float64 (triangle picked by index, uniform barycentrics), and their triangles"""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64).reshape(-1, 4)[:, :3]
    tri = v[np.asarray(idx, np.int64).reshape(-1, 3)]
    pick = rng.integers(0, tri.shape[0], n)
    a, b = rng.random(n), rng.random(n)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    p = tri[pick, 0] + a[:, None] * (tri[pick, 1] - tri[pick, 0]) + b[:, None] * (tri[pick, 2] - tri[pick, 0])
    return p, pick
