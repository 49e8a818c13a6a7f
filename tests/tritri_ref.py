"""NumPy statement of pt_query_triangles' triangle-triangle test (include/acgpt.h states the same definition), the brute force over all
pairs it is held to, and the query sets its tests use.

Every operation is fp32 in the order of csrc/tritri.hip tri_tri_intersect — plain multiplies, adds and subtractions, fmin / fmax that
ignore a NaN operand, the 20 closed conditions combined by `and` — so the GPU's counts, lists and any bytes equal these bit for bit.
The scene triangle is what the build stores in a TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0, one fp32 subtraction per component; the
query triangle is its three vertices a0, a1, a2.  Vectors are tuples of three component arrays."""
import numpy as np

from nearest_ref import records_of_scene, scene_box
from overlap_ref import lists_of_matrix                    # noqa: F401  (the list rule is pt_query_overlap's)

F = np.float32
MAX_PRIMS = 8                   # PT_QUERY_TRIANGLES_MAX
GROUPS = ("boxes", "normals", "edges", "in_a", "in_b")


def _fmin3(a, b, c):
    return np.fmin(np.fmin(a, b), c)


def _fmax3(a, b, c):
    return np.fmax(np.fmax(a, b), c)


def _xyz(a):
    return a[..., 0], a[..., 1], a[..., 2]


def _add(a, b):
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1], a[2] - b[2]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]


def _box_gaps(a0, a1, a2, v0, e1, e2):
    """per axis k the two closed box conditions as gaps that are >= 0 where they hold: (qhi - min w, max w - qlo)"""
    w1, w2 = _add(v0, e1), _add(v0, e2)
    out = []
    for k in range(3):
        out.append(_fmax3(a0[k], a1[k], a2[k]) - _fmin3(v0[k], w1[k], w2[k]))
        out.append(_fmax3(v0[k], w1[k], w2[k]) - _fmin3(a0[k], a1[k], a2[k]))
    return out


def _boxes(a0, a1, a2, v0, e1, e2):
    w1, w2 = _add(v0, e1), _add(v0, e2)
    keep = True
    for k in range(3):
        keep = keep & (_fmin3(v0[k], w1[k], w2[k]) <= _fmax3(a0[k], a1[k], a2[k])) & (_fmax3(v0[k], w1[k], w2[k]) >= _fmin3(a0[k], a1[k], a2[k]))
    return keep


def _axes(a0, a1, a2, v0, e1, e2):
    """(p0, p1, p2, f1, f2) and the 17 axes in the statement's order, each with its group"""
    f1, f2 = _sub(a1, a0), _sub(a2, a0)
    p0 = _sub(v0, a0)
    p1, p2 = _add(p0, e1), _add(p0, e2)
    f21, e21 = _sub(f2, f1), _sub(e2, e1)
    nA, nB = _cross(f1, f2), _cross(e1, e2)
    axes = [("normals", nA), ("normals", nB)]
    axes += [("edges", _cross(a, b)) for a in (f1, f21, f2) for b in (e1, e21, e2)]
    axes += [("in_a", _cross(nA, a)) for a in (f1, f21, f2)]
    axes += [("in_b", _cross(nB, b)) for b in (e1, e21, e2)]
    return (p0, p1, p2, f1, f2), axes


def _axis_terms(L, p0, p1, p2, f1, f2):
    s0, s1, s2 = _dot(L, p0), _dot(L, p1), _dot(L, p2)
    t1, t2 = _dot(L, f1), _dot(L, f2)
    zero = s0.dtype.type(0.0)
    return _fmin3(s0, s1, s2), _fmax3(s0, s1, s2), _fmin3(zero, t1, t2), _fmax3(zero, t1, t2)


def _axis_keeps(L, p0, p1, p2, f1, f2):
    smin, smax, tmin, tmax = _axis_terms(L, p0, p1, p2, f1, f2)
    return (smin <= tmax) & (smax >= tmin)


def conditions(a0, a1, a2, v0, e1, e2):
    """{group: bool}: the five groups of the 20 conditions.  The arrays broadcast against each other, last axis xyz.  Any float dtype:
    float32 arrays give the GPU's bits, float64 arrays the same algorithm in double."""
    a0, a1, a2, v0, e1, e2 = (_xyz(a) for a in np.broadcast_arrays(a0, a1, a2, v0, e1, e2))
    with np.errstate(all="ignore"):
        out = {"boxes": _boxes(a0, a1, a2, v0, e1, e2)}
        vecs, axes = _axes(a0, a1, a2, v0, e1, e2)
        for group, L in axes:
            out[group] = out.get(group, True) & _axis_keeps(L, *vecs)
    return out


def tri_tri_intersect(a0, a1, a2, v0, e1, e2):
    """bool: does the scene triangle {v0, v0 + e1, v0 + e2} intersect the query triangle {a0, a1, a2}: all 20 conditions hold.  The 17
    axes are evaluated only on the pairs the boxes keep, which changes no pair's arithmetic."""
    arrs = np.broadcast_arrays(a0, a1, a2, v0, e1, e2)
    with np.errstate(all="ignore"):
        keep = np.array(_boxes(*(_xyz(a) for a in arrs)), bool)
        sel = np.nonzero(keep)
        if keep.ndim and sel[0].size:
            vecs, axes = _axes(*(_xyz(a[sel]) for a in arrs))
            ok = np.ones(sel[0].size, bool)
            for _, L in axes:
                ok &= _axis_keeps(L, *vecs)
            keep[sel] = ok
        elif not keep.ndim and keep:
            keep = np.array(all(bool(g) for g in conditions(*arrs).values()))
    return keep


def normalised_gaps(a0, a1, a2, v0, e1, e2):
    """[40, ...]: every condition as a signed distance that is >= 0 where the condition holds — the box conditions as they are, an
    axis' two conditions divided by |L|; +inf for an axis of length 0 (it separates nothing).  For float64 arrays: the measure of how
    far a pair is from a contact is the smallest of them."""
    a0, a1, a2, v0, e1, e2 = (_xyz(a) for a in np.broadcast_arrays(a0, a1, a2, v0, e1, e2))
    with np.errstate(all="ignore"):
        out = _box_gaps(a0, a1, a2, v0, e1, e2)
        vecs, axes = _axes(a0, a1, a2, v0, e1, e2)
        for _, L in axes:
            smin, smax, tmin, tmax = _axis_terms(L, *vecs)
            length = np.sqrt(_dot(L, L))
            for g in (tmax - smin, smax - tmin):
                out.append(np.where(length > 0, g / np.where(length > 0, length, 1.0), np.inf))
    return np.stack(out)


def as_records(tris):
    """(n, 12) float32 records {a0.xyz, 0, a1.xyz, 0, a2.xyz, 0} of (n, 3, 3) vertices"""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    r = np.zeros((t.shape[0], 3, 4), np.float32)
    r[:, :, :3] = t
    return r.reshape(-1, 12)


def vertices_of(records):
    """(n, 3, 3) float32: the nine coordinates of (n, 12) records"""
    return np.asarray(records, np.float32).reshape(-1, 3, 4)[:, :, :3]


def searchable(records):
    """False where a query is a miss before any traversal: a non-finite coordinate among its nine"""
    return np.isfinite(vertices_of(records)).all(axis=(1, 2))


def intersect_matrix(records, verts, idx, dtype=np.float32, chunk=1024):
    """bool [n, n_tris]: query i against scene triangle j, by the statement in `dtype` (the fp32 numbers widened for float64), with
    the miss rule applied.  Scene triangles whose nine stored numbers are the same, bit for bit, give the same answers: each distinct
    record is evaluated once."""
    q = vertices_of(records)
    v0, e1, e2 = records_of_scene(verts, idx)
    if v0.shape[0] == 0 or q.shape[0] == 0:
        return np.zeros((q.shape[0], v0.shape[0]), bool)
    rec9 = np.ascontiguousarray(np.concatenate([v0, e1, e2], axis=1), np.float32).view(np.uint32)
    _, first, inverse = np.unique(rec9, axis=0, return_index=True, return_inverse=True)
    v0, e1, e2 = (a[first].astype(dtype) for a in (v0, e1, e2))
    out = np.zeros((q.shape[0], first.size), bool)
    ok = searchable(records)
    for start in range(0, q.shape[0], chunk):
        sl = slice(start, min(q.shape[0], start + chunk))
        a = q[sl].astype(dtype)
        out[sl] = tri_tri_intersect(a[:, None, 0], a[:, None, 1], a[:, None, 2], v0[None], e1[None], e2[None]) & ok[sl, None]
    return out[:, inverse.reshape(-1)]


def triangle_records(records, verts, idx, max_prims=MAX_PRIMS, chunk=1024):
    """(counts, prims, any) by brute force: every query against every scene triangle"""
    return lists_of_matrix(intersect_matrix(records, verts, idx, np.float32, chunk), max_prims)


# ---- query sets ------------------------------------------------------------------------------------------------------------------
# Fixed seeds.  tests/test_tritri_host.py holds the shares on the Cornell fixtures by the brute force alone.
QUERY_SETS = ("random", "self", "edge", "coplanar", "wall_touch", "whole", "degenerate", "far", "outside")
SET_SIZE = 1000


def _diag(lo, hi):
    ext = (hi - lo).astype(np.float64)
    d = float(np.sqrt((ext * ext).sum()))
    return F(d) if d > 0 else F(1.0)


def _unit(rng, n):
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return d / np.sqrt((d * d).sum(axis=1, keepdims=True))


def query_set(name, verts, idx, camera=None, first_hits=None, n=SET_SIZE):
    """(n, 12) float32 records of the named set, from the scene's own box and triangles.  camera: (eye, U, V, W) and first_hits: rays
    -> (t, prim) for "degenerate" (the GPU tests pass the device's closest hits, the host test nearest_ref's brute force)."""
    import nearest_ref as nr
    lo, hi = scene_box(verts, idx)
    ext = hi - lo
    diag = _diag(lo, hi)
    cen = F(0.5) * (lo + hi)
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    tri = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)]
    rows = np.arange(n)
    if name == "random":            # centres uniform in the scene box, sizes log-uniform over 1e-3 .. 0.3 of the diagonal; a vertex is
        rng = np.random.default_rng(909)        # the centre plus the size times a normal deviate per coordinate
        c = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        size = (diag * F(10.0) ** rng.uniform(-3.0, np.log10(0.3), (n, 1, 1)).astype(np.float32)).astype(np.float32)
        return as_records(c[:, None, :] + size * rng.normal(size=(n, 3, 3)).astype(np.float32))
    if name == "self":              # the scene's own triangles: each names itself (p0 = 0, p1 = e1 = f1, p2 = e2 = f2)
        pick = np.resize(np.random.default_rng(919).permutation(tri.shape[0]), n)
        return as_records(tri[pick])
    if name == "edge":              # shares the edge v0 v1 with a scene triangle, the third vertex anywhere within 0.1 diagonals
        rng = np.random.default_rng(929)
        t = tri[rng.integers(0, tri.shape[0], n)]
        third = (t[:, 0] + _unit(rng, n) * (diag * rng.uniform(0.001, 0.1, (n, 1)).astype(np.float32))).astype(np.float32)
        return as_records(np.stack([t[:, 0], t[:, 1], third], axis=1))
    if name == "coplanar":          # affine combinations of a scene triangle's vertices: exactly coplanar on the axis-aligned walls
        rng = np.random.default_rng(939)
        t = tri[rng.integers(0, tri.shape[0], n)]
        e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        uw = rng.uniform(-1.0, 2.0, (n, 3, 2)).astype(np.float32)
        return as_records(t[:, None, 0] + uw[:, :, 0:1] * e1[:, None] + uw[:, :, 1:2] * e2[:, None])
    if name == "wall_touch":        # one vertex exactly in a wall's plane (a face of the scene box), the rest inside or outside the room
        rng = np.random.default_rng(949)
        a = (lo + rng.random((n, 3, 3)).astype(np.float32) * ext).astype(np.float32)
        axis, side, outside = rng.integers(0, 3, n), rng.integers(0, 2, n), rng.integers(0, 2, n).astype(bool)
        plane = np.where(side == 0, lo[axis], hi[axis]).astype(np.float32)
        depth = (diag * rng.uniform(0.01, 0.3, (n, 2)).astype(np.float32)).astype(np.float32)
        sign = np.where(outside == (side == 0), F(-1.0), F(1.0)).astype(np.float32)
        a[rows, 0, axis] = plane
        a[rows, 1, axis] = (plane + sign * depth[:, 0]).astype(np.float32)
        a[rows, 2, axis] = (plane + sign * depth[:, 1]).astype(np.float32)
        return as_records(a)
    if name == "whole":             # triangles 3 to 10 diagonals wide through the scene: long lists, deep stack
        rng = np.random.default_rng(959)
        c = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        r = (diag * rng.uniform(3.0, 10.0, (n, 1)).astype(np.float32)).astype(np.float32)
        x = _unit(rng, n)
        y = np.cross(x, _unit(rng, n)).astype(np.float32)
        y /= np.sqrt((y * y).sum(axis=1, keepdims=True))
        corners = [c + r * (F(np.cos(t)) * x + F(np.sin(t)) * y) for t in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0)]
        return as_records(np.stack(corners, axis=1).astype(np.float32))
    if name == "degenerate":        # points and segments on first-hit points of camera rays
        rng = np.random.default_rng(969)
        p = np.resize(nr.point_set("surface", verts, idx, camera, first_hits=first_hits)[:n], (n, 3))
        d = (_unit(rng, n) * (diag * F(10.0) ** rng.uniform(-4.0, -1.0, (n, 1)).astype(np.float32))).astype(np.float32)
        kind = rows % 4             # 0: a point; 1: a segment from p (a2 = a1); 2: a segment through p (a2 = p); 3: a segment from p (a2 = a0)
        a0 = np.where((kind == 2)[:, None], p - d, p).astype(np.float32)
        a1 = np.where((kind == 0)[:, None], p, p + d).astype(np.float32)
        a2 = np.where((kind == 1)[:, None], a1, p).astype(np.float32)
        return as_records(np.stack([a0, a1, a2], axis=1))
    if name == "far":               # reaching out 10 to 100 diagonals, the bounding box's near face within three ulps of the scene box's face
        rng = np.random.default_rng(979)
        a = (lo + rng.random((n, 3, 3)).astype(np.float32) * ext).astype(np.float32)
        axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
        face = np.where(side == 0, lo[axis], hi[axis]).astype(np.float32)
        out = np.where(side == 0, F(-np.inf), F(np.inf)).astype(np.float32)
        near = face.copy()
        ulps = rng.integers(-3, 4, n)            # positive: away from the scene
        for _ in range(3):
            near = np.where(ulps > 0, np.nextafter(near, out), np.where(ulps < 0, np.nextafter(near, -out), near)).astype(np.float32)
            ulps = ulps - np.sign(ulps)
        dist = (diag * rng.uniform(10.0, 100.0, (n, 2)).astype(np.float32)).astype(np.float32)
        sign = np.where(side == 0, F(-1.0), F(1.0)).astype(np.float32)
        a[rows, 0, axis] = near
        a[rows, 1, axis] = (face + sign * dist[:, 0]).astype(np.float32)
        a[rows, 2, axis] = (face + sign * dist[:, 1]).astype(np.float32)
        return as_records(a)
    if name == "outside":           # far outside: nothing intersects
        rng = np.random.default_rng(989)
        c = (cen + _unit(rng, n) * (diag * rng.uniform(3.0, 50.0, (n, 1)).astype(np.float32))).astype(np.float32)
        size = (diag * F(10.0) ** rng.uniform(-3.0, -0.5, (n, 1, 1)).astype(np.float32)).astype(np.float32)
        return as_records(c[:, None, :] + size * rng.uniform(-1.0, 1.0, (n, 3, 3)).astype(np.float32))
    raise ValueError(name)


# the bad queries of the tests: each with what makes it a miss before any traversal; `good` is the record they are made from
def bad_triangles(good):
    good = np.asarray(good, np.float32).reshape(12)
    out, why = [], []
    for k in (0, 1, 2, 4, 5, 6, 8, 9, 10):
        for val in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = val
            out.append(r); why.append("float %d = %s" % (k, val))
    return np.array(out, np.float32), why
