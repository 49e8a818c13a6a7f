"""NumPy statement of pt_query_nearest's record (include/acgpt.h states the same definition), the brute force over all triangles it is
held to, and the point sets its tests use.

Every operation is fp32 in the order of csrc/nearest.hip closest_on_triangle — plain multiplies and adds, one IEEE division per
triangle, the regions as masks applied in reverse order of priority — so the GPU's record equals this one bit for bit.  The triangle
is what the build stores in a TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0, one fp32 subtraction per component."""
import numpy as np

F = np.float32
MISS_PRIM = np.uint32(0xFFFFFFFF)
SHADE_MAT_MASK = np.uint32(0x00FFFFFF)          # kShadeMatMask (csrc/pt_device.h)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def closest_on_triangle(q, v0, ab, ac):
    """(d2, v, w, c) of points q against triangles {v0, v0 + ab, v0 + ac}; the arrays broadcast against each other, last axis xyz.  Any
    float dtype: float32 arrays give the GPU's bits, float64 arrays the same algorithm in double."""
    q, v0, ab, ac = np.broadcast_arrays(q, v0, ab, ac)
    one, zero = q.dtype.type(1.0), q.dtype.type(0.0)
    with np.errstate(all="ignore"):
        ap = q - v0
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = ap - ab
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = ap - ac
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        at_a = (d1 <= zero) & (d2 <= zero)
        at_b = (d3 >= zero) & (d4 <= d3)
        on_ab = (vc <= zero) & (d1 >= zero) & (d3 <= zero)
        at_c = (d6 >= zero) & (d5 <= d6)
        on_ac = (vb <= zero) & (d2 >= zero) & (d6 <= zero)
        on_bc = (va <= zero) & (e43 >= zero) & (e56 >= zero)
        num, den = np.full_like(d1, one), (va + vb) + vc
        num, den = np.where(on_bc, e43, num), np.where(on_bc, e43 + e56, den)
        num, den = np.where(on_ac, d2, num), np.where(on_ac, d2 - d6, den)
        num, den = np.where(on_ab, d1, num), np.where(on_ab, d1 - d3, den)
        t = num / den
        v, w = vb * t, vc * t
        v, w = np.where(on_bc, one - t, v), np.where(on_bc, t, w)
        v, w = np.where(on_ac, zero, v), np.where(on_ac, t, w)
        v, w = np.where(at_c, zero, v), np.where(at_c, one, w)
        v, w = np.where(on_ab, t, v), np.where(on_ab, zero, w)
        v, w = np.where(at_b, one, v), np.where(at_b, zero, w)
        v, w = np.where(at_a, zero, v), np.where(at_a, zero, w)
        c = (v0 + ab * v[..., None]) + ac * w[..., None]
        s = q - c
        dd = _dot(s, s)
    return dd, v, w, c


def records_of_scene(verts, idx):
    """(v0, e1, e2) float32 [n_tris, 3] each: what the build stores"""
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    tri = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)]
    v0 = tri[:, 0]
    return v0, tri[:, 1] - v0, tri[:, 2] - v0


def searchable(points):
    """False where a point is a miss before any traversal: a non-finite coordinate, a NaN or negative max_radius"""
    p = np.asarray(points, np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p[:, 0:3]).all(axis=1) & (p[:, 3] >= F(0.0))


def miss_records(n):
    """n miss records as uint32 [n, 8]: {-1, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0xFFFFFFFF}"""
    rec = np.zeros((n, 8), np.uint32)
    rec[:, 0] = F(-1.0).view(np.uint32)
    rec[:, 1] = MISS_PRIM
    rec[:, 7] = MISS_PRIM
    return rec


def nearest_records(points, verts, idx, mat_ids, chunk=2048):
    """pt_nearest records as uint32 [n, 8] (distance, prim, u, v, cx, cy, cz, material) by brute force: every point against every
    triangle, candidates d2 <= max_radius * max_radius (fp32), the smallest d2, ties to the lowest triangle index."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 4))
    n = p.shape[0]
    rec = miss_records(n)
    v0, e1, e2 = records_of_scene(verts, idx)
    if v0.shape[0] == 0 or n == 0:
        return rec
    mats = np.asarray(mat_ids, np.uint32)
    ok = searchable(p)
    for start in range(0, n, chunk):
        sl = slice(start, min(n, start + chunk))
        q = p[sl, None, 0:3]
        with np.errstate(all="ignore"):
            r2 = p[sl, 3] * p[sl, 3]
            d2, v, w, c = closest_on_triangle(q, v0[None], e1[None], e2[None])
            cand = (d2 <= r2[:, None]) & ok[sl, None]
        key = np.where(cand, d2, F(np.inf))
        best = key.min(axis=1)
        win = np.argmax(cand & (key == best[:, None]), axis=1)           # the first (lowest) index among the ties
        found = cand.any(axis=1)
        rows = np.arange(win.size)
        out = np.zeros((win.size, 8), np.float32)
        with np.errstate(all="ignore"):
            out[:, 0] = np.sqrt(d2[rows, win])
        out[:, 2] = v[rows, win]
        out[:, 3] = w[rows, win]
        out[:, 4:7] = c[rows, win]
        out = out.view(np.uint32)
        out[:, 1] = win.astype(np.uint32)
        out[:, 7] = mats[win] & SHADE_MAT_MASK
        sub = rec[sl]
        sub[found] = out[found]
    return rec


def closest_f64(q, v0, v1, v2):
    """(distance, point) in float64 from the fp32 inputs, the same region test in double: what the fp32 statement is measured against"""
    q, v0, v1, v2 = (np.asarray(a, np.float64) for a in (q, v0, v1, v2))
    d2, v, w, c = closest_on_triangle(q, v0, v1 - v0, v2 - v0)
    return np.sqrt(d2), c


# ---- point sets ------------------------------------------------------------------------------------------------------------------
# Fixed seeds.  With FINITE_RADIUS (in units of the scene box's diagonal) every set finds something on at least a quarter of its points
# and nothing on at least a tenth, on both Cornell fixtures, by the brute force alone (tests/test_nearest_host.py holds that).
POINT_SETS = ("surface", "inside", "shell", "features", "wall_planes")
SET_SIZE = 1000
FINITE_RADIUS = {"surface": 1e-4, "inside": 0.06, "shell": 9.93, "features": 0.0, "wall_planes": 0.05}


def scene_box(verts, idx):
    used = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3][np.unique(np.asarray(idx, np.uint32))]
    return used.min(axis=0), used.max(axis=0)


def point_set(name, verts, idx, camera, first_hits=None):
    """SET_SIZE points (x, y, z) float32 of the named set.  camera: (eye, U, V, W).  first_hits: for "surface", a function rays ->
    (t, prim) of closest hits (the GPU tests pass pt_trace_closest, the host test the brute force below)."""
    import denoise_ref as dr
    lo, hi = scene_box(verts, idx)
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    idx = np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)
    ext = hi - lo
    diag = F(np.sqrt(float((ext * ext).sum())))
    c = F(0.5) * (lo + hi)
    n = SET_SIZE
    if name == "surface":           # first-hit points of camera rays, o + t d per component: on the surface or within an ulp of it;
        rng = np.random.default_rng(111)        # rays that hit nothing leave their far point, well outside the box
        rays = dr.pixel_rays(97, 61, *camera)[np.sort(rng.permutation(97 * 61)[:n])]
        t, prim = (first_hits or (lambda r: ray_first_hits(r, verts, idx)))(rays)
        t = np.where(np.asarray(prim) == MISS_PRIM, F(4.0) * diag, np.asarray(t, np.float32)).astype(np.float32)
        return (rays[:, 0:3] + t[:, None] * rays[:, 3:6]).astype(np.float32)
    if name == "inside":            # uniform in the scene box
        rng = np.random.default_rng(222)
        return (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
    if name == "shell":             # ten box diagonals from the centre, give or take a twentieth: some within 10 diagonals of the surface, some not
        rng = np.random.default_rng(333)
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
        return (c + d * (diag * rng.uniform(9.5, 10.5, (n, 1)).astype(np.float32))).astype(np.float32)
    if name == "features":          # a fixed random three quarters of the set from feature_points, the rest pushed off such points
        pts = feature_points(verts, idx)
        rng = np.random.default_rng(444)
        pts = pts[rng.permutation(pts.shape[0])][:(n * 3) // 4]
        off = pts[rng.integers(0, pts.shape[0], n - pts.shape[0])] + (rng.normal(size=(n - pts.shape[0], 3)) * 0.01 * float(diag)).astype(np.float32)
        return np.concatenate([pts, off]).astype(np.float32)[rng.permutation(n)]
    if name == "wall_planes":       # in the planes of the scene box's faces, spread to 1.3 times the face: inside the face's outline and just outside the box
        rng = np.random.default_rng(555)
        p = (c + (rng.random((n, 3)).astype(np.float32) - F(0.5)) * ext * F(1.3)).astype(np.float32)
        face = rng.integers(0, 3, n)
        side = rng.integers(0, 2, n)
        p[np.arange(n), face] = np.where(side == 0, lo[face], hi[face])
        return p
    raise ValueError(name)


def feature_points(verts, idx):
    """Every vertex, edge midpoint and centroid of every triangle, computed in fp32, 7 per triangle: all vertices a, all b, all c, the
    midpoints of ab, bc, ca, the centroids"""
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    tri = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    return np.concatenate([a, b, c, F(0.5) * (a + b), F(0.5) * (b + c), F(0.5) * (c + a), (a + b + c) * F(1.0 / 3.0)]).astype(np.float32)


def with_radius(points, radius):
    """(n, 4) float32 {x, y, z, max_radius}"""
    p = np.zeros((np.asarray(points).shape[0], 4), np.float32)
    p[:, 0:3] = points
    p[:, 3] = radius
    return p


def set_radius(name, verts, idx):
    lo, hi = scene_box(verts, idx)
    ext = hi - lo
    return F(FINITE_RADIUS[name]) * F(np.sqrt(float((ext * ext).sum())))


def ray_first_hits(rays, verts, idx):
    """Closest hits (t, prim) of rays by a float64 Moeller-Trumbore brute force, interval (tmin, tmax): the host test's stand-in for
    pt_trace_closest when it makes the "surface" set (the points need not be the GPU's: each side's set is checked against the
    reference on its own points)."""
    rays = np.asarray(rays, np.float64).reshape(-1, 8)
    v = np.asarray(verts, np.float64).reshape(-1, 4)[:, :3]
    tri = v[np.asarray(idx, np.int64).reshape(-1, 3)]
    v0, e1, e2 = tri[:, 0][None], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    with np.errstate(all="ignore"):
        p = np.cross(d, e2)
        det = (e1 * p).sum(-1)
        s = o - v0
        u = (s * p).sum(-1) / det
        qv = np.cross(s, e1)
        vv = (d * qv).sum(-1) / det
        t = (e2 * qv).sum(-1) / det
        ok = (det != 0) & (u >= 0) & (vv >= 0) & (u + vv <= 1) & (t > rays[:, None, 6]) & (t < rays[:, None, 7])
    t = np.where(ok, t, np.inf)
    prim = t.argmin(axis=1)
    best = t[np.arange(t.shape[0]), prim]
    hit = np.isfinite(best)
    return np.where(hit, best, -1.0).astype(np.float32), np.where(hit, prim, 0xFFFFFFFF).astype(np.uint32)


# the bad points of the tests: each with what makes it a miss before any traversal; `good` is the point they are made from
def bad_points(good):
    good = np.asarray(good, np.float32).reshape(4)
    out, why = [], []
    for k in range(3):
        for val in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = val
            out.append(r); why.append("coordinate %d = %s" % (k, val))
    for val, what in ((np.nan, "NaN"), (-np.inf, "-inf"), (F(-1.0), "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        r = good.copy(); r[3] = val
        out.append(r); why.append("max_radius = %s" % what)
    return np.array(out, np.float32), why
