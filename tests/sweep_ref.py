"""NumPy statement of pt_query_sweep's record (include/acgpt.h states the same definition), the brute force over all triangles it is
held to, and the sweep sets its tests use.

Every operation is fp32 in the order of csrc/sweep.hip sweep_triangle — plain multiplies and adds, IEEE divisions and square roots, the
eight features as masks, a NaN no candidate — so the GPU's record equals this one bit for bit.  With float64 arrays the same functions
give the same algorithm in double.  The triangle is what the build stores in a TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0, one fp32
subtraction per component; closest_on_triangle is nearest_ref's."""
import numpy as np

import nearest_ref as nr

F = np.float32
MISS_PRIM = np.uint32(0xFFFFFFFF)
SHADE_MAT_MASK = nr.SHADE_MAT_MASK
START, VERTEX, EDGE, FACE, NONE = 0, 1, 2, 3, 4          # the kind of feature that gives a triangle's time of impact


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _lower(t, kind, cand, tc, k):
    take = cand & (tc < t)
    return np.where(take, tc, t), np.where(take, k, kind)


def _vertex(m, d, dd, rr, t, kind):
    t0 = -_dot(m, d) / dd
    mp = m + d * t0[..., None]
    q = (rr - _dot(mp, mp)) / dd
    tv = t0 - np.sqrt(q)
    return _lower(t, kind, (q >= 0) & (tv >= 0), tv, VERTEX)


def _edge(m, E, d, rr, t, kind):
    ee, md, nd = _dot(E, E), _dot(m, E), _dot(d, E)
    mp = m - E * (md / ee)[..., None]
    dp = d - E * (nd / ee)[..., None]
    a = _dot(dp, dp)
    t0 = -_dot(mp, dp) / a
    mq = mp + dp * t0[..., None]
    q = (rr - _dot(mq, mq)) / a
    te = t0 - np.sqrt(q)
    s = md + te * nd
    return _lower(t, kind, (q >= 0) & (te >= 0) & (s >= 0) & (s <= ee), te, EDGE)


def _face(m, e1, e2, d, r, t, kind):
    n = _cross(e1, e2)
    nn, s0 = _dot(n, n), _dot(n, m)
    sr = np.where(s0 >= 0, r, -r)
    tf = (sr * np.sqrt(nn) - s0) / _dot(n, d)
    w = m + d * tf[..., None]
    u, v = _dot(_cross(w, e2), n) / nn, _dot(_cross(e1, w), n) / nn
    return _lower(t, kind, (tf >= 0) & (u >= 0) & (v >= 0) & (u + v <= 1), tf, FACE)


def sweep_triangle(o, d, r, v0, e1, e2):
    """(t, kind): the time of impact of spheres {o + t d, r} with triangles {v0, v0 + e1, v0 + e2}, +inf where there is none, and which
    kind of feature gave it.  o, d, v0, e1, e2 broadcast against each other (last axis xyz), r against their leading axes.  Any float
    dtype: float32 arrays give the GPU's bits, float64 arrays the same algorithm in double."""
    o, d, v0, e1, e2 = np.broadcast_arrays(o, d, v0, e1, e2)
    r = np.broadcast_to(np.asarray(r, o.dtype), o.shape[:-1])
    with np.errstate(all="ignore"):
        dd, rr = _dot(d, d), r * r
        t = np.full(o.shape[:-1], np.inf, o.dtype)
        kind = np.full(o.shape[:-1], NONE, np.int8)
        m0 = o - v0
        m1, m2 = o - (v0 + e1), o - (v0 + e2)
        for m in (m0, m1, m2):
            t, kind = _vertex(m, d, dd, rr, t, kind)
        t, kind = _edge(m0, e1, d, rr, t, kind)
        t, kind = _edge(m0, e2, d, rr, t, kind)
        t, kind = _edge(m1, e2 - e1, d, rr, t, kind)
        t, kind = _face(m0, e1, e2, d, r, t, kind)
        d2 = nr.closest_on_triangle(o, v0, e1, e2)[0]
        start = d2 <= rr
        t, kind = np.where(start, o.dtype.type(0), t), np.where(start, START, kind)
    return t, kind


def castable(sweeps):
    """False where a sweep is a miss before any traversal: a non-finite component of o or d, a radius that is NaN, negative or infinite,
    a NaN or negative tmax"""
    s = np.asarray(sweeps, np.float32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(s[:, 0:7]).all(axis=1) & (s[:, 6] >= F(0.0)) & (s[:, 7] >= F(0.0))


def miss_records(n):
    return nr.miss_records(n)


def sweep_records(sweeps, verts, idx, mat_ids, chunk=256, kinds=False):
    """pt_sweep_hit records as uint32 [n, 8] (t, prim, u, v, cx, cy, cz, material) by brute force: every sweep against every triangle,
    candidates t <= tmax (and finite: +inf stands for no candidate), the smallest t, ties to the lowest triangle index; then closest_on_triangle on the winner at o + d * t.
    kinds: also the winning feature's kind per sweep (NONE for a miss)."""
    s = np.ascontiguousarray(np.asarray(sweeps, np.float32).reshape(-1, 8))
    n = s.shape[0]
    rec = miss_records(n)
    kind_out = np.full(n, NONE, np.int8)
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    if v0.shape[0] == 0 or n == 0:
        return (rec, kind_out) if kinds else rec
    mats = np.asarray(mat_ids, np.uint32)
    ok = castable(s)
    chunk = max(1, min(chunk, (1 << 19) // v0.shape[0] + 1))
    for start in range(0, n, chunk):
        sl = slice(start, min(n, start + chunk))
        o, d = s[sl, 0:3], s[sl, 3:6]
        t, kind = sweep_triangle(o[:, None], d[:, None], s[sl, 6, None], v0[None], e1[None], e2[None])
        with np.errstate(invalid="ignore"):
            cand = (t <= s[sl, 7, None]) & (t < F(np.inf)) & ok[sl, None]
        key = np.where(cand, t, F(np.inf))
        best = key.min(axis=1)
        win = np.argmax(cand & (key == best[:, None]), axis=1)           # the first (lowest) index among the ties
        found = cand.any(axis=1)
        rows = np.arange(win.size)
        tw = t[rows, win]
        with np.errstate(all="ignore"):
            centre = o + d * tw[:, None]
            _, v, w, c = nr.closest_on_triangle(centre, v0[win], e1[win], e2[win])
        out = np.zeros((win.size, 8), np.float32)
        out[:, 0] = tw
        out[:, 2] = v
        out[:, 3] = w
        out[:, 4:7] = c
        out = out.view(np.uint32)
        out[:, 1] = win.astype(np.uint32)
        out[:, 7] = mats[win] & SHADE_MAT_MASK
        sub = rec[sl]
        sub[found] = out[found]
        kind_out[sl] = np.where(found, kind[rows, win], NONE)
    return (rec, kind_out) if kinds else rec


def blocked_of(rec):
    """pt_query_sweep_any's bytes from the records: t >= 0"""
    return (np.asarray(rec, np.uint32)[:, 0].view(np.float32) >= 0).astype(np.uint8)


def impact_f64(sweeps, tri_v0, tri_e1, tri_e2):
    """float64 time of impact of sweep i with triangle i (fp32 inputs, the same statement in double), +inf where there is none"""
    s = np.asarray(sweeps, np.float64).reshape(-1, 8)
    return sweep_triangle(s[:, 0:3], s[:, 3:6], s[:, 6], *(np.asarray(a, np.float64) for a in (tri_v0, tri_e1, tri_e2)))[0]


# ---- sweep sets ------------------------------------------------------------------------------------------------------------------
# Fixed seeds, SET_SIZE sweeps each (n of the caller's on the large scenes).  "camera" and "short" need a view; the rest are made from
# the triangles alone, so a test can regenerate them per scene.
SWEEP_SETS = ("camera", "aimed", "grazing", "inside", "short", "outside", "zero_d", "bad")
SCENE_SETS = ("aimed", "grazing")
SET_SIZE = 1000
CAMERA_RADII = (0.0, 0.001, 0.01, 0.05, 0.25)            # of the scene diagonal
GRAZE = 2.0 ** -12


def _extent(verts, idx):
    """(lo, hi, centre, scale): scale is the scene box's diagonal, or where there is no box or it is a point a thousandth of its distance
    from the origin (1 at the origin)"""
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    used = np.unique(np.asarray(idx, np.uint32))
    if used.size == 0:
        used = np.arange(v.shape[0])
    lo, hi = v[used].min(axis=0), v[used].max(axis=0)
    ext = (hi - lo).astype(np.float64)
    diag = float(np.sqrt((ext * ext).sum()))
    c = 0.5 * (lo.astype(np.float64) + hi)
    if not diag > 0:
        diag = 1e-3 * float(np.abs(c).max()) or 1.0
    return lo, hi, c, diag


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.sqrt((d * d).sum(axis=1, keepdims=True))


def _perp(rng, u):
    """unit vectors perpendicular to the unit vectors u"""
    w = np.cross(u, _unit(rng, u.shape[0]))
    return w / np.sqrt((w * w).sum(axis=1, keepdims=True))


def _pack(o, d, r, tmax):
    s = np.zeros((o.shape[0], 8), np.float32)
    s[:, 0:3], s[:, 3:6], s[:, 6], s[:, 7] = o, d, r, tmax
    return s


def _targets(rng, verts, idx, n):
    """n points on the triangles, float64, and what they are: 0 a centroid, 1 an edge's midpoint, 2 a vertex; the triangles' own edge
    directions at the point (for "grazing") and, for a vertex, the direction into the mesh there.  A scene without triangles aims
    at its vertices."""
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    tri_idx = np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)
    what = rng.choice([0, 1, 1, 2, 2, 2], n)              # a corner is the smallest target: half the set
    if tri_idx.shape[0] == 0:
        p = v[rng.integers(0, v.shape[0], n)]
        return p, what, _unit(rng, n), _unit(rng, n)
    which = rng.integers(0, tri_idx.shape[0], n)
    tri = v[tri_idx[which]]
    k = rng.integers(0, 3, n)
    rows = np.arange(n)
    a, b = tri[rows, k], tri[rows, (k + 1) % 3]
    p = np.where((what == 0)[:, None], tri.mean(axis=1), np.where((what == 1)[:, None], 0.5 * (a + b), a))
    # a vertex target is a corner or a crease where the mesh has one: a position whose triangles' unit normals do not add up to their
    # number.  On a convex corner the vertex is the first point of the mesh a sphere coming down the mean normal meets; inside a flat
    # or finely tessellated face the face comes first from everywhere.
    corners = v[tri_idx.reshape(-1)]
    uniq, inv = np.unique(corners, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    all_tri = v[tri_idx]
    nrm = np.cross(all_tri[:, 1] - all_tri[:, 0], all_tri[:, 2] - all_tri[:, 0])
    nl = np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
    nrm = np.where(nl > 0, nrm / np.where(nl > 0, nl, 1.0), 0.0)
    acc, cnt = np.zeros_like(uniq), np.zeros(uniq.shape[0])
    np.add.at(acc, inv, np.repeat(nrm, 3, axis=0))
    np.add.at(cnt, inv, np.repeat((nl[:, 0] > 0).astype(np.float64), 3))
    sharp = np.flatnonzero(np.sqrt((acc * acc).sum(axis=1)) < 0.95 * cnt)
    pick = sharp[rng.integers(0, sharp.size, n)] if sharp.size else inv[3 * which + k]
    p = np.where((what == 2)[:, None], uniq[pick], p)
    return p, what, b - a, -acc[pick]


def sweep_set(name, verts, idx, camera=None, mat_ids=None, n=SET_SIZE):
    """n sweeps float32 [n, 8] of the named set.  camera: (eye, U, V, W), for "camera" and "short"."""
    lo, hi, c, diag = _extent(verts, idx)
    ext = hi.astype(np.float64) - lo
    if name == "camera":            # the view's rays, each with one of five radii
        import denoise_ref as dr
        rng = np.random.default_rng(1101)
        rays = dr.pixel_rays(97, 61, *camera)[np.sort(rng.permutation(97 * 61)[:n])]
        r = np.asarray(CAMERA_RADII)[rng.integers(0, len(CAMERA_RADII), n)] * diag
        return _pack(rays[:, 0:3], rays[:, 3:6], r, np.inf)
    if name == "aimed":             # at centroids, edges' midpoints and vertices, from nearby in a random direction and passing within the
        rng = np.random.default_rng(1202)       # radius; an eighth start in contact
        p, what, _, inward = _targets(rng, verts, idx, n)
        r = diag * rng.choice([0.002, 0.01, 0.03], n)
        u = _unit(rng, n)
        # a vertex is approached head-on, give or take: from elsewhere a face or an edge of a finely tessellated surface comes first
        il = np.sqrt((inward * inward).sum(axis=1, keepdims=True))
        head_on = inward / np.where(il > 0, il, 1.0) + 0.3 * u
        hl = np.sqrt((head_on * head_on).sum(axis=1, keepdims=True))
        u = np.where((what == 2)[:, None] & (il > 0) & (hl > 1e-3), head_on / np.where(hl > 1e-3, hl, 1.0), u)
        dist = r * rng.uniform(3.0, 30.0, n)
        dist = np.where(rng.random(n) < 0.125, r * rng.uniform(0.0, 0.9, n), dist)
        off = _perp(rng, u) * (r * rng.uniform(0.0, 0.8, n) * np.where(what == 2, 0.1, 1.0))[:, None]
        o = p + off - u * dist[:, None]
        d = u * (diag * rng.uniform(0.01, 1.0, n))[:, None]            # not normalised: t is in units of |d|
        return _pack(o, d, r, np.inf)
    if name == "grazing":           # centre lines that pass a vertex or a point of an edge at r (1 +- 2^-12)
        rng = np.random.default_rng(1303)
        p, what, edge, _ = _targets(rng, verts, idx, n)
        r = diag * rng.choice([0.002, 0.01, 0.03], n)
        u = _unit(rng, n)
        el = np.sqrt((edge * edge).sum(axis=1, keepdims=True))
        along = np.where(el > 0, edge / np.where(el > 0, el, 1.0), _unit(rng, n))
        # at an edge's midpoint the offset is perpendicular to the edge too, so the distance to the edge's line is the offset's length
        w = np.where((what == 1)[:, None], np.cross(u, along), _perp(rng, u))
        wl = np.sqrt((w * w).sum(axis=1, keepdims=True))
        w = np.where(wl > 1e-6, w / np.where(wl > 1e-6, wl, 1.0), _perp(rng, u))
        sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        o = p + w * (r * (1.0 + sign * GRAZE))[:, None] - u * (r * rng.uniform(3.0, 30.0, n))[:, None]
        d = u * (diag * rng.uniform(0.01, 1.0, n))[:, None]
        return _pack(o, d, r, np.inf)
    if name == "inside":            # start overlap: the centre within the radius of a point of a triangle
        rng = np.random.default_rng(1404)
        p = _targets(rng, verts, idx, n)[0]
        r = diag * rng.choice([0.002, 0.02, 0.1], n)
        o = p + _unit(rng, n) * (r * rng.uniform(0.0, 0.95, n))[:, None]
        d = _unit(rng, n) * (diag * rng.uniform(0.01, 1.0, n))[:, None]
        return _pack(o, d, r, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.0, 2.0, n)))
    if name == "short":             # tmax at 0.5, 1 and 2 times the brute force's t (the t itself: the closed end of the interval)
        base = sweep_set("camera", verts, idx, camera, n=n).copy()
        base[:, 6] = np.where(base[:, 6] == 0, F(0.01 * diag), base[:, 6])
        t = sweep_records(base, verts, idx, mat_ids if mat_ids is not None else np.zeros(len(idx) // 3, np.uint32))[:, 0].view(np.float32)
        factor = np.asarray([0.5, 1.0, 2.0], np.float32)[np.arange(n) % 3]
        base[:, 7] = np.where(t >= 0, t * factor, F(1.0))
        return base
    if name == "outside":           # from outside the scene box, towards a point of it and away from it
        rng = np.random.default_rng(1606)
        o = c + _unit(rng, n) * (diag * rng.uniform(1.5, 5.0, n))[:, None]
        target = lo + rng.random((n, 3)) * ext
        d = (target - o) * np.where(np.arange(n) % 4 == 3, -1.0, 1.0)[:, None] * rng.uniform(0.1, 2.0, n)[:, None]
        r = diag * rng.choice([0.0, 0.01, 0.05, 0.25], n)
        return _pack(o, d, r, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.5, 20.0, n)))
    if name == "zero_d":            # d = 0: only the start overlap can answer
        rng = np.random.default_rng(1707)
        p = _targets(rng, verts, idx, n)[0]
        r = diag * rng.choice([0.0, 0.01, 0.05], n)
        o = p + _unit(rng, n) * (diag * 0.05 * rng.uniform(0.0, 2.0, n))[:, None]
        return _pack(o, np.zeros((n, 3)), r, np.where(rng.random(n) < 0.5, np.inf, 1.0))
    if name == "bad":               # every miss before any traversal, one component at a time, on every third sweep of "aimed"
        s = sweep_set("aimed", verts, idx, n=n).copy()
        cases = bad_cases()
        for i in range(1, n, 3):
            k, val, _ = cases[(i // 3) % len(cases)]
            s[i, k] = val
        return s
    raise ValueError(name)


def bad_cases():
    """(component, value, what) of everything that makes a sweep a miss before any traversal"""
    out = []
    for k in range(6):
        for val in (np.nan, np.inf, -np.inf):
            out.append((k, F(val), "%s%s = %s" % ("od"[k // 3], "xyz"[k % 3], val)))
    for val, what in ((np.nan, "NaN"), (np.inf, "+inf"), (-np.inf, "-inf"), (-1.0, "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        out.append((6, F(val), "radius = %s" % what))
    for val, what in ((np.nan, "NaN"), (-np.inf, "-inf"), (-1.0, "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        out.append((7, F(val), "tmax = %s" % what))
    return out


def bad_sweeps(good):
    good = np.asarray(good, np.float32).reshape(8)
    out, why = [], []
    for k, val, what in bad_cases():
        r = good.copy(); r[k] = val
        out.append(r); why.append(what)
    return np.array(out, np.float32), why


# ---- float64 yardsticks ----------------------------------------------------------------------------------------------------------
def line_distance_f64(sweeps, v0, e1, e2, iters=80):
    """float64 closest approach of the centre line's piece [0, tmax] to triangle i, per sweep i: the distance is convex along the line,
    so a ternary search finds its minimum.  An infinite tmax is cut where the line has left the triangle's neighbourhood for good."""
    s = np.asarray(sweeps, np.float64).reshape(-1, 8)
    o, d = s[:, 0:3], s[:, 3:6]
    v0, e1, e2 = (np.asarray(a, np.float64) for a in (v0, e1, e2))
    dd = (d * d).sum(axis=1)
    with np.errstate(all="ignore"):
        far = (np.sqrt(((o - v0) ** 2).sum(axis=1)) + np.sqrt((e1 * e1).sum(axis=1)) + np.sqrt((e2 * e2).sum(axis=1))) / np.sqrt(dd)
    far = np.where(dd > 0, far, 0.0)
    a, b = np.zeros(s.shape[0]), np.minimum(s[:, 7], far)

    def dist(t):
        return nr.closest_f64(o + d * t[:, None], v0, v0 + e1, v0 + e2)[0]
    for _ in range(iters):
        m1, m2 = a + (b - a) / 3.0, b - (b - a) / 3.0
        left = dist(m1) <= dist(m2)
        a, b = np.where(left, a, m1), np.where(left, m2, b)
    return dist(0.5 * (a + b))


def bisect_impact_f64(sweeps, v0, e1, e2, iters=200):
    """float64 time of impact of sweep i with triangle i by bisection on closest_f64(centre(t)) - r, independent of the decomposition:
    the set dist <= r along the line is one interval, so the impact lies between 0 and the closest approach.  +inf for none."""
    s = np.asarray(sweeps, np.float64).reshape(-1, 8)
    o, d, r = s[:, 0:3], s[:, 3:6], s[:, 6]
    v0, e1, e2 = (np.asarray(a, np.float64) for a in (v0, e1, e2))

    def dist(t):
        return nr.closest_f64(o + d * t[:, None], v0, v0 + e1, v0 + e2)[0]
    dd = (d * d).sum(axis=1)
    far = (np.sqrt(((o - v0) ** 2).sum(axis=1)) + np.sqrt((e1 * e1).sum(axis=1)) + np.sqrt((e2 * e2).sum(axis=1))) / np.sqrt(dd)
    a, b = np.zeros(s.shape[0]), far.copy()
    for _ in range(iters):                       # the closest approach
        m1, m2 = a + (b - a) / 3.0, b - (b - a) / 3.0
        left = dist(m1) <= dist(m2)
        a, b = np.where(left, a, m1), np.where(left, m2, b)
    tmin = 0.5 * (a + b)
    hit = dist(tmin) <= r
    start = dist(np.zeros_like(tmin)) <= r
    lo_t, hi_t = np.zeros_like(tmin), tmin.copy()
    for _ in range(iters):                       # dist(lo_t) > r >= dist(hi_t)
        mid = 0.5 * (lo_t + hi_t)
        inside = dist(mid) <= r
        lo_t, hi_t = np.where(inside, lo_t, mid), np.where(inside, mid, hi_t)
    return np.where(start, 0.0, np.where(hit, hi_t, np.inf))
