"""NumPy statement of pt_query_capsule_cast's record (include/acgpt.h states the same definition), the brute force over all triangles
it is held to, the cast sets its tests use and a float64 yardstick that knows nothing of the decomposition.

Every operation is fp32 in the order of csrc/capsule.hip capsule_triangle — sweep_ref's vertex, edge and face forms at p0 and at p1,
the three axis edges, the three side faces, segment_ref's statement for the start overlap, a NaN no candidate — so the GPU's record
equals this one bit for bit.  With float64 arrays the same functions give the same algorithm in double.  The triangle is what the build
stores in a TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0, one fp32 subtraction per component."""
import numpy as np

import nearest_ref as nr
import segment_ref as sg
import sweep_ref as sw

F = np.float32
MISS_PRIM = np.uint32(0xFFFFFFFF)
SHADE_MAT_MASK = nr.SHADE_MAT_MASK
# the group of features that gives a triangle's time of impact
START, P0_VERTEX, P0_EDGE, P0_FACE, P1_VERTEX, P1_EDGE, P1_FACE, AXIS_EDGE, SIDE_FACE, NONE = range(10)
GROUPS = (START, P0_VERTEX, P0_EDGE, P0_FACE, P1_VERTEX, P1_EDGE, P1_FACE, AXIS_EDGE, SIDE_FACE)
GROUP_NAMES = ("start", "vertex at p0", "edge at p0", "face at p0", "vertex at p1", "edge at p1", "face at p1", "axis edge", "side face", "none")

_dot, _cross = sw._dot, sw._cross


def _side_face(m, E, a, d, r, t):
    """the face form on the parallelogram {A - a + u E + v a}: E in the place of e1, a in the place of e2, 0 <= u, v <= 1"""
    n = _cross(E, a)
    nn, s0 = _dot(n, n), _dot(n, m)
    sr = np.where(s0 >= 0, r, -r)
    tf = (sr * np.sqrt(nn) - s0) / _dot(n, d)
    w = m + d * tf[..., None]
    u, v = _dot(_cross(w, a), n) / nn, _dot(_cross(E, w), n) / nn
    take = (tf >= 0) & (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1) & (tf < t)
    return np.where(take, tf, t)


def _group(t_new, t, kind, g):
    return t_new, np.where(t_new < t, g, kind)


def capsule_triangle(p0, p1, d, r, v0, e1, e2):
    """(t, group): the time of impact of capsules {p0 + t d, p1 + t d, r} with triangles {v0, v0 + e1, v0 + e2}, +inf where there is
    none, and which group of features gave it (the first in the statement's order among equal times).  The vectors broadcast against
    each other (last axis xyz), r against their leading axes.  Any float dtype."""
    p0, p1, d, v0, e1, e2 = np.broadcast_arrays(p0, p1, d, v0, e1, e2)
    r = np.broadcast_to(np.asarray(r, p0.dtype), p0.shape[:-1])
    with np.errstate(all="ignore"):
        a = p1 - p0
        dd, rr = _dot(d, d), r * r
        t = np.full(p0.shape[:-1], np.inf, p0.dtype)
        kind = np.full(p0.shape[:-1], NONE, np.int8)
        scratch = np.zeros(p0.shape[:-1], np.int8)
        q1, q2, e3 = v0 + e1, v0 + e2, e2 - e1
        for o, gv, ge, gf in ((p0, P0_VERTEX, P0_EDGE, P0_FACE), (p1, P1_VERTEX, P1_EDGE, P1_FACE)):
            m0, m1, m2 = o - v0, o - q1, o - q2
            for m in (m0, m1, m2):
                t, kind = _group(sw._vertex(m, d, dd, rr, t, scratch)[0], t, kind, gv)
            for m, E in ((m0, e1), (m0, e2), (m1, e3)):
                t, kind = _group(sw._edge(m, E, d, rr, t, scratch)[0], t, kind, ge)
            t, kind = _group(sw._face(m0, e1, e2, d, r, t, scratch)[0], t, kind, gf)
        m0, m1, m2 = p1 - v0, p1 - q1, p1 - q2
        for m in (m0, m1, m2):
            t, kind = _group(sw._edge(m, a, d, rr, t, scratch)[0], t, kind, AXIS_EDGE)
        for m, E in ((m0, e1), (m0, e2), (m1, e3)):
            t, kind = _group(_side_face(m, E, a, d, r, t), t, kind, SIDE_FACE)
        d2 = sg.segment_triangle(p0, p1, v0, e1, e2)[0]
        start = d2 <= rr
        t, kind = np.where(start, p0.dtype.type(0), t), np.where(start, START, kind)
    return t, kind


def castable(casts):
    """False where a cast is a miss before any traversal: a non-finite component of p0, p1, p1 - p0 or d, a radius that is NaN,
    negative or infinite, a NaN or negative tmax.  The twelfth float is not looked at."""
    c = np.asarray(casts, np.float32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        return (np.isfinite(c[:, 0:4]).all(axis=1) & np.isfinite(c[:, 4:7]).all(axis=1) & np.isfinite(c[:, 4:7] - c[:, 0:3]).all(axis=1) &
                np.isfinite(c[:, 8:11]).all(axis=1) & (c[:, 3] >= F(0.0)) & (c[:, 7] >= F(0.0)))


def miss_records(n):
    return nr.miss_records(n)


def capsule_records(casts, verts, idx, mat_ids, chunk=256, kinds=False):
    """pt_capsule_cast_hit records as uint32 [n, 8] (t, prim, s, feature, cx, cy, cz, material) by brute force: every cast against every
    triangle, candidates t <= tmax (and finite: +inf stands for no candidate), the smallest t, ties to the lowest triangle index; then
    segment_ref's statement on the winner for the axis at impact.  kinds: also the winning group per cast (NONE for a miss)."""
    c = np.ascontiguousarray(np.asarray(casts, np.float32).reshape(-1, 12))
    n = c.shape[0]
    rec = miss_records(n)
    kind_out = np.full(n, NONE, np.int8)
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    if v0.shape[0] == 0 or n == 0:
        return (rec, kind_out) if kinds else rec
    mats = np.asarray(mat_ids, np.uint32)
    ok = castable(c)
    chunk = max(1, min(chunk, (1 << 18) // v0.shape[0] + 1))
    for start in range(0, n, chunk):
        sl = slice(start, min(n, start + chunk))
        p0, p1, d = c[sl, 0:3], c[sl, 4:7], c[sl, 8:11]
        t, kind = capsule_triangle(p0[:, None], p1[:, None], d[:, None], c[sl, 3, None], v0[None], e1[None], e2[None])
        with np.errstate(invalid="ignore"):
            cand = (t <= c[sl, 7, None]) & (t < F(np.inf)) & ok[sl, None]
        key = np.where(cand, t, F(np.inf))
        best = key.min(axis=1)
        win = np.argmax(cand & (key == best[:, None]), axis=1)           # the first (lowest) index among the ties
        found = cand.any(axis=1)
        rows = np.arange(win.size)
        tw = t[rows, win]
        with np.errstate(all="ignore"):
            move = d * tw[:, None]
            _, s, feat, cp = sg.segment_triangle(p0 + move, p1 + move, v0[win], e1[win], e2[win])
        out = np.zeros((win.size, 8), np.float32)
        out[:, 0] = tw
        out[:, 2] = s
        out[:, 3] = feat.astype(np.float32)
        out[:, 4:7] = cp
        out = out.view(np.uint32)
        out[:, 1] = win.astype(np.uint32)
        out[:, 7] = mats[win] & SHADE_MAT_MASK
        sub = rec[sl]
        sub[found] = out[found]
        kind_out[sl] = np.where(found, kind[rows, win], NONE)
    return (rec, kind_out) if kinds else rec


def blocked_of(rec):
    """pt_query_capsule_cast_any's bytes from the records: t >= 0"""
    return (np.asarray(rec, np.uint32)[:, 0].view(np.float32) >= 0).astype(np.uint8)


def impact_f64(casts, tri_v0, tri_e1, tri_e2):
    """float64 (t, group) of cast i with triangle i (fp32 inputs, the same statement in double), +inf where there is none"""
    c = np.asarray(casts, np.float64).reshape(-1, 12)
    return capsule_triangle(c[:, 0:3], c[:, 4:7], c[:, 8:11], c[:, 3], *(np.asarray(a, np.float64) for a in (tri_v0, tri_e1, tri_e2)))


def bisect_impact_f64(casts, v0, e1, e2, iters=200):
    """(t, resolution): float64 time of impact of cast i with triangle i by bisection on segment_f64(axis(t), triangle) - r,
    independent of the decomposition: the distance between the moving axis and the triangle is convex in t, so distance <= r holds on
    one interval and the impact lies between 0 and the closest approach.  +inf for none.  resolution: the width of the last bracket
    plus what an ulp of the distance is worth in t where the bracket closed."""
    c = np.asarray(casts, np.float64).reshape(-1, 12)
    p0, p1, d, r = c[:, 0:3], c[:, 4:7], c[:, 8:11], c[:, 3]
    v0, e1, e2 = (np.asarray(a, np.float64) for a in (v0, e1, e2))

    def dist(t):
        move = d * t[:, None]
        return sg.segment_f64(p0 + move, p1 + move, v0, v0 + e1, v0 + e2)[0]
    dd = (d * d).sum(axis=1)
    with np.errstate(all="ignore"):
        far = (np.sqrt(((p0 - v0) ** 2).sum(axis=1)) + np.sqrt(((p1 - v0) ** 2).sum(axis=1)) + np.sqrt((e1 * e1).sum(axis=1)) + np.sqrt((e2 * e2).sum(axis=1))) / np.sqrt(dd)
    far = np.where(dd > 0, far, 0.0)
    a, b = np.zeros(c.shape[0]), far.copy()
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
    t = np.where(start, 0.0, np.where(hit, hi_t, np.inf))
    return t, hi_t - lo_t


def axis_distance_f64(casts, v0, e1, e2, iters=120):
    """float64 closest approach of the moving axis over [0, tmax] to triangle i, per cast i (the distance is convex in t)"""
    c = np.asarray(casts, np.float64).reshape(-1, 12)
    p0, p1, d = c[:, 0:3], c[:, 4:7], c[:, 8:11]
    v0, e1, e2 = (np.asarray(a, np.float64) for a in (v0, e1, e2))
    dd = (d * d).sum(axis=1)
    with np.errstate(all="ignore"):
        far = (np.sqrt(((p0 - v0) ** 2).sum(axis=1)) + np.sqrt(((p1 - v0) ** 2).sum(axis=1)) + np.sqrt((e1 * e1).sum(axis=1)) + np.sqrt((e2 * e2).sum(axis=1))) / np.sqrt(dd)
    far = np.where(dd > 0, far, 0.0)
    a, b = np.zeros(c.shape[0]), np.minimum(c[:, 7], far)

    def dist(t):
        move = d * t[:, None]
        return sg.segment_f64(p0 + move, p1 + move, v0, v0 + e1, v0 + e2)[0]
    for _ in range(iters):
        m1, m2 = a + (b - a) / 3.0, b - (b - a) / 3.0
        left = dist(m1) <= dist(m2)
        a, b = np.where(left, a, m1), np.where(left, m2, b)
    return dist(0.5 * (a + b))


def sampled_spheres(casts, verts, idx, mat_ids, k=5):
    """What a caller without the capsule cast does: k spheres along the axis through sweep_ref's brute force, the earliest time of
    impact (float32, -1 where no sphere touches anything)"""
    c = np.asarray(casts, np.float32).reshape(-1, 12)
    best = np.full(c.shape[0], np.inf, np.float32)
    for j in range(k):
        o = c[:, 0:3] + (c[:, 4:7] - c[:, 0:3]) * F(j / (k - 1.0))
        t = sw.sweep_records(sw._pack(o, c[:, 8:11], c[:, 3], c[:, 7]), verts, idx, mat_ids)[:, 0].view(np.float32)
        best = np.where((t >= 0) & (t < best), t, best)
    return np.where(np.isfinite(best), best, F(-1.0)).astype(np.float32)


# ---- cast sets -------------------------------------------------------------------------------------------------------------------
# Fixed seeds, SET_SIZE casts each (n of the caller's on other scenes).  "aimed" and "links" are made from the triangles and the scene
# box alone and hold on any scene; the others are meant for the Cornell fixtures.
CAST_SETS = ("aimed", "grazing", "upright", "links", "parallel", "along", "point", "inside", "short", "outside", "zero_d", "bad")
SCENE_SETS = ("aimed", "links")
COVERAGE_SETS = ("aimed", "grazing", "upright", "links")
SET_SIZE = 1000
GRAZE = 2.0 ** -12
UP = np.array([0.0, 1.0, 0.0])


def pack(p0, p1, d, r, tmax, twelfth=0.0):
    c = np.zeros((np.asarray(p0).shape[0], 12), np.float32)
    c[:, 0:3], c[:, 3], c[:, 4:7], c[:, 7], c[:, 8:11], c[:, 11] = p0, r, p1, tmax, d, twelfth
    return c


def from_sweeps(sweeps):
    """pt_query_sweep records {o, d, r, tmax} as capsule casts with p1 = p0"""
    s = np.asarray(sweeps, np.float32).reshape(-1, 8)
    return pack(s[:, 0:3], s[:, 0:3], s[:, 3:6], s[:, 6], s[:, 7])


def _triangles(rng, verts, idx, n):
    """n random triangles of the scene [n, 3, 3] float64 and their unit normals (0 for a triangle without area)"""
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    tri_idx = np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)
    tri = v[tri_idx[rng.integers(0, tri_idx.shape[0], n)]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nl = np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
    return tri, np.where(nl > 0, nrm / np.where(nl > 0, nl, 1.0), 0.0)


def _norm(w, fallback):
    wl = np.sqrt((w * w).sum(axis=1, keepdims=True))
    return np.where(wl > 1e-9, w / np.where(wl > 1e-9, wl, 1.0), fallback)


def cast_set(name, verts, idx, camera=None, mat_ids=None, n=SET_SIZE):
    """n casts float32 [n, 12] of the named set"""
    lo, hi, c, diag = sw._extent(verts, idx)
    ext = hi.astype(np.float64) - lo
    _unit, _perp = sw._unit, sw._perp
    if name == "aimed":             # at centroids, edges' midpoints and corners as sweep_ref's set, an end or the side of the capsule
        rng = np.random.default_rng(2202)       # leading and passing the target within the radius; an eighth start in contact
        p, what, _, inward = sw._targets(rng, verts, idx, n)
        r = diag * rng.choice([0.002, 0.01, 0.03], n)
        u = _unit(rng, n)
        il = np.sqrt((inward * inward).sum(axis=1, keepdims=True))
        head_on = inward / np.where(il > 0, il, 1.0) + 0.15 * u
        hl = np.sqrt((head_on * head_on).sum(axis=1, keepdims=True))
        u = np.where((what == 2)[:, None] & (il > 0) & (hl > 1e-3), head_on / np.where(hl > 1e-3, hl, 1.0), u)
        dist = r * rng.uniform(3.0, 30.0, n)
        dist = np.where(rng.random(n) < 0.125, r * rng.uniform(0.0, 0.9, n), dist)
        off = _perp(rng, u) * (r * rng.uniform(0.0, 0.8, n) * np.where(what == 2, 0.1, 1.0))[:, None]
        # p0 leads and is aimed at the target, p1 leads, or the cylinder's side leads with the target's foot inside the axis: a third
        # each, but for a corner, which only an end that comes down its mean normal meets first: nine in twenty each, a tenth the side
        lead = np.where(what == 2, rng.choice([0, 1, 2], n, p=[0.47, 0.47, 0.06]), rng.integers(0, 3, n))
        tilt = np.where((what == 2)[:, None], 0.1, 0.4) * _unit(rng, n)
        w = _norm(np.where((lead == 0)[:, None], -u + tilt, np.where((lead == 1)[:, None], u + tilt, _perp(rng, u) + 0.25 * tilt)), _perp(rng, u))
        half = r * rng.uniform(1.0, 3.0, n)
        shift = np.where(lead == 0, 1.0, np.where(lead == 1, -1.0, rng.uniform(-0.8, 0.8, n)))
        m = p + off - u * dist[:, None] + w * (half * shift)[:, None]
        d = u * (diag * rng.uniform(0.01, 1.0, n))[:, None]            # not normalised: t is in units of |d|
        return pack(m - w * half[:, None], m + w * half[:, None], d, r, np.inf, np.where(np.arange(n) % 2 == 0, np.nan, 0.0))
    if name == "grazing":           # the side of the cylinder passing a vertex or a point of an edge at r (1 +- 2^-12): the axis is
        rng = np.random.default_rng(2303)       # perpendicular to the motion and to the offset, the target between two sample spheres
        p, what, edge, _ = sw._targets(rng, verts, idx, n)
        r = diag * rng.choice([0.002, 0.01, 0.03], n)
        u = _unit(rng, n)
        el = np.sqrt((edge * edge).sum(axis=1, keepdims=True))
        along = np.where(el > 0, edge / np.where(el > 0, el, 1.0), _unit(rng, n))
        off = np.where((what == 1)[:, None], np.cross(u, along), _perp(rng, u))
        off = _norm(off, _perp(rng, u))
        w = _norm(np.cross(u, off) + 0.3 * u * rng.uniform(-1.0, 1.0, (n, 1)), _perp(rng, u))          # perpendicular to the offset: the distance to the axis' line is the offset's length
        half = r * rng.uniform(4.0, 8.0, n)
        sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        # the foot of the target on the axis at an odd eighth of its length: midway between two of five sample spheres
        foot = half * rng.choice([-0.75, -0.25, 0.25, 0.75], n)
        m = p + off * (r * (1.0 + sign * GRAZE))[:, None] - u * (r * rng.uniform(3.0, 30.0, n))[:, None] - w * foot[:, None]
        d = u * (diag * rng.uniform(0.01, 1.0, n))[:, None]
        return pack(m - w * half[:, None], m + w * half[:, None], d, r, np.inf)
    if name == "upright":           # the controller's case: the axis along the scene's up direction, 2 to 4 radii long, moving near-horizontally
        rng = np.random.default_rng(2404)
        r = diag * rng.choice([0.005, 0.01, 0.02], n)
        length = r * rng.uniform(2.0, 4.0, n)
        foot = lo + np.array([0.08, 0.0, 0.08]) * ext + rng.random((n, 3)) * ext * np.array([0.84, 0.0, 0.84])
        # standing on the floor (a hair above it), a quarter stepping from higher up
        foot[:, 1] = lo[1] + r * (1.0 + 2.0 ** -10) + np.where(rng.random(n) < 0.25, rng.uniform(0.0, 0.6, n) * ext[1], 0.0)
        heading = rng.uniform(0.0, 2.0 * np.pi, n)
        d = np.stack([np.cos(heading), rng.uniform(-0.05, 0.05, n), np.sin(heading)], axis=1) * (diag * rng.uniform(0.05, 0.5, n))[:, None]
        return pack(foot, foot + UP * length[:, None], d, r, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.2, 3.0, n)))
    if name == "links":             # robot links: the axis 20 to 50 % of the scene's diagonal, diagonal to the walls
        rng = np.random.default_rng(2505)
        r = diag * rng.choice([0.0, 0.004, 0.01], n)
        w = _norm(np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0) + 0.3 * _unit(rng, n), _unit(rng, n))
        half = 0.5 * diag * rng.uniform(0.2, 0.5, n)
        m = lo + (0.3 + 0.4 * rng.random((n, 3))) * ext
        d = _unit(rng, n) * (diag * rng.uniform(0.05, 0.5, n))[:, None]
        return pack(m - w * half[:, None], m + w * half[:, None], d, r, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.2, 3.0, n)))
    if name == "parallel":          # the axis parallel to an edge of a triangle (half) or lying in its plane, coming down on it
        rng = np.random.default_rng(2606)
        tri, nrm = _triangles(rng, verts, idx, n)
        k = rng.integers(0, 3, n)
        rows = np.arange(n)
        edge = tri[rows, (k + 1) % 3] - tri[rows, k]
        other = tri[rows, (k + 2) % 3] - tri[rows, k]
        in_plane = edge * rng.uniform(-1.0, 1.0, (n, 1)) + other * rng.uniform(-1.0, 1.0, (n, 1))
        w = _norm(np.where((rows % 2 == 0)[:, None], edge, in_plane), _unit(rng, n))
        r = diag * rng.choice([0.0, 0.01, 0.03], n)
        b = rng.random((n, 2)); fold = b.sum(axis=1) > 1.0; b[fold] = 1.0 - b[fold]
        target = tri[:, 0] + b[:, 0:1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:2] * (tri[:, 2] - tri[:, 0])
        side = np.where(rng.random(n) < 0.5, 1.0, -1.0)[:, None]
        height = r + diag * rng.uniform(0.01, 0.2, n)
        half = diag * rng.uniform(0.01, 0.15, n)
        m = target + nrm * side * height[:, None]
        u = _norm(-nrm * side + 0.3 * _unit(rng, n), _unit(rng, n))
        # a quarter slide along the plane at a fixed height: the motion in the plane too
        slide = rows % 4 == 1
        u = np.where(slide[:, None], _norm(in_plane, _unit(rng, n)), u)
        d = u * (diag * rng.uniform(0.05, 0.5, n))[:, None]
        return pack(m - w * half[:, None], m + w * half[:, None], d, r, np.inf)
    if name == "along":             # d parallel to a: the capsule moves along its own axis, either end first
        rng = np.random.default_rng(2707)
        p, what, _, _ = sw._targets(rng, verts, idx, n)
        r = diag * rng.choice([0.0, 0.002, 0.01, 0.03], n)
        u = _unit(rng, n)
        half = r * rng.uniform(1.0, 6.0, n) + diag * 0.002
        m = p + _perp(rng, u) * (r * rng.uniform(0.0, 1.5, n))[:, None] - u * (half + r * rng.uniform(3.0, 30.0, n))[:, None]
        cst = pack(m - u * half[:, None], m + u * half[:, None], 0.0, r, np.inf)
        scale = (rng.uniform(0.5, 5.0, n) * np.where(rng.random(n) < 0.2, -1.0, 1.0)).astype(np.float32)
        cst[:, 8:11] = (cst[:, 4:7] - cst[:, 0:3]) * scale[:, None]            # fp32: parallel as far as the format goes
        return cst
    if name == "point":             # p1 = p0: sweep_ref's "aimed" spheres
        return from_sweeps(sw.sweep_set("aimed", verts, idx, n=n))
    if name == "inside":            # start overlaps; a quarter with the axis piercing a triangle at more than r from both ends
        rng = np.random.default_rng(2808)
        p = sw._targets(rng, verts, idx, n)[0]
        tri, nrm = _triangles(rng, verts, idx, n)
        r = diag * rng.choice([0.002, 0.02, 0.1], n)
        w = _unit(rng, n)
        half = r * rng.uniform(0.5, 3.0, n)
        m = p + _unit(rng, n) * (r * rng.uniform(0.0, 0.95, n))[:, None] + w * (half * rng.uniform(-1.0, 1.0, n))[:, None]
        p0, p1 = m - w * half[:, None], m + w * half[:, None]
        pierce = np.arange(n) % 4 == 0
        wp = _norm(nrm + 0.5 * _unit(rng, n), _unit(rng, n))
        cen = tri.mean(axis=1)
        p0 = np.where(pierce[:, None], cen - wp * (r * rng.uniform(3.0, 6.0, n))[:, None], p0)
        p1 = np.where(pierce[:, None], cen + wp * (r * rng.uniform(3.0, 6.0, n))[:, None], p1)
        d = _unit(rng, n) * (diag * rng.uniform(0.01, 1.0, n))[:, None]
        return pack(p0, p1, d, r, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.0, 2.0, n)))
    if name == "short":             # tmax at 0.5, 1 and 2 times the brute force's t (the t itself: the closed end of the interval)
        base = cast_set("aimed", verts, idx, n=n).copy()
        t = capsule_records(base, verts, idx, mat_ids if mat_ids is not None else np.zeros(len(idx) // 3, np.uint32))[:, 0].view(np.float32)
        factor = np.asarray([0.5, 1.0, 2.0], np.float32)[np.arange(n) % 3]
        base[:, 7] = np.where(t >= 0, t * factor, F(1.0))
        return base
    if name == "outside":           # from outside the scene box, towards a point of it and away from it
        rng = np.random.default_rng(3010)
        m = c + _unit(rng, n) * (diag * rng.uniform(1.5, 5.0, n))[:, None]
        target = lo + rng.random((n, 3)) * ext
        d = (target - m) * np.where(np.arange(n) % 4 == 3, -1.0, 1.0)[:, None] * rng.uniform(0.1, 2.0, n)[:, None]
        r = diag * rng.choice([0.0, 0.01, 0.05, 0.25], n)
        w = _unit(rng, n) * (diag * rng.uniform(0.01, 0.2, n))[:, None]
        return pack(m - w, m + w, d, r, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.5, 20.0, n)))
    if name == "zero_d":            # d = 0: only the start overlap can answer
        rng = np.random.default_rng(3111)
        p = sw._targets(rng, verts, idx, n)[0]
        r = diag * rng.choice([0.0, 0.01, 0.05], n)
        m = p + _unit(rng, n) * (diag * 0.05 * rng.uniform(0.0, 2.0, n))[:, None]
        w = _unit(rng, n) * (diag * rng.uniform(0.0, 0.05, n))[:, None]
        return pack(m - w, m + w, np.zeros((n, 3)), r, np.where(rng.random(n) < 0.5, np.inf, 1.0))
    if name == "bad":               # every miss before any traversal, one component at a time, on every third cast of "aimed"
        cst = cast_set("aimed", verts, idx, n=n).copy()
        cases = bad_cases()
        for i in range(1, n, 3):
            for k, val in cases[(i // 3) % len(cases)][0]:
                cst[i, k] = val
        return cst
    raise ValueError(name)


def bad_cases():
    """(((component, value), ...), what) of everything that makes a cast a miss before any traversal"""
    out = []
    for k, nm in ((0, "p0"), (4, "p1"), (8, "d")):
        for j in range(3):
            for val in (np.nan, np.inf, -np.inf):
                out.append((((k + j, F(val)),), "%s.%s = %s" % (nm, "xyz"[j], val)))
    out.append((((0, F(3e38)), (4, F(-3e38))), "finite ends whose difference overflows"))
    for val, what in ((np.nan, "NaN"), (np.inf, "+inf"), (-np.inf, "-inf"), (-1.0, "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        out.append((((3, F(val)),), "radius = %s" % what))
    for val, what in ((np.nan, "NaN"), (-np.inf, "-inf"), (-1.0, "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        out.append((((7, F(val)),), "tmax = %s" % what))
    return out


def bad_casts(good):
    good = np.asarray(good, np.float32).reshape(12)
    out, why = [], []
    for sets, what in bad_cases():
        r = good.copy()
        for k, val in sets:
            r[k] = val
        out.append(r); why.append(what)
    return np.array(out, np.float32), why


def distance_at_f64(casts, v0, e1, e2, t):
    """float64 distance of cast i's axis at time t[i] from triangle i"""
    c = np.asarray(casts, np.float64).reshape(-1, 12)
    v0, e1, e2 = (np.asarray(a, np.float64) for a in (v0, e1, e2))
    move = c[:, 8:11] * np.asarray(t, np.float64)[:, None]
    return sg.segment_f64(c[:, 0:3] + move, c[:, 4:7] + move, v0, v0 + e1, v0 + e2)[0]
