"""NumPy statement of pt_query_triangle_cast's record (include/acgpt.h states the same definition), the brute force over all triangles
it is held to, the posed reduction of pt_query_poses_cast and the cast sets their tests use.

Every operation is fp32 in the order of csrc/tricast_device.h cast_pair — plain multiplies, adds and subtractions, IEEE divisions, the 16
features as masks, a NaN no candidate — so the GPU's record equals this one bit for bit.  With float64 arrays the same functions give
the same algorithm in double.  The scene triangle is what the build stores in a TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0, one fp32
subtraction per component; the query triangle is its three vertices a0, a1, a2 and the motion d.  Feature 15 is tritri_ref's test."""
import numpy as np

import nearest_ref as nr
import poses_ref as pr
import sweep_ref as sw
import tritri_ref as tt

F = np.float32
MISS = 0xFFFFFFFF
SHADE_MAT_MASK = nr.SHADE_MAT_MASK
START = 15                      # the feature of a start overlap
NONE = 16                       # no candidate
EPS_REL = 2.0 ** -16


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _fmin3(a, b, c):
    return np.fmin(np.fmin(a, b), c)


def _fmax3(a, b, c):
    return np.fmax(np.fmax(a, b), c)


def _signed(det, *rest):
    neg = det < 0
    return [np.where(neg, -x, x) for x in (det,) + rest]


def _ray(o, r, p, k1, k2):
    """(accepted, t) of the line o + t r against the triangle {p, p + k1, p + k2}: the crossing test without an upper end"""
    pv = _cross(r, k2)
    det = _dot(k1, pv)
    tv = o - p
    U = _dot(tv, pv)
    qv = _cross(tv, k1)
    V = _dot(r, qv)
    T = _dot(k2, qv)
    det, U, V, T = _signed(det, U, V, T)
    acc = (det > 0) & (U >= 0) & (V >= 0) & (U + V <= det) & (T >= 0)
    return acc, T / det + det.dtype.type(0)


def _edges(P, D, A, E, d):
    """(accepted, t, c) of the segment {P, D} moving along d against the segment {A, E}"""
    n = _cross(D, E)
    det = _dot(d, n)
    w = A - P
    T = _dot(w, n)
    S = _dot(d, _cross(w, E))
    G = _dot(d, _cross(w, D))
    det, T, S, G = _signed(det, T, S, G)
    acc = (det > 0) & (S >= 0) & (S <= det) & (G >= 0) & (G <= det) & (T >= 0)
    return acc, T / det + det.dtype.type(0), A + E * (G / det)[..., None]


def _inside(c, lo, hi, eps):
    return ((c >= lo - eps[..., None]) & (c <= hi + eps[..., None])).all(axis=-1)


def cast_pair(a0, a1, a2, d, v0, e1, e2):
    """(t, feature, c): the time of impact of triangles {a0, a1, a2} translating along d with triangles {v0, v0 + e1, v0 + e2}, +inf
    and NONE where there is none; the feature that gave it and the contact point.  No tmax here: the caller's candidates are t <= tmax.
    The arrays broadcast against each other (last axis xyz).  Any float dtype."""
    a0, a1, a2, d, v0, e1, e2 = np.broadcast_arrays(a0, a1, a2, d, v0, e1, e2)
    dt = a0.dtype.type
    with np.errstate(all="ignore"):
        f1, f2, g = a1 - a0, a2 - a0, a2 - a1
        w1, w2, h = v0 + e1, v0 + e2, e2 - e1
        qlo, qhi = _fmin3(a0, a1, a2), _fmax3(a0, a1, a2)
        slo, shi = _fmin3(v0, w1, w2), _fmax3(v0, w1, w2)
        big_s = np.fmax(np.abs(slo), np.abs(shi)).max(axis=-1)
        big_q = np.fmax(np.abs(qlo), np.abs(qhi)).max(axis=-1)
        eps = dt(EPS_REL) * (big_s + big_q)
        t = np.full(a0.shape[:-1], np.inf, a0.dtype)
        feature = np.full(a0.shape[:-1], NONE, np.int8)
        c = np.zeros(a0.shape, a0.dtype)

        def lower(k, acc, tk, ck, guard):
            nonlocal t, feature, c
            take = acc & guard & (tk < t)
            t = np.where(take, tk, t)
            feature = np.where(take, np.int8(k), feature)
            c = np.where(take[..., None], ck, c)

        for i, a in enumerate((a0, a1, a2)):
            acc, tk = _ray(a, d, v0, e1, e2)
            ck = a + d * tk[..., None]
            lower(i, acc, tk, ck, _inside(ck, slo, shi, eps))
        for j, b in enumerate((v0, w1, w2)):
            acc, tk = _ray(b, -d, a0, f1, f2)
            lower(3 + j, acc, tk, b, _inside(b - d * tk[..., None], qlo, qhi, eps))
        for i, (P, D) in enumerate(((a0, f1), (a0, f2), (a1, g))):
            for j, (A, E) in enumerate(((v0, e1), (v0, e2), (w1, h))):
                acc, tk, ck = _edges(P, D, A, E, d)
                lower(6 + 3 * i + j, acc, tk, ck, _inside(ck - d * tk[..., None], qlo, qhi, eps))
        start = tt.tri_tri_intersect(a0, a1, a2, v0, e1, e2)
        t = np.where(start, dt(0), t)
        feature = np.where(start, np.int8(START), feature)
        c = np.where(start[..., None], dt(0), c)
    return t, feature, c


def castable(casts):
    """False where a cast is a miss before any traversal: a non-finite coordinate of the triangle or of d, a non-finite difference of
    two vertices, a NaN or negative tmax"""
    s = np.asarray(casts, np.float32).reshape(-1, 16)
    a0, a1, a2, d = s[:, 0:3], s[:, 4:7], s[:, 8:11], s[:, 12:15]
    with np.errstate(all="ignore"):
        fin = np.isfinite(a0) & np.isfinite(a1) & np.isfinite(a2) & np.isfinite(d) & np.isfinite(a1 - a0) & np.isfinite(a2 - a0) & np.isfinite(a2 - a1)
        return fin.all(axis=1) & (s[:, 3] >= F(0.0))


def miss_records(n, query_triangle=0):
    rec = np.zeros((n, 8), np.uint32)
    rec[:, 0] = np.array([-1.0], np.float32).view(np.uint32)[0]
    rec[:, 1] = MISS
    rec[:, 3] = query_triangle
    rec[:, 7] = MISS
    return rec


def cast_records(casts, verts, idx, mat_ids, chunk=256, dtype=np.float32):
    """pt_triangle_cast_hit records as uint32 [n, 8] (t, prim, feature, query_triangle = 0, cx, cy, cz, material) by brute force: every
    cast against every triangle, candidates t <= tmax (and finite: +inf stands for no candidate), the smallest t, ties to the lowest
    triangle index.  dtype float64: the same statement in double on the fp32 inputs, the record rounded to fp32 at the end."""
    s = np.ascontiguousarray(np.asarray(casts, np.float32).reshape(-1, 16))
    n = s.shape[0]
    rec = miss_records(n)
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    if v0.shape[0] == 0 or n == 0:
        return rec
    v0, e1, e2 = (a.astype(dtype) for a in (v0, e1, e2))
    mats = np.asarray(mat_ids, np.uint32)
    ok = castable(s)
    chunk = max(1, min(chunk, (1 << 17) // v0.shape[0] + 1))
    for start in range(0, n, chunk):
        sl = slice(start, min(n, start + chunk))
        q = s[sl].astype(dtype)
        t, feature, c = cast_pair(q[:, None, 0:3], q[:, None, 4:7], q[:, None, 8:11], q[:, None, 12:15], v0[None], e1[None], e2[None])
        with np.errstate(invalid="ignore"):
            cand = (t <= q[:, 3, None]) & (t < np.inf) & ok[sl, None]
        key = np.where(cand, t, np.inf)
        best = key.min(axis=1)
        win = np.argmax(cand & (key == best[:, None]), axis=1)           # the first (lowest) index among the ties
        found = cand.any(axis=1)
        rows = np.arange(win.size)
        out = np.zeros((win.size, 8), np.float32)
        out[:, 0] = t[rows, win]
        out[:, 2] = feature[rows, win]
        out[:, 4:7] = c[rows, win]
        out = out.view(np.uint32)
        out[:, 1] = win.astype(np.uint32)
        out[:, 7] = mats[win] & SHADE_MAT_MASK
        sub = rec[sl]
        sub[found] = out[found]
    return rec


def blocked_of(rec):
    """pt_query_triangle_cast_any's bytes from the records: t >= 0"""
    return (np.asarray(rec, np.uint32)[:, 0].view(np.float32) >= 0).astype(np.uint8)


def columns(rec):
    rec = np.asarray(rec, np.uint32)
    return {"t": rec[:, 0].view(np.float32), "prim": rec[:, 1], "feature": rec[:, 2].view(np.float32), "query_triangle": rec[:, 3],
            "point": rec[:, 4:7].view(np.float32), "material": rec[:, 7]}


# ---- the posed call ----------------------------------------------------------------------------------------------------------------
def posed_casts(poses, motions, records):
    """(P * T, 16) casts, pose-major: pt_pose_triangles' records with motions[p] behind each"""
    posed = pr.transform(poses, records)
    P, T = posed.shape[:2]
    m = np.asarray(motions, np.float32).reshape(P, 4)
    s = np.zeros((P, T, 16), np.float32)
    s[:, :, 0:12] = posed
    s[:, :, 3] = m[:, None, 3]
    s[:, :, 12:15] = m[:, None, 0:3]
    return s.reshape(P * T, 16)


def reduce_casts(rec, P):
    """pt_query_poses_cast's records from the per-triangle records of P * T posed triangles (pose-major): the smallest t, ties to the
    lowest mesh triangle, its index in query_triangle; the miss record carries 0xFFFFFFFF there"""
    rec = np.asarray(rec, np.uint32).reshape(P, -1, 8)
    out = miss_records(P, MISS)
    t = rec[:, :, 0].view(np.float32)
    for p in range(P):
        c = np.flatnonzero(t[p] >= 0)
        if c.size:
            k = c[np.lexsort((c, t[p, c]))[0]]
            out[p] = rec[p, k]
            out[p, 3] = k
    return out


def poses_cast(poses, motions, records, verts, idx, mat_ids):
    P = np.asarray(poses, np.float32).reshape(-1, 12).shape[0]
    return reduce_casts(cast_records(posed_casts(poses, motions, records), verts, idx, mat_ids), P)


def icosphere(level=0, radius=1.0):
    """(vertices float32 [V, 3], indices int64 [T, 3]): an icosahedron (20 triangles), each level splitting every triangle in four"""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.sqrt(1.0 + g * g) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.sqrt((p * p).sum()))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int64)


# ---- cast sets ---------------------------------------------------------------------------------------------------------------------
# Fixed seeds, SET_SIZE casts each.  All are made from the triangles alone, so a test can regenerate them per scene.
CAST_SETS = ("aimed", "links", "grazing", "overlap", "short", "outside", "zero_d", "degenerate", "coplanar", "bad")
SCENE_SETS = ("aimed", "grazing")
SET_SIZE = 1000
GRAZE = 2.0 ** -12


def pack(tri, d, tmax):
    """(n, 16) float32 casts of (n, 3, 3) vertices, (n, 3) motions and tmax"""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    s = np.zeros((tri.shape[0], 16), np.float32)
    with np.errstate(over="ignore"):
        s[:, 0:3], s[:, 4:7], s[:, 8:11] = tri[:, 0], tri[:, 1], tri[:, 2]
        s[:, 12:15] = d
        s[:, 3] = tmax
    return s


def triangles_of(casts):
    """(n, 12) float32 triangle records {a0, 0 | a1, 0 | a2, 0} of the casts"""
    r = np.asarray(casts, np.float32).reshape(-1, 16)[:, 0:12].copy()
    r[:, 3] = 0
    return r


def moved(casts, t):
    """(n, 3, 3) float64: the casts' triangles translated by d t"""
    s = np.asarray(casts, np.float64).reshape(-1, 16)
    tri = np.stack([s[:, 0:3], s[:, 4:7], s[:, 8:11]], axis=1)
    return tri + (s[:, 12:15] * np.asarray(t, np.float64)[:, None])[:, None, :]


def _shape(rng, n, size):
    """(n, 3, 3) float64 offsets of a random triangle's vertices from its centroid, each within `size` of it"""
    off = rng.normal(size=(n, 3, 3))
    off -= off.mean(axis=1, keepdims=True)
    off /= np.sqrt((off * off).sum(axis=2)).max(axis=1)[:, None, None]
    return off * np.asarray(size)[:, None, None]


def cast_set(name, verts, idx, mat_ids=None, n=SET_SIZE):
    """n casts float32 [n, 16] of the named set"""
    lo, hi, c, diag = sw._extent(verts, idx)
    ext = hi.astype(np.float64) - lo
    mats = mat_ids if mat_ids is not None else np.zeros(len(idx) // 3, np.uint32)
    if name == "aimed":             # triangles of 1 to 5 % of the diagonal, aimed at centroids, edges' midpoints and corners from nearby
        rng = np.random.default_rng(3701)
        p, what, _, inward = sw._targets(rng, verts, idx, n)
        size = diag * rng.uniform(0.01, 0.05, n)
        u = sw._unit(rng, n)
        il = np.sqrt((inward * inward).sum(axis=1, keepdims=True))
        head_on = inward / np.where(il > 0, il, 1.0) + 0.3 * u
        hl = np.sqrt((head_on * head_on).sum(axis=1, keepdims=True))
        u = np.where((what == 2)[:, None] & (il > 0) & (hl > 1e-3), head_on / np.where(hl > 1e-3, hl, 1.0), u)
        off = sw._perp(rng, u) * (size * rng.uniform(0.0, 0.3, n))[:, None]
        centre = p + off - u * (size * rng.uniform(1.5, 20.0, n))[:, None]
        d = u * (diag * rng.uniform(0.01, 1.0, n))[:, None]             # not normalised: t is in units of |d|
        return pack(centre[:, None, :] + _shape(rng, n, size), d, np.inf)
    if name == "links":             # a posed icosphere's triangles moving at the walls and blocks
        rng = np.random.default_rng(3702)
        v, f = icosphere(0, 0.04 * diag)
        T = f.shape[0]
        P = (n + T - 1) // T
        rot = pr._rotations(rng, P)
        centre = lo + (0.2 + 0.6 * rng.random((P, 3))) * ext
        poses = pr.as_poses(pr._rigid(rot, centre))
        target = sw._targets(rng, verts, idx, P)[0]
        motions = np.zeros((P, 4), np.float32)
        motions[:, 0:3] = (target - centre) * rng.uniform(0.5, 2.0, (P, 1))
        motions[:, 3] = np.where(rng.random(P) < 0.5, np.inf, rng.uniform(0.2, 2.0, P))
        return posed_casts(poses, motions, pr.records_of(v, f))[:n].copy()
    if name == "grazing":           # a vertex passing an edge, and an edge passing an edge, at +- 2^-12 of the diagonal
        rng = np.random.default_rng(3703)
        p, what, edge, _ = sw._targets(rng, verts, idx, n)
        size = diag * rng.uniform(0.01, 0.05, n)
        u = sw._unit(rng, n)
        el = np.sqrt((edge * edge).sum(axis=1, keepdims=True))
        along = np.where(el > 0, edge / np.where(el > 0, el, 1.0), sw._unit(rng, n))
        w = np.cross(u, along)
        wl = np.sqrt((w * w).sum(axis=1, keepdims=True))
        w = np.where(wl > 1e-6, w / np.where(wl > 1e-6, wl, 1.0), sw._perp(rng, u))
        sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        lead = p + w * (diag * GRAZE * sign)[:, None] - u * (size * rng.uniform(1.5, 20.0, n))[:, None]
        # the leading vertex, or the leading edge's midpoint, passes the target at the offset; the rest trails on the offset's side
        back = -u + 0.5 * w * sign[:, None]
        side = np.cross(u, w)
        half = np.where((np.arange(n) % 2 == 0)[:, None], 0.0, 1.0) * side * (0.5 * size)[:, None]
        a0, a1 = lead - half, lead + half + np.where((np.arange(n) % 2 == 0)[:, None], back * size[:, None] + side * (0.4 * size)[:, None], 0.0)
        a2 = lead + back * size[:, None] - side * (0.3 * size)[:, None]
        d = u * (diag * rng.uniform(0.01, 1.0, n))[:, None]
        return pack(np.stack([a0, a1, a2], axis=1), d, np.inf)
    if name == "overlap":           # casts that start intersecting: centred within a third of their size of a point of the scene
        rng = np.random.default_rng(3704)
        p = sw._targets(rng, verts, idx, n)[0]
        size = diag * rng.uniform(0.01, 0.05, n)
        centre = p + sw._unit(rng, n) * (size * rng.uniform(0.0, 0.3, n))[:, None]
        d = sw._unit(rng, n) * (diag * rng.uniform(0.01, 1.0, n))[:, None]
        return pack(centre[:, None, :] + _shape(rng, n, size), d, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.0, 2.0, n)))
    if name == "short":             # tmax at 0.5, 1 and 2 times the brute force's t (the t itself: the closed end of the interval)
        base = cast_set("aimed", verts, idx, n=n).copy()
        t = cast_records(base, verts, idx, mats)[:, 0].view(np.float32)
        factor = np.asarray([0.5, 1.0, 2.0], np.float32)[np.arange(n) % 3]
        base[:, 3] = np.where(t >= 0, t * factor, F(1.0))
        return base
    if name == "outside":           # from outside the scene box: three in four away from it, one in four towards a point of it
        rng = np.random.default_rng(3706)
        centre = c + sw._unit(rng, n) * (diag * rng.uniform(1.5, 5.0, n))[:, None]
        target = lo + rng.random((n, 3)) * ext
        d = (target - centre) * np.where(np.arange(n) % 4 == 3, 1.0, -1.0)[:, None] * rng.uniform(0.1, 2.0, n)[:, None]
        size = diag * rng.uniform(0.01, 0.05, n)
        return pack(centre[:, None, :] + _shape(rng, n, size), d, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.5, 20.0, n)))
    if name == "zero_d":            # d = 0: only the start overlap can answer
        rng = np.random.default_rng(3707)
        p = sw._targets(rng, verts, idx, n)[0]
        size = diag * rng.uniform(0.01, 0.05, n)
        centre = p + sw._unit(rng, n) * (size * rng.uniform(0.0, 1.5, n))[:, None]
        return pack(centre[:, None, :] + _shape(rng, n, size), np.zeros((n, 3)), np.where(rng.random(n) < 0.5, np.inf, 1.0))
    if name == "degenerate":        # segment and point queries on the casts of "aimed" and "overlap"
        s = np.concatenate([cast_set("aimed", verts, idx, n=n)[0::2], cast_set("overlap", verts, idx, n=n)[1::2]])[:n].copy()
        kind = np.arange(n) % 4     # 0: a point; 1: a segment (a2 = a1); 2: a segment (a2 = a0); 3: a segment (a1 = a0)
        s[kind == 0, 4:7] = s[kind == 0, 0:3]
        s[kind == 0, 8:11] = s[kind == 0, 0:3]
        s[kind == 1, 8:11] = s[kind == 1, 4:7]
        s[kind == 2, 8:11] = s[kind == 2, 0:3]
        s[kind == 3, 4:7] = s[kind == 3, 0:3]
        return s
    if name == "coplanar":          # affine combinations of a scene triangle's vertices moving along a combination of its edges: exactly
        rng = np.random.default_rng(3709)       # in the plane on the axis-aligned walls
        v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
        tri = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)]
        t = tri[rng.integers(0, tri.shape[0], n)]
        e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        uw = rng.uniform(-1.0, 2.0, (n, 3, 2)).astype(np.float32)
        q = (t[:, None, 0] + uw[:, :, 0:1] * e1[:, None] + uw[:, :, 1:2] * e2[:, None]).astype(np.float32)
        k = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
        d = (k[:, 0:1] * e1 + k[:, 1:2] * e2).astype(np.float32)
        return pack(q, d, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.0, 2.0, n)))
    if name == "bad":               # every miss before any traversal, one component at a time, on every third cast of "aimed"
        s = cast_set("aimed", verts, idx, n=n).copy()
        cases = bad_cases()
        for i in range(1, n, 3):
            for k, val in cases[(i // 3) % len(cases)][0]:
                s[i, k] = val
        return s
    raise ValueError(name)


def bad_cases():
    """([(component, value), ...], what) of everything that makes a cast a miss before any traversal"""
    out = []
    names = {0: "a0.x", 1: "a0.y", 2: "a0.z", 4: "a1.x", 5: "a1.y", 6: "a1.z", 8: "a2.x", 9: "a2.y", 10: "a2.z", 12: "d.x", 13: "d.y", 14: "d.z"}
    for k, nm in names.items():
        for val in (np.nan, np.inf, -np.inf):
            out.append(([(k, F(val))], "%s = %s" % (nm, val)))
    for val, what in ((np.nan, "NaN"), (-np.inf, "-inf"), (-1.0, "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        out.append(([(3, F(val))], "tmax = %s" % what))
    big = F(3e38)
    for (i, j), nm in (((0, 4), "f1"), ((0, 8), "f2"), ((4, 8), "g")):
        for k in range(3):
            out.append(([(i + k, big), (j + k, -big)], "%s.%s overflows" % (nm, "xyz"[k])))
    return out


def bad_casts(good):
    good = np.asarray(good, np.float32).reshape(16)
    out, why = [], []
    for edits, what in bad_cases():
        r = good.copy()
        for k, val in edits:
            r[k] = val
        out.append(r); why.append(what)
    return np.array(out, np.float32), why
