"""NumPy statement of pt_query_box_cast's record (include/acgpt.h states the same definition), the brute force over all triangles it
is held to, the cast sets its tests use, a float64 bisection that knows nothing of the 13 axes and the 12-triangle route a caller
without the box cast takes.

Every operation is fp32 in the order of csrc/boxcast_device.h obox_triangle and obox_contact — oriented_ref's local coordinates,
overlap_ref's projections and radii, one speed per axis by the expression that projects a corner, two divisions per axis, selects
where the device selects, a NaN never a candidate — so the GPU's record equals this one bit for bit.  With float64 arrays the same
functions give the same algorithm in double.  The triangle is what the build stores in a TriRecord: v0, e1 = v1 - v0, e2 = v2 - v0,
one fp32 subtraction per component."""
import numpy as np

import nearest_ref as nr
import oriented_ref as ot
import overlap_ref as ov
import segment_ref as sg
import sweep_ref as sw
import tricast_ref as tc

F = np.float32
MISS_PRIM = np.uint32(0xFFFFFFFF)
SHADE_MAT_MASK = nr.SHADE_MAT_MASK
START = 13                      # the feature of a start overlap
N_FEATURES = 14
FLT_MAX = np.finfo(np.float32).max

_fmin3, _fmax3 = ov._fmin3, ov._fmax3


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


# ---- the record ---------------------------------------------------------------------------------------------------------------------
def pack(boxes, d, tmax):
    """(n, 20) float32 casts of (n, 16) oriented-box records, directions and tmax"""
    b = np.asarray(boxes, np.float32).reshape(-1, 16)
    c = np.zeros((b.shape[0], 20), np.float32)
    c[:, :16] = b
    c[:, 16:19] = d
    c[:, 19] = tmax
    return c


def parts(casts, dtype=np.float32):
    """(A, c, h, d, tmax) of (n, 20) casts, widened to dtype"""
    s = np.asarray(casts, np.float32).reshape(-1, 20)
    A, c, h = ot.parts(s[:, :16], dtype)
    return A, c, h, s[:, 16:19].astype(dtype), s[:, 19].astype(dtype)


def castable(casts):
    """False where a cast is a miss before any traversal: oriented_ref's rules on the first sixteen floats, a non-finite component of
    d, a NaN or negative tmax"""
    s = np.asarray(casts, np.float32).reshape(-1, 20)
    with np.errstate(all="ignore"):
        return ot.searchable(s[:, :16]) & np.isfinite(s[:, 16:19]).all(axis=1) & (s[:, 19] >= F(0.0))


def miss_records(n):
    rec = np.zeros((n, 12), np.uint32)
    rec[:, 0] = np.array([-1.0], np.float32).view(np.uint32)[0]
    rec[:, 1] = MISS_PRIM
    rec[:, 3] = MISS_PRIM
    return rec


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def _axis(k, lo, hi, r, s, st):
    te, tx, ax, sw_ = st
    dt = te.dtype.type
    still = s == 0
    sd = np.where(still, dt(1), s)
    a, b = (-r - hi) / sd, (r - lo) / sd
    swap = b < a
    en, ex = np.where(swap, b, a), np.where(swap, a, b)
    out = (lo > r) | (hi < -r)
    en = np.where(still, np.where(out, dt(np.inf), dt(-np.inf)), en)
    ex = np.where(still, np.where(out, dt(-np.inf), dt(np.inf)), ex)
    take = en > te
    return np.where(take, en, te), np.where(ex < tx, ex, tx), np.where(take, np.int8(k), ax), np.where(take, s, sw_)


def local_triangle(A, c, h, d, v0, e1, e2):
    """(P0, E1, E2, V): the triangle's stored vectors in the box's frame and the velocity -L(d)"""
    P0, E1, E2 = ot.local(A, v0 - c), ot.local(A, e1), ot.local(A, e2)
    return P0, E1, E2, -ot.local(A, d)


def box_triangle_local(h, P0, E1, E2, V):
    """(t, feature, s): the statement on local vectors; +inf where the pair is no candidate (tmax is the caller's), the winning axis
    (13: start overlap) and the speed on it"""
    dt = P0.dtype.type
    p0, p1, p2 = P0, P0 + E1, P0 + E2
    shape = np.broadcast(P0[..., 0], h[..., 0], V[..., 0]).shape
    st = (np.full(shape, -np.inf, P0.dtype), np.full(shape, np.inf, P0.dtype), np.zeros(shape, np.int8), np.zeros(shape, P0.dtype))
    for k in range(3):
        st = _axis(k, _fmin3(p0[..., k], p1[..., k], p2[..., k]), _fmax3(p0[..., k], p1[..., k], p2[..., k]), h[..., k], V[..., k], st)
    N = _cross(E1, E2)
    dn = _dot(N, p0)
    rn = (h[..., 0] * np.abs(N[..., 0]) + h[..., 1] * np.abs(N[..., 1])) + h[..., 2] * np.abs(N[..., 2])
    st = _axis(3, dn, dn, rn, _dot(N, V), st)
    for g, f in enumerate((E1, E2 - E1, E2)):
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            s0 = p0[..., k] * f[..., j] - p0[..., j] * f[..., k]
            s1 = p1[..., k] * f[..., j] - p1[..., j] * f[..., k]
            s2 = p2[..., k] * f[..., j] - p2[..., j] * f[..., k]
            r = h[..., j] * np.abs(f[..., k]) + h[..., k] * np.abs(f[..., j])
            s = V[..., k] * f[..., j] - V[..., j] * f[..., k]
            st = _axis(4 + 3 * g + i, _fmin3(s0, s1, s2), _fmax3(s0, s1, s2), r, s, st)
    te, tx, ax, sw_ = st
    cand = (te <= tx) & (tx >= 0)
    t = np.where(cand, np.where(te > 0, te, dt(0)), dt(np.inf))
    start = ov.tri_box_overlap(np.zeros(3, P0.dtype), h, P0, E1, E2)
    return np.where(start, dt(0), t), np.where(start, np.int8(START), ax), sw_


def box_triangle(A, c, h, d, v0, e1, e2):
    """(t, feature, s) of boxes {A, c, h} translating along d with triangles {v0, v0 + e1, v0 + e2}; the arrays broadcast against each
    other (A [..., 3, 3], the rest [..., 3]).  Any float dtype."""
    with np.errstate(all="ignore"):
        P0, E1, E2, V = local_triangle(A, c, h, d, v0, e1, e2)
        return box_triangle_local(h, P0, E1, E2, V)


def contact(A, c, h, d, v0, e1, e2, feature, s, t):
    """(normal, point) of the record for one winner per row (feature 0..12): rows of [n, 3] arrays, A [n, 3, 3]"""
    dt = c.dtype.type
    with np.errstate(all="ignore"):
        P0, E1, E2, V = local_triangle(A, c, h, d, v0, e1, e2)
        p0, p1, p2 = P0, P0 + E1, P0 + E2
        F1 = E2 - E1
        ax = feature.astype(np.int64)
        grp = np.where(ax < 7, 0, np.where(ax < 10, 1, 2))
        i = np.where(ax < 4, ax, ax - 4 - 3 * grp)
        i = np.where(ax == 3, 0, i)
        f = np.where((grp == 0)[:, None], E1, np.where((grp == 1)[:, None], F1, E2))
        zero = np.zeros_like(f[:, 0])
        unit = np.stack([(ax == 0).astype(c.dtype), (ax == 1).astype(c.dtype), (ax == 2).astype(c.dtype)], axis=1)
        edge = np.where((i == 0)[:, None], np.stack([zero, -f[:, 2], f[:, 1]], 1),
                        np.where((i == 1)[:, None], np.stack([f[:, 2], zero, -f[:, 0]], 1), np.stack([-f[:, 1], f[:, 0], zero], 1)))
        a = np.where((ax < 3)[:, None], unit, np.where((ax == 3)[:, None], _cross(E1, E2), edge))
        g = np.where((s > 0)[:, None], a, -a)
        u, v, w = A[:, :, 0], A[:, :, 1], A[:, :, 2]
        W = (g[:, 0:1] * u + g[:, 1:2] * v) + g[:, 2:3] * w
        ln = np.sqrt(_dot(W, W))
        normal = np.where((ln > 0)[:, None], W / ln[:, None], dt(0))
        sc = np.where(g > 0, -h, h)
        rows = np.arange(ax.shape[0])
        # 0..2: the triangle's corner that is extreme towards the box
        k3 = np.minimum(ax, 2)
        c0, c1, c2 = p0[rows, k3], p1[rows, k3], p2[rows, k3]
        ext = np.where(s > 0, _fmax3(c0, c1, c2), _fmin3(c0, c1, c2))
        corner = np.where((c0 == ext)[:, None], v0, np.where((c1 == ext)[:, None], v0 + e1, v0 + e2))
        # 3: the box's corner
        cen = c + d * t[:, None]
        bc = cen + ((sc[:, 0:1] * u + sc[:, 1:2] * v) + sc[:, 2:3] * w)
        # 4..12: the point of the triangle's edge
        j, k = (i + 1) % 3, (i + 2) % 3
        pa = np.where((grp == 1)[:, None], p1, p0)
        al = pa + V * t[:, None]
        fj, fk = f[rows, j], f[rows, k]
        dj, dk = sc[rows, j] - al[rows, j], sc[rows, k] - al[rows, k]
        ff = fj * fj + fk * fk
        par = (dj * fj + dk * fk) / ff
        par = np.where(par < 0, dt(0), par)
        par = np.where(par > 1, dt(1), par)
        par = np.where(ff > 0, par, dt(0))
        Aw = np.where((grp == 1)[:, None], v0 + e1, v0)
        Ew = np.where((grp == 0)[:, None], e1, np.where((grp == 1)[:, None], e2 - e1, e2))
        on_edge = Aw + Ew * par[:, None]
        point = np.where((ax < 3)[:, None], corner, np.where((ax == 3)[:, None], bc, on_edge))
    return normal, point


def box_records(casts, verts, idx, mat_ids, chunk=64):
    """pt_box_cast_hit records as uint32 [n, 12] (t, prim, feature, material | n.xyz, 0 | c.xyz, 0) by brute force: every cast against
    every triangle, candidates t <= min(tmax, FLT_MAX), the smallest t, ties to the lowest triangle index; then the contact on the
    winner"""
    s = np.ascontiguousarray(np.asarray(casts, np.float32).reshape(-1, 20))
    n = s.shape[0]
    rec = miss_records(n)
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    if v0.shape[0] == 0 or n == 0:
        return rec
    mats = np.asarray(mat_ids, np.uint32)
    ok = castable(s)
    A, c, h, d, tmax = parts(s)
    with np.errstate(all="ignore"):
        tmax = np.fmin(tmax, F(FLT_MAX))
    chunk = max(1, min(chunk, (1 << 17) // v0.shape[0] + 1))
    for start in range(0, n, chunk):
        sl = slice(start, min(n, start + chunk))
        t, feat, sp = box_triangle(A[sl, None], c[sl, None], h[sl, None], d[sl, None], v0[None], e1[None], e2[None])
        with np.errstate(invalid="ignore"):
            cand = (t <= tmax[sl, None]) & ok[sl, None]
        key = np.where(cand, t, F(np.inf))
        best = key.min(axis=1)
        win = np.argmax(cand & (key == best[:, None]), axis=1)           # the first (lowest) index among the ties
        found = cand.any(axis=1)
        rows = np.arange(win.size)
        tw, fw, sw_ = t[rows, win], feat[rows, win], sp[rows, win]
        nrm, pt = contact(A[sl], c[sl], h[sl], d[sl], v0[win], e1[win], e2[win], np.where(fw == START, 0, fw), sw_, tw)
        started = (fw == START)[:, None]
        out = np.zeros((win.size, 12), np.float32)
        out[:, 0] = tw
        out[:, 2] = fw.astype(np.float32)
        out[:, 4:7] = np.where(started, F(0.0), nrm)
        out[:, 8:11] = np.where(started, F(0.0), pt)
        out = out.view(np.uint32)
        out[:, 1] = win.astype(np.uint32)
        out[:, 3] = mats[win] & SHADE_MAT_MASK
        sub = rec[sl]
        sub[found] = out[found]
    return rec


def blocked_of(rec):
    """pt_query_box_cast_any's bytes from the records: t >= 0"""
    return (np.asarray(rec, np.uint32)[:, 0].view(np.float32) >= 0).astype(np.uint8)


def columns(rec):
    """dict of the record's fields from uint32 [n, 12] records"""
    r = np.asarray(rec, np.uint32)
    f = r.view(np.float32)
    return {"t": f[:, 0].copy(), "prim": r[:, 1].copy(), "feature": f[:, 2].copy(), "material": r[:, 3].copy(), "normal": f[:, 4:7].copy(), "point": f[:, 8:11].copy()}


# ---- float64 yardsticks ---------------------------------------------------------------------------------------------------------------
def impact_f64(casts, tri_v0, tri_e1, tri_e2):
    """float64 (t, feature) of cast i with triangle i (fp32 inputs, the same statement in double), +inf where there is none"""
    A, c, h, d, _ = parts(casts, np.float64)
    t, feat, _ = box_triangle(A, c, h, d, *(np.asarray(a, np.float64) for a in (tri_v0, tri_e1, tri_e2)))
    return t, feat


def _box_edges(A, c, h):
    """the 12 edges of boxes as (start, end) [12, n, 3] float64"""
    sign = np.array([[(-1.0, 1.0)[(k >> b) & 1] for b in range(3)] for k in range(8)])
    # the statement's box is {p : |L(p - c)| <= h}, L = A^T: its corners are c + A^-T (+-h), which is c + A (+-h) only for exactly
    # orthonormal axes (a rotation rounded to fp32 is off by 1e-7)
    corners = c[None] + np.einsum("nkj,cnj->cnk", np.linalg.inv(A).transpose(0, 2, 1), sign[:, None, :] * h[None])
    pairs = [(k, k | (1 << b)) for k in range(8) for b in range(3) if not k & (1 << b)]
    return np.stack([corners[i] for i, _ in pairs]), np.stack([corners[j] for _, j in pairs])


def box_triangle_distance_f64(A, c, h, v0, v1, v2):
    """float64 distance between the solid boxes and triangle i where they are disjoint (the smallest of the 12 box edges' distances to
    the triangle and the three corners' distances to the box); no axis of the statement is used"""
    e0, e1 = _box_edges(A, c, h)
    best = np.full(c.shape[0], np.inf)
    for k in range(12):
        best = np.minimum(best, sg.segment_f64(e0[k], e1[k], v0, v1, v2)[0])
    for p in (v0, v1, v2):
        q = np.maximum(np.abs(ot.local(A, p - c)) - h, 0.0)         # orthonormal to fp32's rounding: the yardstick's own tolerance
        best = np.minimum(best, np.sqrt((q * q).sum(axis=1)))
    return best


def bisect_impact_f64(casts, v0, e1, e2, iters=120):
    """(t, resolution): float64 time of impact of cast i with triangle i by bisection on oriented_ref.tri_obox_overlap(c + t d), which
    knows nothing of the sweep.  Box and triangle are convex, so their distance is convex in t and the overlap holds on one interval:
    a ternary search on the distance finds a time in it (or the closest approach), the bisection its start.  +inf for none.
    resolution: the width of the last bracket."""
    A, c, h, d, _ = parts(casts, np.float64)
    v0, e1, e2 = (np.asarray(a, np.float64) for a in (v0, e1, e2))
    v1, v2 = v0 + e1, v0 + e2

    def inside(t):
        return ot.tri_obox_overlap(A, c + d * t[:, None], h, v0, e1, e2)

    def dist(t):         # 0 where they overlap: a triangle's edge through a box face touches no box edge and brings no corner inside
        return np.where(inside(t), 0.0, box_triangle_distance_f64(A, c + d * t[:, None], h, v0, v1, v2))
    dd = (d * d).sum(axis=1)
    with np.errstate(all="ignore"):
        far = (np.sqrt(((c - v0) ** 2).sum(axis=1)) + np.sqrt((e1 * e1).sum(axis=1)) + np.sqrt((e2 * e2).sum(axis=1)) + 2.0 * np.sqrt((h * h).sum(axis=1))) / np.sqrt(dd)
    far = np.where(dd > 0, far, 0.0)
    a, b = np.zeros(c.shape[0]), far.copy()
    for _ in range(iters):                       # a tie is two times of overlap: both ends move in, and the bracket stays inside the interval
        m1, m2 = a + (b - a) / 3.0, b - (b - a) / 3.0
        d1, d2 = dist(m1), dist(m2)
        a, b = np.where(d1 >= d2, m1, a), np.where(d1 <= d2, m2, b)
    mid = 0.5 * (a + b)
    hit = inside(mid)
    start = inside(np.zeros_like(mid))
    lo_t, hi_t = np.zeros_like(mid), mid.copy()
    for _ in range(200):                         # not inside(lo_t), inside(hi_t)
        mid = 0.5 * (lo_t + hi_t)
        ins = inside(mid)
        lo_t, hi_t = np.where(ins, lo_t, mid), np.where(ins, mid, hi_t)
    t = np.where(start, 0.0, np.where(hit, hi_t, np.inf))
    return t, hi_t - lo_t


def obb_distance_f64(casts, t, points):
    """float64 distance of points[i] from the surface of cast i's box at c + d t[i] (0 on the surface; inside counts by depth)"""
    A, c, h, d, _ = parts(casts, np.float64)
    q = ot.local(A, np.asarray(points, np.float64) - (c + d * np.asarray(t, np.float64)[:, None]))
    out = np.maximum(np.abs(q) - h, 0.0)
    outside = np.sqrt((out * out).sum(axis=1))
    depth = (h - np.abs(q)).min(axis=1)
    return np.where(outside > 0, outside, np.maximum(depth, 0.0))


# ---- the 12-triangle route ----------------------------------------------------------------------------------------------------------
_CUBE_TRIS = ((0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3))


def surface_triangles(casts):
    """(n, 12, 3, 3) float32: the 12 triangles of each box's surface, corners c + A (+-h) rounded to fp32"""
    A, c, h, _, _ = parts(casts, np.float64)
    sign = np.array([[(-1.0, 1.0)[(k >> b) & 1] for b in range(3)] for k in range(8)])
    corners = c[:, None, :] + np.einsum("nkj,ncj->nck", A, sign[None] * h[:, None, :])
    return corners[:, np.array(_CUBE_TRIS)].astype(np.float32)


def twelve_triangle_route(casts, verts, idx, mat_ids):
    """What a caller without the box cast does: pt_query_triangle_cast's statement (tricast_ref, fp32) on the 12 n surface triangles
    and the reduction to the earliest.  t per cast, float64 (-1 where no surface triangle touches anything)."""
    s = np.asarray(casts, np.float32).reshape(-1, 20)
    tri = surface_triangles(s)
    n = s.shape[0]
    recs = tc.pack(tri.reshape(n * 12, 3, 3), np.repeat(s[:, 16:19], 12, axis=0), np.repeat(s[:, 19], 12))
    t = tc.cast_records(recs, verts, idx, mat_ids)[:, 0].view(np.float32).reshape(n, 12).astype(np.float64)
    best = np.where(t >= 0, t, np.inf).min(axis=1)
    return np.where(np.isfinite(best), best, -1.0)


def twelve_triangle_route_f64(casts, verts, idx, chunk=16):
    """The same route in float64 on the boxes' exact corners (tricast_ref.cast_pair, no rounding of the surface to fp32): t per cast,
    +inf where no surface triangle touches anything, tmax not applied"""
    A, c, h, d, _ = parts(casts, np.float64)
    sign = np.array([[(-1.0, 1.0)[(k >> b) & 1] for b in range(3)] for k in range(8)])
    corners = c[:, None, :] + np.einsum("nkj,ncj->nck", np.linalg.inv(A).transpose(0, 2, 1), sign[None] * h[:, None, :])      # _box_edges' corners
    tri = corners[:, np.array(_CUBE_TRIS)]                                     # [n, 12, 3, 3]
    v0, e1, e2 = (a.astype(np.float64) for a in nr.records_of_scene(verts, idx))
    out = np.full(c.shape[0], np.inf)
    for start in range(0, c.shape[0], chunk):
        sl = slice(start, min(c.shape[0], start + chunk))
        q = tri[sl].reshape(-1, 1, 3, 3)
        dq = np.repeat(d[sl], 12, axis=0)[:, None]
        t = tc.cast_pair(q[:, :, 0], q[:, :, 1], q[:, :, 2], dq, v0[None], e1[None], e2[None])[0]
        out[sl] = t.reshape(-1, 12 * v0.shape[0]).min(axis=1)
    return out


# ---- cast sets -------------------------------------------------------------------------------------------------------------------
# Fixed seeds, SET_SIZE casts each (n of the caller's on other scenes).  "aimed" and "links" are made from the triangles and the scene
# box alone and hold on any scene; the others are meant for the Cornell fixtures.
CAST_SETS = ("aimed", "grazing", "links", "cells", "flat", "identity", "axis_turns", "overlap", "contain", "short", "outside", "zero_d", "tolerance", "bad")
SCENE_SETS = ("aimed", "links")
COVERAGE_SETS = ("aimed", "grazing", "links", "cells")
SET_SIZE = 1000
GRAZE = 2.0 ** -12


def _pieces(tri):
    """(lo, hi) float64 of every connected piece of the mesh (triangles that share a vertex position), from [n, 3, 3] corners"""
    uniq, inv = np.unique(tri.reshape(-1, 3), axis=0, return_inverse=True)
    ti = inv.reshape(-1, 3)
    parent = np.arange(uniq.shape[0])

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in ti:
        ra = find(a)
        parent[find(b)] = ra
        parent[find(c)] = ra
    root = np.array([find(x) for x in ti[:, 0]])
    return [(tri[root == r].reshape(-1, 3).min(axis=0), tri[root == r].reshape(-1, 3).max(axis=0)) for r in np.unique(root)]


def _frame(ai, hint, i):
    """(n, 3, 3) float64 rotations whose column i[n] is the unit vector ai and whose column i + 1 is hint made perpendicular to it"""
    b = hint - ai * (hint * ai).sum(axis=1, keepdims=True)
    b /= np.sqrt((b * b).sum(axis=1, keepdims=True))
    third = np.cross(ai, b)
    R = np.zeros((ai.shape[0], 3, 3))
    rows = np.arange(ai.shape[0])
    R[rows, :, i] = ai
    R[rows, :, (i + 1) % 3] = b
    R[rows, :, (i + 2) % 3] = third
    return R


def _aimed_boxes(rng, verts, idx, n, diag):
    """Boxes placed so that a chosen feature leads onto a target of the mesh: a face onto a corner, an edge onto an edge's midpoint, a
    corner onto a centroid.  Returns (R, h, lead point in world offsets R q, u, target, what)."""
    p, what, edge, inward = sw._targets(rng, verts, idx, n)
    h = diag * rng.uniform(0.005, 0.04, (n, 3))
    u = sw._unit(rng, n)
    il = np.sqrt((inward * inward).sum(axis=1, keepdims=True))
    head_on = inward / np.where(il > 0, il, 1.0) + 0.15 * u
    hl = np.sqrt((head_on * head_on).sum(axis=1, keepdims=True))
    u = np.where((what == 2)[:, None] & (il > 0) & (hl > 1e-3), head_on / np.where(hl > 1e-3, hl, 1.0), u)
    i = rng.integers(0, 3, n)
    rows = np.arange(n)
    j, k = (i + 1) % 3, (i + 2) % 3
    q = np.zeros((n, 3))
    # a corner: any rotation, the corner that leads along u
    R = ot.rotations(rng, n).astype(np.float64)
    ul = np.einsum("nkj,nk->nj", R, u)
    q_corner = np.where(ul >= 0, 1.0, -1.0) * h
    # a face: axis i along u, tilted a little; the target somewhere on the face
    tilt = u + 0.2 * sw._unit(rng, n)
    tilt /= np.sqrt((tilt * tilt).sum(axis=1, keepdims=True))
    R_face = _frame(tilt, sw._unit(rng, n), i)
    q_face = np.zeros((n, 3))
    q_face[rows, i] = h[rows, i]
    q_face[rows, j] = h[rows, j] * rng.uniform(-0.6, 0.6, n)
    q_face[rows, k] = h[rows, k] * rng.uniform(-0.6, 0.6, n)
    # an edge: axis i across the motion, the edge (+j, -k) leading, turned up to 25 degrees from the symmetric position
    ai = sw._perp(rng, u) + 0.2 * sw._unit(rng, n)
    ai /= np.sqrt((ai * ai).sum(axis=1, keepdims=True))
    b1 = u - ai * (u * ai).sum(axis=1, keepdims=True)
    b1 /= np.sqrt((b1 * b1).sum(axis=1, keepdims=True))
    b2 = np.cross(ai, b1)
    ang = np.pi / 4 + rng.uniform(-0.45, 0.45, n)
    aj = b1 * np.cos(ang)[:, None] + b2 * np.sin(ang)[:, None]
    R_edge = _frame(ai, aj, i)
    q_edge = np.zeros((n, 3))
    q_edge[rows, i] = h[rows, i] * rng.uniform(-0.6, 0.6, n)
    q_edge[rows, j] = h[rows, j]
    q_edge[rows, k] = -h[rows, k]
    w2, w1 = (what == 2)[:, None, None], (what == 1)[:, None, None]
    R = np.where(w2, R_face, np.where(w1, R_edge, R))
    q = np.where(w2[:, 0], q_face, np.where(w1[:, 0], q_edge, q_corner))
    return R, h, np.einsum("nkj,nj->nk", R, q), u, p, what


def cast_set(name, verts, idx, camera=None, mat_ids=None, n=SET_SIZE):
    """n casts float32 [n, 20] of the named set"""
    lo, hi, cen, diag = sw._extent(verts, idx)
    ext = hi.astype(np.float64) - lo
    _unit = sw._unit
    rows = np.arange(n)
    if name == "aimed":             # a face onto a corner, an edge onto an edge, a corner onto a face; an eighth start in contact
        rng = np.random.default_rng(4001)
        R, h, lead, u, p, what = _aimed_boxes(rng, verts, idx, n, diag)
        size = h.max(axis=1)
        dist = size * rng.uniform(3.0, 30.0, n)
        dist = np.where(rng.random(n) < 0.125, -size * rng.uniform(0.0, 0.5, n), dist)
        c = p - lead - u * dist[:, None]
        d = u * (diag * rng.uniform(0.01, 1.0, n))[:, None]            # not normalised: t is in units of |d|
        return pack(ot.as_oboxes(c, h, R), d, np.inf)
    if name == "grazing":           # the box moves along its own axis i and a vertex or a point of an edge passes a side face at
        rng = np.random.default_rng(4002)       # h_j (1 +- 2^-12) from the axis: just caught by the leading face, or just missed
        p, what, edge, _ = sw._targets(rng, verts, idx, n)
        h = diag * rng.uniform(0.005, 0.04, (n, 3))
        u = _unit(rng, n)
        i = rng.integers(0, 3, n)
        j, k = (i + 1) % 3, (i + 2) % 3
        R = _frame(u, _unit(rng, n), i)
        sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        q = np.zeros((n, 3))
        q[rows, i] = h[rows, i]
        q[rows, j] = h[rows, j] * (1.0 + sign * GRAZE) * np.where(rng.random(n) < 0.5, 1.0, -1.0)
        q[rows, k] = h[rows, k] * rng.uniform(-0.6, 0.6, n)
        c = p - np.einsum("nkj,nj->nk", R, q) - u * (h.max(axis=1) * rng.uniform(3.0, 30.0, n))[:, None]
        d = u * (diag * rng.uniform(0.01, 1.0, n))[:, None]
        return pack(ot.as_oboxes(c, h, R), d, np.inf)
    if name == "links":             # long and thin: one half extent 5 - 20 % of the diagonal, the other two 0.2 - 2 %
        rng = np.random.default_rng(4003)
        h = diag * rng.uniform(0.002, 0.02, (n, 3))
        h[rows, rng.integers(0, 3, n)] = diag * rng.uniform(0.05, 0.20, n)
        c = lo + (0.3 + 0.4 * rng.random((n, 3))) * ext
        d = _unit(rng, n) * (diag * rng.uniform(0.05, 0.5, n))[:, None]
        return pack(ot.as_oboxes(c, h, ot.rotations(rng, n)), d, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.2, 3.0, n)))
    if name == "cells":             # cubes in any rotation from inside the scene box
        rng = np.random.default_rng(4004)
        h = np.repeat(diag * rng.uniform(0.01, 0.05, (n, 1)), 3, axis=1)
        c = lo + (0.15 + 0.7 * rng.random((n, 3))) * ext
        d = _unit(rng, n) * (diag * rng.uniform(0.05, 0.5, n))[:, None]
        return pack(ot.as_oboxes(c, h, ot.rotations(rng, n)), d, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.2, 3.0, n)))
    if name == "flat":              # oriented_ref's points, segments, rectangles and thin boxes, moved back from their surface points
        rng = np.random.default_rng(4005)
        b = ot.box_set("flat", verts, idx, n=n).copy()
        u = _unit(rng, n)
        back = diag * rng.uniform(0.0, 0.3, n) * (rows % 5 != 0)
        b[:, 3], b[:, 7], b[:, 11] = (b[:, [3, 7, 11]].astype(np.float64) - u * back[:, None]).T
        return pack(b, u * (diag * rng.uniform(0.05, 0.5, n))[:, None], np.inf)
    if name == "identity":          # oriented_ref's axis-aligned boxes under the exact identity; half move along a world axis
        rng = np.random.default_rng(4006)
        b = ot.box_set("identity", verts, idx, n=n)
        u = _unit(rng, n)
        axis = np.eye(3)[rng.integers(0, 3, n)] * np.where(rng.random(n) < 0.5, 1.0, -1.0)[:, None]
        u = np.where((rows % 2 == 0)[:, None], axis, u)
        return pack(b, u * (diag * rng.uniform(0.05, 0.5, n))[:, None], np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.2, 3.0, n)))
    if name == "axis_turns":        # signed permutations: the walls' edges run along box axes and the cross axes vanish
        rng = np.random.default_rng(4007)
        b = ot.box_set("axis_turns", verts, idx, n=n)
        u = _unit(rng, n)
        axis = np.eye(3)[rng.integers(0, 3, n)] * np.where(rng.random(n) < 0.5, 1.0, -1.0)[:, None]
        u = np.where((rows % 2 == 0)[:, None], axis, u)
        return pack(b, u * (diag * rng.uniform(0.05, 0.5, n))[:, None], np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.2, 3.0, n)))
    if name == "overlap":           # starts in contact: oriented_ref's mixed sets, which overlap the mesh for a good part
        rng = np.random.default_rng(4008)
        b = np.concatenate([ot.box_set("random", verts, idx, n=n)[: n - n // 2], ot.box_set("walls_turned", verts, idx, n=n)[: n // 2]])
        return pack(b, _unit(rng, n) * (diag * rng.uniform(0.01, 0.5, n))[:, None], np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.0, 2.0, n)))
    if name == "contain":           # whole triangles of the scene start inside the solid box: a quarter of the smallest triangles under any
        rng = np.random.default_rng(4009)       # rotation (the surface usually meets their neighbours), and whole connected pieces of the mesh
        v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
        tri = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)]
        m = tri.mean(axis=1)
        rad = np.sqrt(((tri - m[:, None]) ** 2).sum(axis=2)).max(axis=1)
        small = np.argsort(rad)[: max(1, tri.shape[0] // 4)]
        pick = small[rng.integers(0, small.size, n)]
        h = np.repeat((rad[pick] * rng.uniform(1.05, 1.5, n))[:, None], 3, axis=1) + diag * 1e-4
        c, R = m[pick], ot.rotations(rng, n).astype(np.float64)
        # pieces whose box is well inside the scene's: under the identity with a margin below a thousandth of the diagonal (a piece that
        # floats that far from its neighbours is touched by no face of the box), and in a cube about their bounding sphere, turned
        pieces = [(plo, phi) for plo, phi in _pieces(tri) if ((phi - plo) <= 0.6 * ext).all()]
        for i in range(0, n, 2):
            if not pieces:
                break
            plo, phi = pieces[rng.integers(0, len(pieces))]
            pc, ph = 0.5 * (plo + phi), 0.5 * (phi - plo)
            if (i // 2) % 2 == 0:
                c[i], h[i], R[i] = pc, ph + diag * rng.uniform(1e-4, 4e-4), np.eye(3)
            else:
                c[i], h[i] = pc, np.sqrt((ph * ph).sum()) * rng.uniform(1.02, 1.1)
        return pack(ot.as_oboxes(c, h, R), _unit(rng, n) * (diag * rng.uniform(0.01, 0.5, n))[:, None], np.inf)
    if name == "short":             # tmax one ulp below, at, and one ulp above the brute force's t (the closed end of the interval)
        base = cast_set("aimed", verts, idx, n=n).copy()
        t = box_records(base, verts, idx, mat_ids if mat_ids is not None else np.zeros(len(idx) // 3, np.uint32))[:, 0].view(np.float32)
        k = rows % 3
        with np.errstate(all="ignore"):
            near = np.where(k == 0, np.nextafter(t, F(-np.inf)), np.where(k == 1, t, np.nextafter(t, F(np.inf))))
        base[:, 19] = np.where(t > 0, near, F(1.0))
        return base
    if name == "outside":           # from outside the scene box, towards a point of it and away from it
        rng = np.random.default_rng(4010)
        c = cen + _unit(rng, n) * (diag * rng.uniform(1.5, 5.0, n))[:, None]
        target = lo + rng.random((n, 3)) * ext
        d = (target - c) * np.where(rows % 4 == 3, -1.0, 1.0)[:, None] * rng.uniform(0.1, 2.0, n)[:, None]
        h = diag * rng.choice([0.0, 0.01, 0.05, 0.25], (n, 3))
        return pack(ot.as_oboxes(c, h, ot.rotations(rng, n)), d, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.5, 20.0, n)))
    if name == "zero_d":            # d = 0: only the start overlap can answer, and the byte is pt_query_overlap_oriented_any's
        rng = np.random.default_rng(4011)
        b = np.concatenate([ot.box_set("random", verts, idx, n=n)[: n - n // 2], ot.box_set("links", verts, idx, n=n)[: n // 2]])
        return pack(b, np.zeros((n, 3)), np.where(rng.random(n) < 0.5, np.inf, 1.0))
    if name == "tolerance":         # oriented_ref's axes just inside and just outside the orthonormality rule
        rng = np.random.default_rng(4012)
        b = ot.box_set("tolerance", verts, idx, n=n)
        return pack(b, _unit(rng, n) * (diag * rng.uniform(0.05, 0.5, n))[:, None], np.inf)
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
    for k in list(range(15)) + [16, 17, 18]:
        for val in (np.nan, np.inf, -np.inf):
            out.append((((k, F(val)),), "float %d = %s" % (k, val)))
    for k in range(12, 15):
        for val, what in ((F(-1.0), "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
            out.append((((k, val),), "half extent %d = %s" % (k - 12, what)))
    for val, what in ((np.nan, "NaN"), (-np.inf, "-inf"), (-1.0, "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
        out.append((((19, F(val)),), "tmax = %s" % what))
    out.append((((0, F(2.0)),), "an axis that is not a unit vector"))
    return out


def bad_casts(good):
    good = np.asarray(good, np.float32).reshape(20)
    out, why = [], []
    for sets, what in bad_cases():
        r = good.copy()
        for k, val in sets:
            r[k] = val
        out.append(r); why.append(what)
    return np.array(out, np.float32), why
