"""NumPy statement of pt_query_overlap_oriented (include/acgpt.h states the same definition): the local coordinates, the miss rule with
its orthonormality check, the brute force over all triangles, pt_pose_boxes' statement, and the box sets the tests use.

Every operation is fp32 in the order of csrc/oriented_device.h OBoxQuery — nine dot products written (a.x b.x + a.y b.y) + a.z b.z, one
subtraction per component for v0 - c, then overlap_ref.tri_box_overlap about the origin — so the GPU's counts, lists and any bytes equal
these bit for bit.  The edges are rotated, not formed again from rotated points."""
import numpy as np

import overlap_ref as ov
from nearest_ref import records_of_scene, scene_box
from overlap_ref import lists_of_matrix          # the list rule is the axis-aligned query's

F = np.float32
NO_PRIM = ov.NO_PRIM
MAX_PRIMS = ov.MAX_PRIMS
ORTHO_TOL = F(2.0 ** -10)
SET_SIZE = 1000
GRID = (16, 16, 16)


# ---- the record ---------------------------------------------------------------------------------------------------------------------
def as_oboxes(centres, half_extents, rotations):
    """(n, 16) float32 records {m[0..11] | hx, hy, hz, 0}: rotations (3, 3) or (n, 3, 3), local -> world, its columns the box's axes"""
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    n = c.shape[0]
    b = np.zeros((n, 16), np.float32)
    m = b[:, :12].reshape(n, 3, 4)
    m[:, :, :3] = np.broadcast_to(np.asarray(rotations, np.float32), (n, 3, 3))
    m[:, :, 3] = c
    b[:, 12:15] = np.broadcast_to(np.asarray(half_extents, np.float32), (n, 3))
    return b


def parts(boxes, dtype=np.float32):
    """(A [n, 3, 3], c [n, 3], h [n, 3]) of (n, 16) records, widened to dtype: A[:, k, j] = m[4 k + j], column j the box's axis j"""
    b = np.asarray(boxes, np.float32).reshape(-1, 16)
    m = b[:, :12].reshape(-1, 3, 4)
    return m[:, :, :3].astype(dtype), m[:, :, 3].astype(dtype), b[:, 12:15].astype(dtype)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def local(A, p):
    """L(p) = ((m0 p.x + m4 p.y) + m8 p.z, ...): component j is the dot product of column j with p.  A [..., 3, 3], p [..., 3], any dtype"""
    return np.stack([_dot3(A[..., :, j], p) for j in range(3)], axis=-1)


def searchable(boxes):
    """False where a record is a miss before any traversal: a non-finite value among the first 15 floats, a negative or NaN half extent,
    axes that are not orthonormal to 2^-10 by the fp32 dot products of the statement"""
    b = np.asarray(boxes, np.float32).reshape(-1, 16)
    A, _, h = parts(b)
    one = F(1.0)
    with np.errstate(all="ignore"):
        u, v, w = A[:, :, 0], A[:, :, 1], A[:, :, 2]
        ortho = (np.abs(_dot3(u, u) - one) <= ORTHO_TOL) & (np.abs(_dot3(v, v) - one) <= ORTHO_TOL) & (np.abs(_dot3(w, w) - one) <= ORTHO_TOL) & \
                (np.abs(_dot3(u, v)) <= ORTHO_TOL) & (np.abs(_dot3(v, w)) <= ORTHO_TOL) & (np.abs(_dot3(w, u)) <= ORTHO_TOL)
        return np.isfinite(b[:, :15]).all(axis=1) & (h >= F(0.0)).all(axis=1) & ortho


def tri_obox_overlap(A, c, h, v0, e1, e2):
    """bool: the statement on broadcastable arrays of one dtype (A [..., 3, 3], the rest [..., 3])"""
    with np.errstate(all="ignore"):
        P0, E1, E2 = local(A, v0 - c), local(A, e1), local(A, e2)
        return ov.tri_box_overlap(np.zeros(3, P0.dtype), h, P0, E1, E2)


def overlap_matrix(boxes, verts, idx, dtype=np.float32, chunk=256):
    """bool [n, n_tris]: box i against triangle j, by the statement in `dtype` (the fp32 records widened for float64), with the miss
    rule applied (in fp32 whatever dtype is)"""
    b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 16))
    v0, e1, e2 = (a.astype(dtype) for a in records_of_scene(verts, idx))
    out = np.zeros((b.shape[0], v0.shape[0]), bool)
    if v0.shape[0] == 0 or b.shape[0] == 0:
        return out
    ok = searchable(b)
    A, c, h = parts(b, dtype)
    for start in range(0, b.shape[0], chunk):
        sl = slice(start, min(b.shape[0], start + chunk))
        out[sl] = tri_obox_overlap(A[sl, None], c[sl, None], h[sl, None], v0[None], e1[None], e2[None]) & ok[sl, None]
    return out


def overlap_records(boxes, verts, idx, max_prims=MAX_PRIMS, chunk=256):
    """(counts, prims, any) by brute force: every box against every triangle"""
    return lists_of_matrix(overlap_matrix(boxes, verts, idx, np.float32, chunk), max_prims)


def world_aabbs(boxes):
    """(n, 8) float32 pt_query_overlap records: the world AABB of each oriented box, H_k = sum_j |A_kj| h_j in float64, rounded up"""
    A, c, h = parts(boxes, np.float64)
    H = (np.abs(A) * h[:, None, :]).sum(axis=2)
    H32 = H.astype(np.float32)
    H32 = np.where(H32.astype(np.float64) < H, np.nextafter(H32, F(np.inf)), H32)
    return ov.as_boxes(c.astype(np.float32), H32)


def pose_boxes(poses, local_box):
    """pt_pose_boxes in NumPy: (P, 16) float32 records of (P, 12) poses and local_box = (cx, cy, cz, hx, hy, hz); the centre is the pose
    statement of include/acgpt.h, ((m0 x + m1 y) + m2 z) + m3 per row, every operation fp32"""
    m = np.asarray(poses, np.float32).reshape(-1, 3, 4)
    lb = np.asarray(local_box, np.float32).reshape(6)
    out = np.zeros((m.shape[0], 16), np.float32)
    o = out[:, :12].reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        o[:, :, :3] = m[:, :, :3]
        o[:, :, 3] = ((m[:, :, 0] * lb[0] + m[:, :, 1] * lb[1]) + m[:, :, 2] * lb[2]) + m[:, :, 3]
    out[:, 12:15] = lb[3:6]
    return out


# ---- rotations ----------------------------------------------------------------------------------------------------------------------
def rotations(rng, n):
    """n uniform random rotations (n, 3, 3) float32, from unit quaternions in float64"""
    q = rng.normal(size=(n, 4))
    return _of_quaternions(q / np.linalg.norm(q, axis=1, keepdims=True))


def _of_quaternions(q):
    w, x, y, z = q.T
    r = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)
    return r.astype(np.float32)


def turns_about(axis, angle):
    """(n, 3, 3) float32 rotations about world axis axis[i] by angle[i]: the axis' row and column are exactly those of the identity"""
    n = len(axis)
    r = np.zeros((n, 3, 3), np.float32)
    cs, sn = np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)
    rows = np.arange(n)
    j, k = (axis + 1) % 3, (axis + 2) % 3
    r[rows, axis, axis] = 1.0
    r[rows, j, j], r[rows, j, k], r[rows, k, j], r[rows, k, k] = cs, -sn, sn, cs
    return r


def signed_permutations():
    """the 48 signed permutation matrices (24 of them mirrors), float32"""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3), np.float32)
            for j in range(3):
                m[perm[j], j] = signs[j]
            out.append(m)
    return np.array(out)


# ---- box sets -------------------------------------------------------------------------------------------------------------------------
# Fixed seeds.  tests/test_oriented_host.py holds the shares of the sets on the Cornell fixtures by the brute force alone.
BOX_SETS = ("random", "links", "grid_frame", "identity", "axis_turns", "walls_turned", "flat", "tolerance", "whole", "outside", "far")
MIXED_SETS = ("random", "links", "grid_frame")
IDENTITY_PARTS = ("random", "centroids", "wall_faces")
TOLERANCE_KINDS = ("scale up, inside", "scale down, inside", "shear, inside", "scale up, outside", "scale down, outside", "shear, outside")


def identity_aabbs(verts, idx, n=SET_SIZE):
    """(n, 8) pt_query_overlap records behind the "identity" set: a third each of overlap_ref's random, centroids and wall_faces"""
    per = [n - 2 * (n // 3), n // 3, n // 3]
    return np.concatenate([ov.box_set(name, verts, idx, n=max(k, 1))[:k] for name, k in zip(IDENTITY_PARTS, per)])


def tolerance_kinds(n=SET_SIZE):
    return np.arange(n) % len(TOLERANCE_KINDS)


def _wall_planes(rng, n, lo, hi, tri):
    """wall_faces' planes (overlap_ref): per box an axis, the coordinate of a wall of the scene box or of a vertex on that axis, the
    vertex, and which of the two it is"""
    axis, side, vert = rng.integers(0, 3, n), rng.integers(0, 2, n), rng.integers(0, 2, n).astype(bool)
    pv = tri[rng.integers(0, tri.shape[0], n), rng.integers(0, 3, n)]
    plane = np.where(vert, pv[np.arange(n), axis], np.where(side == 0, lo[axis], hi[axis])).astype(np.float32)
    return axis, side, vert, pv, plane


def box_set(name, verts, idx, n=SET_SIZE):
    """n oriented boxes (n, 16) float32 of the named set, from the scene's own box"""
    lo, hi = scene_box(verts, idx)
    ext = hi - lo
    d64 = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    diag = F(d64) if d64 > 0 else F(1.0)
    cen = F(0.5) * (lo + hi)
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    tri = v[np.asarray(idx, np.uint32).reshape(-1, 3).astype(np.int64)]
    rows = np.arange(n)
    if name == "random":            # overlap_ref's "random" with uniform random rotations
        b = ov.box_set("random", verts, idx, n=n)
        return as_oboxes(b[:, 0:3], b[:, 3:6], rotations(np.random.default_rng(3801), n))
    if name == "links":             # elongated: one half extent 5 - 20 % of the diagonal, the other two 0.2 - 2 %
        rng = np.random.default_rng(3802)
        c = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        h = (diag * rng.uniform(0.002, 0.02, (n, 3)).astype(np.float32)).astype(np.float32)
        h[rows, rng.integers(0, 3, n)] = (diag * rng.uniform(0.05, 0.20, n).astype(np.float32)).astype(np.float32)
        return as_oboxes(c, h, rotations(rng, n))
    if name == "grid_frame":        # n cells of the 16^3 grid over the scene box, turned by one rotation about the scene's centre
        rng = np.random.default_rng(3803)
        g = ov.grid_boxes(GRID, lo, hi)
        if n < g.shape[0]:
            g = g[np.sort(rng.permutation(g.shape[0])[:n])]
        r = rotations(rng, 1)[0]
        c = (cen + (g[:, 0:3] - cen) @ r.T).astype(np.float32)
        return as_oboxes(c, g[:, 3:6], r)
    if name == "identity":          # overlap_ref's own boxes under the exact identity
        b = identity_aabbs(verts, idx, n)
        return as_oboxes(b[:, 0:3], b[:, 3:6], np.eye(3, dtype=np.float32))
    if name == "axis_turns":        # signed permutation matrices, mirrors among them
        rng = np.random.default_rng(3804)
        b = ov.box_set("random", verts, idx, n=n)
        return as_oboxes(b[:, 0:3], b[:, 3:6], signed_permutations()[rng.integers(0, 48, n)])
    if name == "walls_turned":      # wall_faces, turned only about the axis of the touching face: L is exact on that axis, so the closed
        rng = np.random.default_rng(3805)       # conditions meet equality
        c = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        h = (diag * F(10.0) ** rng.uniform(-3.0, -1.0, (n, 3)).astype(np.float32)).astype(np.float32)
        axis, side, vert, pv, plane = _wall_planes(rng, n, lo, hi, tri)
        c[vert] = pv[vert]
        out = rng.integers(0, 2, n).astype(bool)
        sign = np.where(out == (side == 0), F(-1.0), F(1.0)).astype(np.float32)
        c[rows, axis] = (plane + sign * h[rows, axis]).astype(np.float32)
        return as_oboxes(c, h, turns_about(axis, rng.uniform(0.0, 2.0 * np.pi, n)))
    if name == "flat":              # points, segments, rectangles and thin boxes on points of the surface
        rng = np.random.default_rng(3806)
        pts, _ = ov.surface_points_f64(verts, idx, n, seed=3816)
        h = (diag * F(10.0) ** rng.uniform(-5.0, -1.5, (n, 3)).astype(np.float32)).astype(np.float32)
        kind = rows % 4                 # 0: point, 1: segment (two zero axes), 2: rectangle (one zero axis), 3: a thin box
        ax = rng.integers(0, 3, n)
        h[kind == 0] = 0.0
        for k in range(3):
            h[(kind == 1) & (ax != k), k] = 0.0
            h[(kind == 2) & (ax == k), k] = 0.0
        return as_oboxes(pts.astype(np.float32), h, rotations(rng, n))
    if name == "tolerance":         # rotations scaled and sheared to just inside and just outside the 2^-10 of the orthonormality rule
        rng = np.random.default_rng(3807)
        c = (lo + rng.random((n, 3)).astype(np.float32) * ext).astype(np.float32)
        h = (diag * rng.uniform(0.01, 0.15, (n, 3)).astype(np.float32)).astype(np.float32)
        r = rotations(rng, n).astype(np.float64)
        kind = tolerance_kinds(n)
        scale = np.choose(kind, [1.0 + 2.0 ** -11.2, 1.0 - 2.0 ** -11.2, 1.0, 1.0 + 2.0 ** -10.8, 1.0 - 2.0 ** -10.8, 1.0])
        shear = np.choose(kind, [0.0, 0.0, 2.0 ** -10.2, 0.0, 0.0, 2.0 ** -9.8])
        s = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
        s[:, 0, 1] = shear
        return as_oboxes(c, h, (r @ s) * scale[:, None, None])
    if name == "whole":             # boxes containing the whole scene (count == n_tris) in any rotation: every half extent above the diagonal's half
        rng = np.random.default_rng(3808)
        h = (np.maximum(diag, F(1e-3)) * (F(0.75) + rng.random((n, 3)).astype(np.float32) * F(10.0))).astype(np.float32)
        return as_oboxes(np.broadcast_to(cen, (n, 3)), h, rotations(rng, n))
    if name == "outside":           # overlap_ref's "outside", 3 diagonals out and more with half extents below a third of one: still outside when turned
        b = ov.box_set("outside", verts, idx, n=n)
        return as_oboxes(b[:, 0:3], b[:, 3:6], rotations(np.random.default_rng(3809), n))
    if name == "far":               # overlap_ref's "far", centred 10 to 100 diagonals out, turned about a random axis by an angle that moves
        rng = np.random.default_rng(3810)       # the near end by up to a fifth of the diagonal: it swings into the scene, or just out of it
        b = ov.box_set("far", verts, idx, n=n)
        axis = rng.normal(size=(n, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        half = 0.5 * rng.uniform(0.02, 0.2, n) * float(diag) / b[:, 3:6].max(axis=1).astype(np.float64)
        q = np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * axis], axis=1)
        return as_oboxes(b[:, 0:3], b[:, 3:6], _of_quaternions(q))
    raise ValueError(name)


# the bad records of the tests: each with what makes it a miss before any traversal; `good` is the record they are made from
def bad_boxes(good):
    good = np.asarray(good, np.float32).reshape(16)
    out, why = [], []
    for k in range(15):
        for val in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = val
            out.append(r); why.append("float %d = %s" % (k, val))
    for k in range(12, 15):
        for val, what in ((F(-1.0), "-1"), (np.nextafter(F(0.0), F(-1.0)), "the largest negative number")):
            r = good.copy(); r[k] = val
            out.append(r); why.append("half extent %d = %s" % (k - 12, what))
    return np.array(out, np.float32), why
