"""The NumPy statement of the posed-mesh queries (include/acgpt.h: pt_pose_triangles, pt_query_poses_any, pt_query_poses_distance),
the meshes and the pose sets of their tests.

transform is the header's statement, x' = ((m[0] x + m[1] y) + m[2] z) + m[3] per row, every multiply and add a float32 operation of
its own in that order.  poses_any and poses_distance are brute force on the posed records: tritri_ref.intersect_matrix and
tridist_ref.triangle_distance_records decide each posed triangle, and the pose's answer is the lowest intersecting mesh triangle,
respectively the minimum of (d2, mesh triangle) over the triangles that found something."""
import functools
import os

import numpy as np

import tridist_ref as tr
import tritri_ref as tt

F = np.float32
MISS = 0xFFFFFFFF


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def as_poses(matrices):
    """(P, 12) float32 rows of (P, 3, 4) or (P, 4, 4) matrices (or one)"""
    m = np.asarray(matrices, np.float32)
    if m.ndim == 2 and m.shape[1] != 12:
        m = m[None]
    if m.ndim == 2:
        return np.ascontiguousarray(m)
    return np.ascontiguousarray(m[:, :3, :]).reshape(-1, 12)


def transform(poses, records):
    """(P, T, 12) float32 posed records {a0', 0 | a1', 0 | a2', 0} of (T, 12) mesh records under (P, 12) poses"""
    m = np.asarray(poses, np.float32).reshape(-1, 12)
    r = np.asarray(records, np.float32).reshape(-1, 12)
    out = np.zeros((m.shape[0], r.shape[0], 12), np.float32)
    with np.errstate(all="ignore"):
        for k in range(3):
            x, y, z = r[None, :, 4 * k], r[None, :, 4 * k + 1], r[None, :, 4 * k + 2]
            for j in range(3):
                m0, m1, m2, m3 = (m[:, 4 * j + c, None] for c in range(4))
                out[:, :, 4 * k + j] = ((m0 * x + m1 * y) + m2 * z) + m3
    return out


def transform_f64(poses, records):
    """(P, T, 3, 3) float64: the posed vertices in exact-enough arithmetic, and the bound's scale sum |m| |x| + |t| beside them"""
    m = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    v = np.asarray(records, np.float64).reshape(-1, 3, 4)[:, :, :3]
    out = np.einsum("pjc,tkc->ptkj", m[:, :, :3], v) + m[:, None, None, :, 3]
    mag = np.einsum("pjc,tkc->ptkj", np.abs(m[:, :, :3]), np.abs(v)) + np.abs(m[:, None, None, :, 3])
    return out, mag


def poses_any(poses, records, verts, idx):
    """(hit uint8 [P], first uint32 [P]): does any posed triangle intersect the scene, and the lowest mesh triangle that does"""
    posed = transform(poses, records)
    P, T = posed.shape[:2]
    per = tt.intersect_matrix(posed.reshape(P * T, 12), verts, idx).any(axis=1).reshape(P, T)
    hit = per.any(axis=1)
    first = np.where(hit, per.argmax(axis=1), MISS).astype(np.uint32)
    return hit.astype(np.uint8), first


def per_triangle_distance(poses, records, verts, idx, mat_ids):
    """(records uint32 [P, T, 12], d2 float32 [P, T]) of every posed triangle at max_radius = +inf (NaN d2 where nothing is found)"""
    posed = transform(poses, records)
    P, T = posed.shape[:2]
    g = posed.reshape(P * T, 12).copy()
    g[:, 3] = np.inf
    rec, d2 = tr.triangle_distance_records(g, verts, idx, mat_ids, return_d2=True)
    return rec.reshape(P, T, 12), d2.reshape(P, T)


def miss_records(P):
    rec = tr.miss_records(P)
    rec[:, 7] = MISS
    return rec


def reduce_distance(rec_inf, d2, radius):
    """pt_pose_distance_hit records as uint32 [P, 12] at max_radius = radius from per_triangle_distance's: the candidates are the
    triangles with d2 <= radius * radius (fp32; none for a NaN or negative radius), the winner the smallest (d2, mesh triangle)"""
    P, T = d2.shape
    out = miss_records(P)
    with np.errstate(all="ignore"):
        r = F(radius)
        cand = (d2 <= r * r) & bool(r >= F(0.0))
    for p in range(P):
        c = np.flatnonzero(cand[p])
        if c.size:
            t = c[np.lexsort((c, d2[p, c]))[0]]
            out[p] = rec_inf[p, t]
            out[p, 7] = t
    return out


def poses_distance(poses, records, verts, idx, mat_ids, radius=np.inf):
    rec_inf, d2 = per_triangle_distance(poses, records, verts, idx, mat_ids)
    return reduce_distance(rec_inf, d2, radius)


# ---- the meshes: name -> (vertices float32 [V, 3], indices int [T, 3]) --------------------------------------------------------------
def records_of(vertices, indices):
    """(T, 12) float32 records of a mesh, de-indexed"""
    v = np.asarray(vertices, np.float32)[np.asarray(indices).reshape(-1, 3)]
    return tt.as_records(v)


def _box(h=30.0):
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)
    # the two triangles of -y first, then -x: the faces the touching and the symmetric poses put against the floor and the x = 0 wall
    quads = [(0, 1, 5, 4), (0, 2, 3, 1), (2, 6, 7, 3), (4, 5, 7, 6), (0, 4, 6, 2), (1, 3, 7, 5)]
    idx = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(idx, np.int64)


def _strip(n):
    """n triangles in a row along x, in the plane y = 0 of the mesh, 2 units wide: a wave of 64 lanes straddles two poses at 63 and 65"""
    k = np.arange(n + 2)
    v = np.stack([k - 0.5 * (n + 1), np.zeros(n + 2), np.where(k % 2 == 0, -1.0, 1.0)], axis=1).astype(np.float32)
    idx = np.stack([k[:-2], k[1:-1], k[2:]], axis=1)
    return v, idx.astype(np.int64)


def _sphere(nlon=15, nlat=11, radius=30.0):
    """2 * nlon * (nlat - 1) triangles (300): latitude rings with the poles as degenerate-free fans"""
    v = [[0.0, -radius, 0.0]]
    for i in range(1, nlat):
        th = np.pi * i / nlat
        for j in range(nlon):
            ph = 2.0 * np.pi * j / nlon
            v.append([radius * np.sin(th) * np.cos(ph), -radius * np.cos(th), radius * np.sin(th) * np.sin(ph)])
    v.append([0.0, radius, 0.0])
    top = len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * nlon + j % nlon
    idx = [(0, ring(1, j + 1), ring(1, j)) for j in range(nlon)]
    for i in range(1, nlat - 1):
        for j in range(nlon):
            idx += [(ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i + 1, j))]
    idx += [(top, ring(nlat - 1, j), ring(nlat - 1, j + 1)) for j in range(nlon)]
    return np.array(v, np.float32), np.array(idx, np.int64)


def _coincident():
    """the sphere with triangle 200 replaced by a copy of triangle 3: whatever triangle 3 finds, 200 finds with the same bits"""
    v, idx = _sphere()
    idx = idx.copy()
    idx[200] = idx[3]
    return v, idx


def _probe(at_last, n=40):
    """n - 1 small triangles within 4 units of the origin and one needle that reaches 60 units down (-y): under the touching poses that
    rest the mesh on the floor (PROBE_POSES) the needle is the only triangle that intersects the scene and the closest one.  It is the
    last triangle or triangle 0."""
    rng = np.random.default_rng(3611)
    c = rng.uniform(-3.0, 3.0, (n - 1, 1, 3))
    small = c + rng.uniform(-1.0, 1.0, (n - 1, 3, 3))
    needle = np.array([[[-1.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, -60.0, 0.0]]])
    tris = np.concatenate([small, needle] if at_last else [needle, small]).astype(np.float32)
    return tris.reshape(-1, 3), np.arange(3 * n).reshape(-1, 3)


PROBE_POSES = (0, 2)      # of the touching set: the poses that rest the mesh on the floor


MESHES = {"single": lambda: (np.array([[-20.0, 0.0, -10.0], [25.0, 0.0, -5.0], [0.0, 0.0, 30.0]], np.float32), np.array([[0, 1, 2]], np.int64)),
          "box": _box, "strip63": lambda: _strip(63), "strip64": lambda: _strip(64), "strip65": lambda: _strip(65), "sphere": _sphere,
          "coincident": _coincident, "probe_last": lambda: _probe(True), "probe_first": lambda: _probe(False)}


def mesh(name):
    v, idx = MESHES[name]()
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(idx, np.int64)


# ---- the pose sets, sized to the Cornell box (556 x 548.8 x 559.2; the floor is y = 0 and a wall x = 0, exactly) -----------------------
# The open region: 60 units (the longest mesh's reach) from the walls, the blocks (x >= 265 or z <= 272) and the small objects.
FREE_LO, FREE_HI = np.array([70.0, 180.0, 340.0]), np.array([190.0, 400.0, 480.0])
BASE = np.array([150.0, 0.0, 400.0])        # over open floor
FINITE_RADIUS = {"identity": 10.0, "free": 5.0, "touching": 0.0, "deep": 1.0, "mixed": 40.0, "symmetric": 10.0, "nonrigid": 25.0, "bad": 50.0}
POSE_SETS = tuple(FINITE_RADIUS)


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def _rigid(rot, t):
    m = np.zeros((len(t), 3, 4))
    m[:, :, :3] = rot
    m[:, :, 3] = t
    return m


def _translations(t):
    t = np.atleast_2d(np.asarray(t, np.float64))
    return _rigid(np.broadcast_to(np.eye(3), (len(t), 3, 3)), t)


def pose_set(name, vertices, n=8):
    """(P, 12) float32 poses of set `name` for a mesh with these vertices (the touching and symmetric sets rest it on its own lowest
    point).  Fixed seeds."""
    v = np.asarray(vertices, np.float32)
    lo = v.min(axis=0).astype(np.float64)
    rng = np.random.default_rng({"free": 11, "deep": 12, "mixed": 13, "nonrigid": 14, "bad": 15}.get(name, 10))
    if name == "identity":
        m = _translations([0.0, 0.0, 0.0])
    elif name == "free":
        m = _rigid(_rotations(rng, n), rng.uniform(FREE_LO, FREE_HI, (n, 3)))
    elif name == "touching":
        # the mesh's lowest point exactly in the floor's plane, its lowest x exactly in the wall's: y + (-lo_y) is 0 in fp32
        m = _translations([BASE + [0.0, -lo[1], 0.0], [-lo[0], 200.0, 400.0], BASE + [16.0, -lo[1], 32.0], [-lo[0], 300.0, 450.0]])
    elif name == "deep":
        t = np.array([[0.0, 250.0, 400.0], [150.0, 0.0, 420.0], [180.0, 90.0, 160.0], [368.0, 200.0, 350.0], [100.0, 548.8, 300.0], [278.0, 270.0, 559.2]])
        m = _rigid(_rotations(rng, len(t)), t)
    elif name == "mixed":
        t = rng.uniform(FREE_LO, FREE_HI, (n, 3))
        t[1::2] = np.array([[0.0, 250.0, 400.0], [150.0, 10.0, 420.0], [200.0, 100.0, 150.0], [556.0, 300.0, 300.0]])[:n // 2]
        m = _rigid(_rotations(rng, n), t)
    elif name == "symmetric":
        # 8 units from the floor and 8 units from the x = 0 wall, exactly: small whole numbers throughout
        m = _translations([[8.0 - lo[0], 8.0 - lo[1], 400.0], [16.0 - lo[0], 16.0 - lo[1], 300.0]])
    elif name == "nonrigid":
        scale = np.diag([1.5, 0.5, 2.0])
        shear = np.array([[1.0, 0.75, 0.0], [0.0, 1.0, 0.25], [0.0, 0.0, 1.0]])
        mirror = np.diag([-1.0, 1.0, 1.0])
        flat = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.0, 1.0]])      # singular: everything lands in one plane
        line = np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])      # rank 1: a segment
        mats = np.array([scale, shear, mirror, flat, line, np.zeros((3, 3))])
        t = np.array([[150.0, 30.0, 400.0], [120.0, 250.0, 420.0], [20.0, 200.0, 400.0], [150.0, 0.0, 400.0], [150.0, 12.0, 400.0], [150.0, 20.0, 430.0]])
        m = _rigid(mats, t)
    elif name == "bad":
        good = _rigid(_rotations(rng, 7), np.concatenate([rng.uniform(FREE_LO, FREE_HI, (4, 3)), [[0.0, 250.0, 400.0], [150.0, 10.0, 420.0], [150.0, 100.0, 400.0]]]))
        m = good.copy()
        m[1, 0, 3] = np.nan                 # a NaN in the translation
        m[3, 1, 1] = np.inf                 # an infinity in the matrix
        m[5] = _rigid(np.eye(3)[None] * 3e38, [[3e38, 3e38, 3e38]])[0]      # finite entries whose transform overflows
    else:
        raise KeyError(name)
    return as_poses(m)


# The (mesh, pose set) pairs the GPU tests run: every mesh and every set at least once.
CASES = (("single", "identity"), ("single", "touching"), ("single", "mixed"), ("box", "identity"), ("box", "free"), ("box", "touching"), ("box", "deep"),
         ("box", "mixed"), ("box", "symmetric"), ("box", "nonrigid"), ("box", "bad"), ("strip63", "mixed"), ("strip64", "mixed"), ("strip65", "mixed"),
         ("strip65", "bad"), ("sphere", "mixed"), ("sphere", "symmetric"), ("coincident", "touching"), ("coincident", "free"), ("probe_last", "touching"),
         ("probe_last", "free"), ("probe_first", "touching"), ("probe_first", "free"))
CASE_POSES = {("coincident", "free"): 2, ("probe_last", "free"): 4, ("probe_first", "free"): 4}      # the brute force is paid per posed triangle


def case(mesh_name, set_name):
    """(records [T, 12], poses [P, 12], finite radius)"""
    v, idx = mesh(mesh_name)
    return records_of(v, idx), pose_set(set_name, v)[:CASE_POSES.get((mesh_name, set_name))], FINITE_RADIUS[set_name]


@functools.lru_cache(maxsize=None)
def cornell_scene():
    """(vertices, indices, material ids) of the Cornell box fixture; cornell_box_diffuse.obj shares its geometry"""
    import acgpathtracing_amd as pt
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj"))
    return obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()


@functools.lru_cache(maxsize=None)
def cornell_reference(mesh_name, set_name):
    """The brute force of one case on the Cornell box, computed once per process, shared and never written: a dict of records, poses,
    radius, hit, first, rec_inf and d2 (per_triangle_distance's), out_inf and out_r (the pose records at +inf and at the radius)"""
    verts, idx, mats = cornell_scene()
    records, poses, radius = case(mesh_name, set_name)
    hit, first = poses_any(poses, records, verts, idx)
    rec_inf, d2 = per_triangle_distance(poses, records, verts, idx, mats)
    got = {"records": records, "poses": poses, "radius": radius, "hit": hit, "first": first, "rec_inf": rec_inf, "d2": d2,
           "out_inf": reduce_distance(rec_inf, d2, np.inf), "out_r": reduce_distance(rec_inf, d2, radius)}
    for a in got.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return got
