"""The scenes on which the three query stages (pt_query_closest / pt_query_any, pt_ao_points / pt_ao_image, pt_query_nearest) are held
to their references beyond the Cornell fixtures: every builder, a tree of ~96 levels, one-node trees, no triangles, flat, collapsed and
zero-area geometry, four magnitudes.  A plain module: the scene table (functions returning (verts[n, 4] f32, idx[t, 3] u32, mat_ids[t]
u32, materials)), the ray, point and AO-point sets of every scene, the references (all on the CPU: the oracle's brute force,
tests/query_ref.py, tests/ao_ref.py, tests/nearest_ref.py), the table of which conditions hold for which scene, and the device-side
helpers of the three existing GPU test files with 64 guard bytes of 0xCD behind every output.

tests/test_query_scenes_host.py holds the sets to their conditions with the references alone; tests/test_gpu_query_scenes.py holds the
GPU to the references."""
import ctypes as C
import functools
import os
import tempfile
import types

import numpy as np

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import ao_ref as ar
import denoise_ref as dr
import nearest_ref as nr
import query_ref as qr
import test_gpu_ao as gpu_ao
import test_gpu_nearest as gpu_nearest
import test_gpu_query as gpu_query
from scene_utils import make_params
from test_gpu_refit_edges import BOX, _Arrays, _Ctx, _box, _deformations, _object_tris, _refit, _stress          # noqa: F401  (_Ctx, _refit, _Arrays: for the GPU file)

F = np.float32
MISS = 0xFFFFFFFF
GUARD = gpu_nearest.GUARD
K_AO = 4                                 # rays per AO point
BIG = 20000                              # from this many triangles on a set has 257 queries: one workgroup plus one lane
POINT = (278.0, 274.0, 280.0)            # where scene 7 collapses to


# ---- the scene table ---------------------------------------------------------------------------------------------------------------

def _frozen(v, idx, ids, mats):
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 4)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    ids = np.ascontiguousarray(ids, np.uint32)
    for a in (v, idx, ids):
        a.setflags(write=False)
    return v, idx, ids, mats


@functools.lru_cache(maxsize=None)
def box():
    return _frozen(*_box())


@functools.lru_cache(maxsize=None)
def sphere():
    """One icosphere of 20 480 triangles in the Cornell shell"""
    path = os.path.join(tempfile.mkdtemp(prefix="query_scenes_"), "sphere.obj")
    return _frozen(*_stress(path, n_spheres=1, subdiv=5))


@functools.lru_cache(maxsize=None)
def copies(lifted=False):
    """20 000 copies of one triangle, each with its own vertices; lifted: copy i moved i * 1e-3 along the normal"""
    n = 20000
    tri = np.array([[100, 100, 300, 0], [400, 100, 300, 0], [100, 400, 300, 0]], np.float32)
    v = np.ascontiguousarray(np.tile(tri, (n, 1)), np.float32)
    if lifted:
        v[:, 2] += (np.repeat(np.arange(n), 3) * 1e-3).astype(np.float32)
    return _frozen(v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), np.zeros(n, np.uint32), box()[3])


@functools.lru_cache(maxsize=None)
def triangles(n_tris):
    tris = np.array([[100, 100, 300, 0], [400, 120, 310, 0], [150, 400, 290, 0],
                     [200, 50, 400, 0], [450, 300, 420, 0], [300, 480, 380, 0]], np.float32)
    mats = box()[3]
    return _frozen(tris[:3 * n_tris], np.arange(3 * n_tris, dtype=np.uint32).reshape(-1, 3), np.arange(n_tris, dtype=np.uint32) % len(mats), mats)


@functools.lru_cache(maxsize=None)
def empty():
    """No triangles: the box's vertices and materials, an empty index buffer"""
    v, _, _, mats = box()
    return _frozen(v, np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32), mats)


@functools.lru_cache(maxsize=None)
def flat():
    v, idx, ids, mats = box()
    vn = v.copy()
    vn[:, 1] = F(200.0)
    return _frozen(vn, idx, ids, mats)


@functools.lru_cache(maxsize=None)
def point():
    v, idx, ids, mats = box()
    vn = v.copy()
    vn[:, :3] = np.float32(POINT)
    return _frozen(vn, idx, ids, mats)


@functools.lru_cache(maxsize=None)
def zero_area():
    """Every other triangle of the box and the lamp's first lose their area: the second vertex is moved onto the first (the construction
    of test_gpu_refit_edges.test_half_the_triangles_zero_area)"""
    v, idx, ids, mats = box()
    vn = v.copy()
    lamp = np.flatnonzero(_object_tris(BOX, idx, "lamp"))
    for t in sorted(set(range(0, len(idx), 2)) | {int(lamp[0])}):
        vn[idx[t, 1], :3] = vn[idx[t, 0], :3]
    return _frozen(vn, idx, ids, mats)


def zero_area_mask(v, idx):
    t = v[:, :3][idx.astype(np.int64)]
    c = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return np.linalg.norm(c, axis=1) == 0


@functools.lru_cache(maxsize=None)
def magnitude(s, off):
    v, idx, ids, mats = box()
    vn = v.copy()
    vn[:, :3] = vn[:, :3] * F(s) + F(off)
    return _frozen(vn, idx, ids, mats)


SCALED = (8.0, (-1234.5, 333.25, 777.0))          # the "scale" deformation of test_gpu_update._deformations


@functools.lru_cache(maxsize=None)
def scaled():
    v, idx, ids, mats = box()
    return _frozen(_deformations(v)["scale"], idx, ids, mats)


MAGNITUDES = {"x1e6": (1e6, 0.0), "x1e-6": (1e-6, 0.0), "plus1e7": (1.0, 1e7), "x2^-7plus4096": (2.0 ** -7, 4096.0)}

# which conditions of the host test hold for which scene ("Conditions" in the module docstring of tests/test_query_scenes_host.py)
RAY_SHARES, ALL_FOUND, RADIUS_SHARES, DISTINCT, ZERO_AREA_WINNERS, AO_PARTIAL = "ray shares", "all found", "radius shares", "distinct winners", "zero-area winners", "ao partial"
_USUAL = frozenset({RAY_SHARES, ALL_FOUND, RADIUS_SHARES, DISTINCT})


class Scene:
    """name; arrays(): the scene; xform: the map x -> s x + off of the Cornell box it is (the camera follows it), or None; sets_of: the
    scene whose box the sets are generated from, if not its own (a scene without a box of its own); ao_of: the scene whose surfaces
    the AO points lie on, if not its own; thin: a scene without a volume, which the rays from inside the scene box cannot hit (they
    start in its plane): three more aimed sets stand in for them; conditions: which hold"""

    def __init__(self, name, arrays, conditions, xform=None, sets_of=None, box_shaped=False, ao="centroids", ao_of=None, radii=None, thin=False):
        self.name, self._arrays, self.conditions, self.xform = name, arrays, frozenset(conditions), xform
        self.sets_of, self.box_shaped, self.ao, self.ao_of, self.radii, self.thin = sets_of, box_shaped, ao, ao_of, radii or {}, thin

    def arrays(self):
        return self._arrays()

    def set_arrays(self):
        return (SCENES[self.sets_of] if self.sets_of else self).arrays()

    @property
    def n_queries(self):
        return 257 if len(self.arrays()[1]) >= BIG else 1000


SCENES = {s.name: s for s in [
    Scene("box", box, _USUAL | {AO_PARTIAL}, box_shaped=True, ao="occlusion"),
    Scene("sphere", sphere, _USUAL | {AO_PARTIAL}, box_shaped=True, ao="occlusion"),
    Scene("copies", copies, _USUAL - {DISTINCT}, thin=True),                     # 20 000 exact ties: every winner is triangle 0
    Scene("copies_lifted", lambda: copies(True), _USUAL),
    Scene("one_triangle", lambda: triangles(1), _USUAL - {DISTINCT}, thin=True),
    Scene("two_triangles", lambda: triangles(2), _USUAL - {DISTINCT}, thin=True),
    # nothing to hit or find; the sets are the box's
    Scene("empty", empty, (), sets_of="box", box_shaped=False),
    Scene("flat", flat, _USUAL | {AO_PARTIAL}, ao="lifted", thin=True),
    # a point: no ray hits it, one winner; the sets are the box's, the radii a share of the box's diagonal that reaches the point from some
    Scene("point", point, {ALL_FOUND, RADIUS_SHARES}, sets_of="box", radii={"surface": 0.3, "inside": 0.3, "features": 0.3, "wall_planes": 0.4, "around": 0.4}),
    # the AO points lie on the box's own surfaces, half of which are gone here: centroids of this scene's triangles see next to nothing
    Scene("zero_area", zero_area, _USUAL | {ZERO_AREA_WINNERS, AO_PARTIAL}, box_shaped=True, ao="occlusion", ao_of="box"),
    Scene("scaled", scaled, _USUAL, xform=SCALED, box_shaped=True),      # what the forced variant is refitted to
] + [
    # at 1e-6 the scene is 5.6e-4 across and pt_render_features' camera rays start at t = 0.01: no pixel sees it, no pt_ao_image case
    Scene(name, functools.partial(magnitude, s, off), _USUAL, xform=(s, (off, off, off)), box_shaped=name != "x1e-6")
    for name, (s, off) in MAGNITUDES.items()
]}

# (scene, build mode, pt_set_tuning's variant or None): the matrix of tests/test_gpu_query_scenes.py.  None is the default variant
# (chosen per scene), 1 the fp32 nodes, 7 the fp16 centre / half-extent nodes forced where the default would not take them.
CASES = ([("box", m, None) for m in (0, 1, 2)] + [("box", 2, 1)] +
         [("sphere", m, None) for m in (0, 1, 2)] +
         [(name, 2, t) for name in ("copies", "copies_lifted") for t in (None, 1)] +
         [(name, None, t) for name in ("one_triangle", "two_triangles", "flat") for t in (None, 1)] +
         [("point", None, None), ("zero_area", None, None), ("zero_area", None, 7)] +
         [(name, None, None) for name in MAGNITUDES] + [(name, None, 1) for name in ("plus1e7", "x2^-7plus4096")])

# The node format a scene holds under the default variant where that is not the fp16 centre / half-extent nodes: the variant is chosen
# per scene, and geometry finer than the fp16 planes gets the fp32 nodes (pt_bvh_info.half_area_ratio / half_box_inflation).
DEFAULT_FORMAT = {"zero_area": 0}           # half_box_inflation 16: boxes around collapsed edges

# the targets of the refits into and out of the hard states (scene 11): the box refitted to each, and back
REFIT_TARGETS = ("flat", "point", "zero_area") + tuple(MAGNITUDES)


def camera(scene, w=97, h=61):
    """(eye, U, V, W) of the Cornell camera mapped with the scene, as tuples of Python floats"""
    q = params(scene, w, h)
    return tuple((a.x, a.y, a.z) for a in (q.cameraEye, q.cameraU, q.cameraV, q.cameraW))


def params(scene, w, h, handle=0):
    """PathTraceParams of a w x h view whose camera follows the scene's map (test_gpu_refit_edges._Ctx._params)"""
    shim = types.SimpleNamespace(handle=lambda: handle)
    return _Ctx._params(shim, w, h, 1, scene.xform)


# ---- the sets ----------------------------------------------------------------------------------------------------------------------

def _extent(v, idx):
    """(lo, hi, centre, scale): scale is the box's diagonal, or where the box is a point a thousandth of its distance from the origin"""
    lo, hi = nr.scene_box(v, idx)
    ext = hi - lo
    diag = F(np.sqrt(float((ext * ext).sum())))
    c = F(0.5) * (lo + hi)
    if not diag > 0:
        diag = F(max(1e-3 * float(np.abs(c).max()), 1e-30))
    return lo, hi, c, diag


def _thin(a, n):
    """n of a's rows, evenly spread (the first n of a camera set would be one edge of the image)"""
    return a if a.shape[0] <= n else np.ascontiguousarray(a[np.linspace(0, a.shape[0] - 1, n).astype(np.int64)])


def _unit(rng, n):
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return d / np.sqrt((d * d).sum(axis=1, keepdims=True))


def aimed_rays(v, idx, n, seed=606):
    """From 0.6 .. 2 scales off the centre towards random points of random triangles: a third aimed exactly (half of those end before
    their target or just behind it), the rest scattered around their aim by up to a quarter of their length.  Works on boxes without
    a volume, where query_ref's sets from inside the box lie in the geometry's own plane."""
    lo, hi, c, scale = _extent(v, idx)
    rng = np.random.default_rng(seed)
    tri = v[:, :3][idx[rng.integers(0, idx.shape[0], n)].astype(np.int64)]
    b = rng.random((n, 2)).astype(np.float32)
    fold = b.sum(axis=1) > 1.0
    b[fold] = F(1.0) - b[fold]
    target = tri[:, 0] + b[:, 0:1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:2] * (tri[:, 2] - tri[:, 0])
    o = (c + _unit(rng, n) * (scale * rng.uniform(0.6, 2.0, (n, 1)).astype(np.float32))).astype(np.float32)
    d = (target - o).astype(np.float32)
    scatter = np.arange(n) % 3 != 0
    length = np.sqrt((d * d).sum(axis=1, keepdims=True))
    d[scatter] += (_unit(rng, n) * length * rng.uniform(0.0, 0.25, (n, 1)).astype(np.float32))[scatter]
    tmax = np.full(n, np.inf, np.float32)
    short = np.arange(n) % 6 == 0
    tmax[short] = rng.uniform(0.5, 1.5, n).astype(np.float32)[short]          # t is in units of |d|: the target is at t = 1
    return qr._rays(o, d, F(0.0), tmax)


RAY_SETS = qr.RAY_SETS + ("aimed",)
THIN_RAY_SETS = ("camera", "aimed", "aimed_2", "aimed_3", "aimed_4", "outside")
AIMED_SEEDS = {"aimed": 606, "aimed_2": 616, "aimed_3": 626, "aimed_4": 636}


def ray_set_names(name):
    return THIN_RAY_SETS if SCENES[name].thin else RAY_SETS


@functools.lru_cache(maxsize=None)
def ray_sets(name):
    """set name -> rays [n, 8] of the scene, from its own box (or the box of the scene it borrows)"""
    s = SCENES[name]
    v, idx = s.set_arrays()[:2]
    out = {}
    for k in ray_set_names(name):
        r = aimed_rays(v, idx, qr.SET_SIZE, AIMED_SEEDS[k]) if k in AIMED_SEEDS else qr.ray_set(k, v, idx, camera(s))
        out[k] = np.ascontiguousarray(_thin(r, s.n_queries), np.float32)
        out[k].setflags(write=False)
    return out


def around_points(v, idx, n, seed=707):
    """Vertices, edge midpoints and centroids of random triangles, pushed off them by 0, 1e-3, 0.05, 1 and 100 scales in a random
    direction, a fifth each: points exactly on a vertex, an edge and the face, points beside them, points far away"""
    lo, hi, c, scale = _extent(v, idx)
    rng = np.random.default_rng(seed)
    feats = nr.feature_points(v, idx)
    p = feats[rng.integers(0, feats.shape[0], n)]
    step = np.array([0.0, 1e-3, 0.05, 1.0, 100.0], np.float32)[np.arange(n) % 5]
    return (p + _unit(rng, n) * (step * scale)[:, None]).astype(np.float32)


POINT_SETS = nr.POINT_SETS + ("around",)


def zero_area_features(v, idx):
    """The distinct vertices and edge midpoints of the zero-area triangles: the points whose winner may be one of them"""
    t = v[:, :3][idx[zero_area_mask(v, idx)].astype(np.int64)]
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    return np.unique(np.concatenate([a, b, c, F(0.5) * (a + b), F(0.5) * (b + c), F(0.5) * (c + a)]).astype(np.float32), axis=0)


@functools.lru_cache(maxsize=None)
def point_sets(name):
    """set name -> (points [n, 3], finite radius) of the scene.  "surface": first hits, by nearest_ref's float64 brute force, of camera
    rays mapped with the scene."""
    s = SCENES[name]
    v, idx = s.set_arrays()[:2]
    lo, hi, c, scale = _extent(v, idx)
    out = {}
    for k in POINT_SETS:
        if k == "around":
            p, r = around_points(v, idx, nr.SET_SIZE), F(0.05) * scale
        else:
            p, r = nr.point_set(k, v, idx, camera(s)), nr.set_radius(k, v, idx)
        if k in s.radii:
            r = F(s.radii[k]) * scale
        out[k] = (np.ascontiguousarray(_thin(p, s.n_queries), np.float32), F(r))
        out[k][0].setflags(write=False)
    if ZERO_AREA_WINNERS in s.conditions:
        out["zero_area_features"] = (zero_area_features(v, idx), F(0.0))
    return out


def ao_parameters(name):
    """radius a quarter and bias a thousandth of the diagonal of the scene's own box (of the box its sets come from where it has none)"""
    v, idx = SCENES[name].set_arrays()[:2]
    return ar.gpu_test_parameters(v, idx)


@functools.lru_cache(maxsize=None)
def ao_points(name):
    """(P, N) [n, 3] of the scene.  "occlusion": ao_ref.occlusion_points, random points on random triangles.  "centroids": the centroids
    of random triangles with their face normals, normalize(cross(e1, e2)) in fp32 — a zero-area triangle gives a NaN normal, a point
    that is no surface — and a few more no-surface points.  "lifted" (the flat scene, where no ray from the plane can meet the plane
    again): the centroids a twentieth of the diagonal above and below the plane, the normal tilted back towards it."""
    s = SCENES[name]
    v, idx = (SCENES[s.ao_of] if s.ao_of else s).set_arrays()[:2]
    n = s.n_queries
    if s.ao == "occlusion":
        P, N = ar.occlusion_points(v, idx, camera(s))
        P, N = _thin(P, n).copy(), _thin(N, n).copy()
    else:
        rng = np.random.default_rng(808)
        t = v[:, :3][idx[rng.integers(0, idx.shape[0], n)].astype(np.int64)]
        e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        with np.errstate(all="ignore"):
            N = (c * (F(1.0) / np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]))[:, None]).astype(np.float32)
        P = ((t[:, 0] + t[:, 1] + t[:, 2]) * F(1.0 / 3.0)).astype(np.float32)
        if s.ao == "lifted":
            scale = _extent(v, idx)[3]
            side = np.where(np.arange(n) % 2 == 0, F(1.0), F(-1.0))
            P[:, 1] += side * F(0.05) * scale
            tilt = _unit(rng, n)
            tilt[:, 1] = -side
            N = (tilt / np.sqrt((tilt * tilt).sum(axis=1, keepdims=True))).astype(np.float32)
    P[5], N[17], N[40, 2] = F(np.nan), F(0.0), F(np.inf)               # no surface: a NaN point, a zero normal, an infinite component
    for a in (P, N):
        a.setflags(write=False)
    return P, N


# ---- the references ----------------------------------------------------------------------------------------------------------------
_cache = {}


def _oracle_scene(oracle, name):
    v, idx, ids, mats = SCENES[name].arrays()
    return oracle.scene(v, idx.reshape(-1), ids, mats)


def ray_reference(oracle, name):
    """set name -> (rays, pt_hit records [n, 8] u32, any-hit [n] bool) by the oracle's brute force and query_ref.hit_records"""
    if ("rays", name) not in _cache:
        v, idx, ids, mats = SCENES[name].arrays()
        out = {}
        sc = _oracle_scene(oracle, name) if len(idx) else None
        try:
            for k, rays in ray_sets(name).items():
                if sc is None:
                    t, prim, hit = np.full(len(rays), -1, np.float32), np.full(len(rays), MISS, np.uint32), np.zeros(len(rays), bool)
                else:
                    t, prim = sc.trace_closest(rays, use_bvh=False)
                    hit = sc.trace_any(rays, use_bvh=False) != 0
                rec = qr.hit_records(rays, t, prim, v, idx, ids)
                rec.setflags(write=False)
                out[k] = (rays, rec, hit & qr.traceable(rays))
        finally:
            if sc is not None:
                sc.close()
        _cache[("rays", name)] = out
    return _cache[("rays", name)]


def any_hits(oracle, name, rays):
    """The oracle's brute-force any-hit on rays that may hold non-rays (those are no hit)"""
    ok = qr.traceable(rays)
    if len(SCENES[name].arrays()[1]) == 0:
        return np.zeros(len(rays), bool)
    send = np.ascontiguousarray(rays, np.float32).copy()
    send[~ok] = (0, 0, 0, 0, 0, 1, 0, 1)
    sc = _oracle_scene(oracle, name)
    try:
        return (sc.trace_any(send, use_bvh=False) != 0) & ok
    finally:
        sc.close()


def ao_expected(oracle, name, P, N, p, seed=None):
    """(visible [n] u32, ao bits [n] u32) of the points by ao_ref's rays under the oracle's brute-force any-hit"""
    disk = pt.aoSamples(K_AO)
    r = ar.rays(P, N, disk, p if seed is None else dict(p, seed=seed))
    vis = ar.counts(any_hits(oracle, name, r), r, K_AO)
    return vis, ar.ao_value(vis, K_AO).view(np.uint32)


def ao_reference(oracle, name):
    """(P, N, parameters, visible, ao bits)"""
    if ("ao", name) not in _cache:
        P, N = ao_points(name)
        p = ao_parameters(name)
        _cache[("ao", name)] = (P, N, p) + ao_expected(oracle, name, P, N, p)
    return _cache[("ao", name)]


def _chunk(n_tris):
    return max(1, min(2048, 2_000_000 // max(n_tris, 1)))


def nearest_reference(name):
    """set name -> (points [n, 3], radius, records at +inf, records at the radius) by nearest_ref's brute force"""
    if ("nearest", name) not in _cache:
        v, idx, ids, _ = SCENES[name].arrays()
        out = {}
        for k, (pts, r) in point_sets(name).items():
            recs = [nr.nearest_records(nr.with_radius(pts, rad), v, idx, ids, chunk=_chunk(len(idx))) for rad in (np.inf, r)]
            for a in recs:
                a.setflags(write=False)
            out[k] = (pts, r, recs[0], recs[1])
        _cache[("nearest", name)] = out
    return _cache[("nearest", name)]


def scene_magnitude(name):
    """S: the largest coordinate magnitude of the scene box (what nearest_abs_term is taken from)"""
    v, idx = SCENES[name].arrays()[:2]
    if len(idx) == 0:
        return 0.0
    lo, hi = nr.scene_box(v, idx)
    return float(max(np.abs(lo).max(), np.abs(hi).max()))


def f64_distance(name, pts):
    """The float64 brute force: nearest_ref.closest_f64 over all triangles, the minimum per point"""
    v, idx = SCENES[name].arrays()[:2]
    t = v[:, :3][idx.astype(np.int64)]
    best = np.full(len(pts), np.inf)
    step = _chunk(len(idx))
    for a in range(0, len(pts), step):
        d, _ = nr.closest_f64(pts[a:a + step, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2])
        best[a:a + step] = np.where(np.isnan(d), np.inf, d).min(axis=1)
    return best


def dead_share(name, pts):
    """The share of a set's pairs of a point and a triangle WITH an area whose fp32 d2 is NaN or infinite: where the statement
    overflows.  (A triangle without area gives a NaN in the region of its collapsed edge, 0 / 0, by the contract: no candidate.)  Every
    fourth point of the set: it is a share."""
    v, idx = SCENES[name].arrays()[:2]
    idx = idx[~zero_area_mask(v, idx)]
    if len(idx) == 0:
        return 0.0
    v0, e1, e2 = nr.records_of_scene(v, idx)
    pts = pts[::4]
    dead = 0
    step = _chunk(len(idx))
    for a in range(0, len(pts), step):
        d2 = nr.closest_on_triangle(pts[a:a + step, None, :], v0[None], e1[None], e2[None])[0]
        dead += int((~np.isfinite(d2)).sum())
    return dead / float(len(pts) * len(idx))


# The largest deviation of the fp32 reference's distance from the float64 brute force over a scene's sets (at +inf radius, every point
# whose fp32 winner has a finite d2), relative to the scene's S, as tests/test_query_scenes_host.py measures and prints it.  The host test
# holds the reference to four times these.
F64_DEVIATION = {"box": 1.432e-05, "sphere": 1.596e-05, "copies": 8.159e-06, "copies_lifted": 8.638e-06, "one_triangle": 7.983e-06,
                 "two_triangles": 7.881e-06, "flat": 1.193e-05, "point": 3.365e-05, "zero_area": 1.760e-05, "x1e6": 1.395e-05, "scaled": 1.220e-05,
                 "x1e-6": 1.826e-05, "plus1e7": 1.354e-07, "x2^-7plus4096": 1.432e-07}


# ---- device-side helpers: the three GPU test files' own, with 64 bytes of 0xCD checked behind every output ----------------------

def state_of(c, scene=None, w=97, h=61):
    """What the helpers of the existing GPU tests take for a PathTracerState: .context and .params (the view mapped with the scene)"""
    p = params(scene, w, h, c.handle()) if scene is not None else None
    return types.SimpleNamespace(context=c.ctx, params=p)


def _L():
    return _native.hip()


def _arm(state, ptr):
    assert _L().pt_device_memset(state.context, ptr, 0xCD, GUARD) == 0


def _intact(state, ptr, what):
    g = np.zeros(GUARD // 4, np.uint32)
    assert _L().pt_copy_to_host(state.context, g.ctypes.data, ptr, GUARD) == 0
    assert (g == 0xCDCDCDCD).all(), "written past the end of " + what


DevicePoints = gpu_nearest._DevicePoints          # carries its guard already


class DeviceRays(gpu_query._DeviceRays):
    """test_gpu_query's, its three buffers two rays longer than the rays: the room for the guards"""

    def __init__(self, state, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        super().__init__(state, np.concatenate([rays, np.zeros((GUARD // 32, 8), np.float32)]))
        self.n = rays.shape[0]

    def closest(self):
        _arm(self.state, self.bufs[1] + self.n * 32)
        rec = super().closest()
        _intact(self.state, self.bufs[1] + self.n * 32, "the hit records")
        return rec

    def any(self):
        _arm(self.state, self.bufs[2] + self.n)
        occ = super().any()
        _intact(self.state, self.bufs[2] + self.n, "occluded")
        return occ


class DeviceAO(gpu_ao._Device):
    """test_gpu_ao's: its output buffers are as long as the input records (32 or 16 bytes a point against 4), so the guards fit"""

    def _guarded(self, n, call):
        assert n * 4 + GUARD <= max(self.rec.nbytes, 32)
        for b in self.bufs[1:]:
            _arm(self.state, b + n * 4)
        out = call()
        for b, what in zip(self.bufs[1:], ("visible", "ao")):
            _intact(self.state, b + n * 4, what)
        return out

    def points(self, n, disk, ap, **kw):
        return self._guarded(n, lambda: super(DeviceAO, self).points(n, disk, ap, **kw))

    def image(self, disk, ap, **kw):
        n = int(self.state.params.width) * int(self.state.params.height)
        return self._guarded(n, lambda: super(DeviceAO, self).image(disk, ap, **kw))


def check_shares(name, rays, nearest, ao):
    """The conditions of tests/test_query_scenes_host.py on what a GPU test compares: rays, nearest and ao are ray_reference's,
    nearest_reference's and ao_reference's values (or the GPU's own outputs in the same layout)"""
    cond = SCENES[name].conditions
    hit = np.concatenate([rec[:, 1] != MISS for _, rec, _ in rays.values()])
    assert (hit.mean() >= 0.25 and (~hit).mean() >= 0.10) if RAY_SHARES in cond else not hit.any(), (name, hit.mean())
    found_inf = np.concatenate([r[2][:, 1] != MISS for r in nearest.values()])
    found_r = np.concatenate([r[3][:, 1] != MISS for r in nearest.values()])
    winners = np.unique(np.concatenate([r[i][:, 1] for r in nearest.values() for i in (2, 3)]))
    winners = winners[winners != MISS]
    assert found_inf.all() if ALL_FOUND in cond else not found_inf.any(), name
    assert RADIUS_SHARES not in cond or (found_r.mean() >= 0.2 and (~found_r).mean() >= 0.1), (name, found_r.mean())
    assert DISTINCT not in cond or winners.size >= 8, (name, winners.size)
    if ZERO_AREA_WINNERS in cond:
        zero = zero_area_mask(*SCENES[name].arrays()[:2])
        assert sum(int(zero[r[i][r[i][:, 1] != MISS, 1]].sum()) for r in nearest.values() for i in (2, 3)) >= 20
    vis = ao[3]
    assert AO_PARTIAL not in cond or ((vis > 0) & (vis < K_AO)).mean() >= 0.10, name


def ao_args(p, seed=None):
    return gpu_ao._params(pt.aoSamples(K_AO), p, seed=seed)
