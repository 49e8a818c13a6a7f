"""pt_update_vertices(PT_UPDATE_REFIT) where its code paths are thin in tests/test_gpu_update.py: every build mode and the long chains of
hashed pairing, a scene large enough that each thread of refit.hip k_rf_leaves takes several leaf slots (its grid stride and per-block
scene-box reduction), the one-triangle path k_rf_single, flat, collapsed, zero-area and extreme-magnitude targets, an unreferenced vertex
that only moves pad_abs, the arrays derived from the old boxes (node formats, four-wide records) across variant switches, and material
edits interleaved with refits.

Unless a case says otherwise, after each refit: the queries (closest and any-hit, random and adversarial rays of the new vertices) equal a
fresh pt_set_scene of the same arrays bit for bit and equal the CPU oracle (brute force, or its own BVH plus a brute-force sample on the
largest scene); pt_get_bvh_info.scene_lo / hi equal the fresh build's and tests/refit_ref.py's; accumulation, frame buffer and both
feature buffers equal the fresh context's in light modes 0 and 1; a refit back to the original vertices restores queries, images and
scene box bit for bit and the fp16 ratios to rel=1e-5."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

import acgpathtracing_amd as pt
import refit_ref
import test_gpu_update as upd_tests
from acgpathtracing_amd import _native
from scene_utils import adversarial_rays, make_params, random_rays
from test_gpu_update import BOX, _deformations, _object_vertices

pytestmark = pytest.mark.gpu

IEEE, FAST = _native.MATH_IEEE, _native.MATH_FAST
BOTH_MATHS, BOTH_LIGHTS = (IEEE, FAST), (0, 1)
BRUTE_LIMIT = 25000           # triangles up to which the oracle answers every ray by brute force
MISS = 0xFFFFFFFF


def _table(mats):
    return (_native.Material * len(mats))(*[_native.Material.from_buffer_copy(m) for m in mats])


class _Arrays:
    """Stands in for a TinyObjWrapper: a scene from raw arrays."""

    def __init__(self, idx, ids, mats):
        self.idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        self.ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        self.mats = mats if isinstance(mats, C.Array) else _table(mats)

    def getIndexBuffer(self):
        return self.idx

    def getMaterialIndices(self):
        return self.ids

    def getMaterials(self):
        return self.mats

    def as_scene(self):
        """What _oracle_answers reads of a context."""
        return types.SimpleNamespace(idx=self.idx, mid=self.ids, mats=self.mats)


class _Ctx(upd_tests._Ctx):
    """test_gpu_update's context, plus: a build mode set before every pt_set_scene, a constructor from raw arrays, material edits, the
    ray-stream kernel, a render whose camera follows an affine map of the scene, and pt_temporal_blend."""

    def __init__(self, obj, verts, build_mode=None, **kw):
        self.build_mode = build_mode
        super().__init__(obj, verts, **kw)

    @classmethod
    def from_arrays(cls, verts, idx, ids, mats, **kw):
        return cls(_Arrays(idx, ids, mats), verts, **kw)

    def set_scene(self, verts):
        if self.build_mode is not None:
            assert self.L.pt_set_build_mode(self.ctx, self.build_mode) == 0
        super().set_scene(verts)

    def modes(self, math, light):
        assert self.L.pt_set_math_mode(self.ctx, math) == 0 and self.L.pt_set_light_mode(self.ctx, light) == 0

    def update_materials(self, mats, ids=None):
        t = _table(mats)
        i = None if ids is None else np.ascontiguousarray(ids, np.uint32)
        rc = self.L.pt_update_materials(self.ctx, C.addressof(t), len(t), None if i is None else i.ctypes.data, 0 if i is None else i.size, None)
        assert rc == 0, self.err()
        self.mats = t
        if i is not None:
            self.mid = i

    def bench(self, rays, fmt):
        n = rays.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32); ms = C.c_float()
        assert self.L.pt_bench_traversal(self.ctx, rays.ctypes.data, n, 1, fmt, t.ctypes.data, prim.ctypes.data, C.byref(ms), None) == 0, self.err()
        return t.view(np.uint32), prim

    def _alloc(self, sizes):
        out = []
        for nbytes in sizes:
            p = C.c_void_p()
            assert self.L.pt_device_malloc(self.ctx, C.byref(p), nbytes) == 0
            assert self.L.pt_device_memset(self.ctx, p, 0, nbytes) == 0
            out.append(p.value)
        return out

    def _get(self, p, nbytes):
        a = np.zeros(nbytes // 4, np.uint32)
        assert self.L.pt_copy_to_host(self.ctx, a.ctypes.data, p, nbytes) == 0
        return a

    def _params(self, w, h, spp, xform):
        q = make_params(w, h, spp, 6, True, True)
        if xform is not None:          # the camera of the scene mapped by x -> s x + off: the same rays, in the mapped scene
            s, off = xform
            e = q.cameraEye
            q.cameraEye = pt.Float3(*(float(np.float32(x) * np.float32(s) + np.float32(o)) for x, o in zip((e.x, e.y, e.z), off)))
            for name in ("cameraU", "cameraV", "cameraW"):
                a = getattr(q, name)
                setattr(q, name, pt.Float3(*(float(np.float32(x) * np.float32(s)) for x in (a.x, a.y, a.z))))
        q.handle = self.handle()
        return q

    def render(self, w=64, h=48, spp=8, frames=2, handle=None, xform=None):
        """[accumulation, frame buffer, albedo_prim, normal_depth] as raw bits."""
        L, ctx = self.L, self.ctx
        sizes = (w * h * 16, w * h * 4, w * h * 16, w * h * 16)
        bufs = self._alloc(sizes)
        try:
            q = self._params(w, h, spp, xform)
            q.accumulationBuffer, q.frameBuffer = bufs[0], bufs[1]
            assert L.pt_launch_frames(ctx, C.byref(q), frames) == 0, self.err()
            assert L.pt_render_features(ctx, C.byref(q), bufs[2], bufs[3]) == 0, self.err()
            return [self._get(p, n) for p, n in zip(bufs, sizes)]
        finally:
            for p in bufs:
                L.pt_device_free(ctx, p)

    def blend(self, w=64, h=48, spp=8):
        """pt_temporal_blend of a 2-frame view (the history) into a 1-frame view at the same camera: the output's bits."""
        L, ctx = self.L, self.ctx
        n = w * h * 16
        acc0, alb0, nd0, hist0, acc1, alb1, nd1, out = bufs = self._alloc((n,) * 8)
        try:
            p0 = self._params(w, h, spp, None)
            p0.accumulationBuffer = acc0
            assert L.pt_launch_frames(ctx, C.byref(p0), 2) == 0, self.err()
            assert L.pt_render_features(ctx, C.byref(p0), alb0, nd0) == 0
            hist = self._get(acc0, n).view(np.float32).reshape(-1, 4).copy()
            hist[:, 3] = 2 * spp
            assert L.pt_copy_to_device(ctx, hist0, hist.ctypes.data, n) == 0
            p1 = self._params(w, h, spp, None)
            p1.accumulationBuffer = acc1
            assert L.pt_launch_frames(ctx, C.byref(p1), 1) == 0, self.err()
            assert L.pt_render_features(ctx, C.byref(p1), alb1, nd1) == 0
            assert L.pt_temporal_blend(ctx, C.byref(p1), spp, alb1, nd1, C.byref(p0), hist0, alb0, nd0, 256.0, out) == 0, self.err()
            return self._get(out, n)
        finally:
            for p in bufs:
                L.pt_device_free(ctx, p)


@pytest.fixture
def ctxs():
    made = []

    def make(*a, **kw):
        c = _Ctx(*a, **kw)
        made.append(c)
        return c

    def arrays(*a, **kw):
        c = _Ctx.from_arrays(*a, **kw)
        made.append(c)
        return c

    make.arrays = arrays
    yield make
    for c in made:
        c.close()


# ---- scenes and rays ---------------------------------------------------------------------------------------------------------------

def _box():
    obj = pt.TinyObjWrapper(BOX)
    v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    return v, np.ascontiguousarray(obj.getIndexBuffer(), np.uint32).reshape(-1, 3), np.ascontiguousarray(obj.getMaterialIndices(), np.uint32), \
        _table(obj.getMaterials())


def _stress(path, **kw):
    sys.path.insert(0, pt.SCENES)
    import make_scenes
    make_scenes.stress_scene(path, mtl_name=os.path.basename(path)[:-4] + ".mtl", **kw)
    obj = pt.TinyObjWrapper(path)
    v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    return v, np.ascontiguousarray(obj.getIndexBuffer(), np.uint32).reshape(-1, 3), np.ascontiguousarray(obj.getMaterialIndices(), np.uint32), \
        _table(obj.getMaterials())


def _jitter_and_move(path, v, seed=3):
    """0.3-unit jitter of every sphere vertex, and sphere s000 moved as a whole."""
    rng = np.random.default_rng(seed)
    vn = v.copy()
    spheres, first = _object_vertices(path, "s0"), _object_vertices(path, "s000")
    vn[spheres, :3] += rng.normal(scale=0.3, size=(len(spheres), 3)).astype(np.float32)
    vn[first, :3] += np.float32([40.0, -25.0, 30.0])
    return vn


def _object_tris(path, idx, prefix):
    return np.all(np.isin(idx, _object_vertices(path, prefix)), axis=1)


def _light_material(mats):
    return next(i for i, m in enumerate(mats) if m.emission.x + m.emission.y + m.emission.z > 0)


def _rays(v, idx, seed, n=10000, per_kind=500):
    """Random rays over the scene box of v (grown by 10 %) and adversarial rays of v's own triangles."""
    lo, hi = refit_ref.scene_box(v, idx)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    ext = hi - lo
    r = random_rays(n, seed, lo=tuple(lo - 0.1 * ext), hi=tuple(hi + 0.1 * ext))
    return np.ascontiguousarray(np.concatenate([r, adversarial_rays(v, idx, seed + 1, n_per_kind=per_kind)]), np.float32)


def _map_rays(rays, s, off):
    """The rays of the scene mapped by x -> s x + off: origins mapped, directions scaled, so every t and tmin / tmax stays."""
    r = rays.copy()
    r[:, 0:3] = r[:, 0:3] * np.float32(s) + np.float32(off)
    r[:, 3:6] = r[:, 3:6] * np.float32(s)
    return np.ascontiguousarray(r, np.float32)


# ---- the checks -------------------------------------------------------------------------------------------------------------------

def _box_of(c):
    i = c.info()
    return np.array(i.scene_lo, np.float32), np.array(i.scene_hi, np.float32)


def _same_box(upd, fresh, v):
    (a, b), (x, y) = _box_of(upd), _box_of(fresh)
    lo, hi = refit_ref.scene_box(v, upd.idx.reshape(-1, 3))
    assert np.array_equal(a, x) and np.array_equal(b, y), (a, b, x, y)
    assert np.array_equal(a, lo) and np.array_equal(b, hi), (a, b, lo, hi)


def _oracle_answers(oracle, c, v, rays):
    """(t bits, prim, any-hit) of the oracle on c's scene with vertices v: brute force up to BRUTE_LIMIT triangles, else its BVH plus a
    brute-force check of that on the first 150 rays."""
    sc = oracle.scene(v, c.idx, c.mid, c.mats)
    try:
        brute = c.idx.size // 3 <= BRUTE_LIMIT
        t, p = sc.trace_closest(rays, use_bvh=not brute)
        hit = sc.trace_any(rays, use_bvh=not brute)
        if not brute:
            tb, pb = sc.trace_closest(rays[:150], use_bvh=False)
            assert np.array_equal(pb, p[:150]) and np.array_equal(tb.view(np.uint32), t[:150].view(np.uint32))
        return t.view(np.uint32), p, hit
    finally:
        sc.close()


def _same_queries(upd, fresh, rays, ref=None):
    """upd's queries equal fresh's and, if given, the oracle's (ref); returns upd's."""
    q = upd.trace(rays)
    for x, y in zip(q, fresh.trace(rays)):
        assert np.array_equal(x, y)
    if ref is not None:
        t, p, hit = ref
        assert np.array_equal(q[1], p) and np.array_equal(q[0], t)
        assert np.array_equal(q[2] != 0, hit != 0)
    assert np.array_equal(q[2] != 0, q[1] != MISS)
    return q


def _images(c, maths, lights, **kw):
    out = {}
    for m in maths:
        for l in lights:
            c.modes(m, l)
            out[(m, l)] = c.render(**kw)
    return out


def _same_images(a, b, maths=BOTH_MATHS, lights=BOTH_LIGHTS, **kw):
    ia = _images(a, maths, lights, **kw)
    for key, want in _images(b, maths, lights, **kw).items():
        for x, y in zip(ia[key], want):
            assert np.array_equal(x, y), key
    return ia


class _Snapshot:
    """What a context answers before its refits: queries, images, scene box, fp16 ratios."""

    def __init__(self, c, rays, maths=BOTH_MATHS, lights=BOTH_LIGHTS, **kw):
        self.rays, self.maths, self.lights, self.kw = rays, maths, lights, kw
        self.q = c.trace(rays)
        self.img = _images(c, maths, lights, **kw)
        i = c.info()
        self.box = (list(i.scene_lo), list(i.scene_hi))
        self.ratios = (i.half_area_ratio, i.half_box_inflation)

    def restored(self, c):
        for x, y in zip(c.trace(self.rays), self.q):
            assert np.array_equal(x, y)
        for key, imgs in _images(c, self.maths, self.lights, **self.kw).items():
            for x, y in zip(imgs, self.img[key]):
                assert np.array_equal(x, y), key
        i = c.info()
        assert (list(i.scene_lo), list(i.scene_hi)) == self.box
        assert i.half_area_ratio == pytest.approx(self.ratios[0], rel=1e-5)
        assert i.half_box_inflation == pytest.approx(self.ratios[1], rel=1e-5)


def _refit(c, v):
    rc, info = c.update(v)
    assert rc == 0, c.err()
    assert info.rebuilt == 0
    return info


def _refit_and_check(ctxs, oracle, upd, v, rays, maths=BOTH_MATHS, lights=BOTH_LIGHTS, xform=None):
    """Refit upd to v; everything against a fresh context of the same arrays and build mode, and the oracle."""
    _refit(upd, v)
    fresh = ctxs.arrays(v, upd.idx, upd.mid, upd.mats, build_mode=upd.build_mode)
    _same_box(upd, fresh, v)
    _same_queries(upd, fresh, rays, _oracle_answers(oracle, upd, v, rays))
    imgs = _same_images(upd, fresh, maths, lights, xform=xform)
    fresh.close()
    return imgs


# ---- A. every builder ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build_mode", [0, 1, 2])
def test_every_builder_on_the_box(ctxs, oracle, build_mode):
    v, idx, ids, mats = _box()
    c = ctxs.arrays(v, idx, ids, mats, build_mode=build_mode)
    base = _Snapshot(c, _rays(v, idx, 11))
    for kind, vn in _deformations(v).items():
        _refit_and_check(ctxs, oracle, c, vn, _rays(vn, idx, 13))
        _refit(c, v)
        base.restored(c)


@pytest.mark.parametrize("build_mode", [0, 1, 2])
def test_every_builder_on_82k_triangles(ctxs, oracle, tmp_path, build_mode):
    path = str(tmp_path / "s82k.obj")
    v, idx, ids, mats = _stress(path, n_spheres=4, subdiv=5)
    assert len(idx) == 4 * 20480 + 12
    c = ctxs.arrays(v, idx, ids, mats, build_mode=build_mode)
    base = _Snapshot(c, _rays(v, idx, 21, per_kind=300), maths=(IEEE,))
    vn = _jitter_and_move(path, v)
    _refit_and_check(ctxs, oracle, c, vn, _rays(vn, idx, 23, per_kind=300), maths=(IEEE,))
    _refit(c, v)
    base.restored(c)


# ---- B. past the grid-stride bound of k_rf_leaves --------------------------------------------------------------------------------

def test_config5_scene_past_the_grid_stride(ctxs, oracle, tmp_path):
    """1 310 732 triangles: k_rf_leaves launches at most 1024 x 256 threads, so each takes five or more leaf slots."""
    path = str(tmp_path / "stress.obj")
    v, idx, ids, mats = _stress(path)
    n = len(idx)
    assert n == 64 * 20480 + 12 and n > 5 * 1024 * 256
    kw = dict(w=96, h=54, spp=2, frames=1)
    c = ctxs.arrays(v, idx, ids, mats)
    rays0 = np.ascontiguousarray(np.concatenate([random_rays(120000, 41, lo=(20, 20, 20), hi=(530, 530, 540)),
                                                 adversarial_rays(v, idx, 42, n_per_kind=500)]), np.float32)
    base = _Snapshot(c, rays0, maths=(IEEE,), **kw)

    # (1) jitter plus a sphere moved: against a fresh build and the oracle's BVH (with its brute-force sample)
    v1 = _jitter_and_move(path, v, seed=5)
    rays = np.ascontiguousarray(np.concatenate([rays0[:120000], adversarial_rays(v1, idx, 43, n_per_kind=500)]), np.float32)
    _refit(c, v1)
    fresh = ctxs.arrays(v1, idx, ids, mats)
    _same_box(c, fresh, v1)
    ref = _oracle_answers(oracle, c, v1, rays)
    _same_queries(c, fresh, rays, ref)
    for fmt in (0, 1, 2, 3, 4):       # the ray-stream kernel over each node format, rebuilt from the refitted tree
        t, p = c.bench(rays, fmt)
        assert np.array_equal(p, ref[1]) and np.array_equal(t, ref[0]), fmt
    _same_images(c, fresh, maths=(IEEE,), **kw)
    fresh.close()

    # (2) the whole scene x3 and moved: a new fp16 space
    v2 = v.copy()
    v2[:, :3] = v2[:, :3] * np.float32(3.0) + np.float32([-700.0, 250.0, 1300.0])
    rays2 = _map_rays(rays0, 3.0, (-700.0, 250.0, 1300.0))
    _refit(c, v2)
    fresh = ctxs.arrays(v2, idx, ids, mats)
    _same_box(c, fresh, v2)
    q = _same_queries(c, fresh, rays2)
    assert (q[1] != MISS).mean() > 0.5
    for fmt in (0, 1, 2, 3, 4):
        t, p = c.bench(rays2, fmt)
        assert np.array_equal(p, q[1]) and np.array_equal(t, q[0]), fmt
    _same_images(c, fresh, maths=(IEEE,), xform=(3.0, (-700.0, 250.0, 1300.0)), **kw)
    fresh.close()

    # (3) back to the original vertices
    _refit(c, v)
    base.restored(c)


# ---- C. long chains ----------------------------------------------------------------------------------------------------------------

def test_twenty_thousand_copies_of_one_triangle(ctxs, oracle):
    """20 000 copies of one triangle, each with its own vertices, under hashed pairing (build mode 2): a tree of long chains, so long
    runs of hand-offs between threads in k_rf_refit.  Copy i moves i * 1e-3 along the normal, then back."""
    n = 20000
    tri = np.array([[100, 100, 300, 0], [400, 100, 300, 0], [100, 400, 300, 0]], np.float32)
    v = np.ascontiguousarray(np.tile(tri, (n, 1)), np.float32)
    idx = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    _, _, _, mats = _box()
    ids = np.zeros(n, np.uint32)
    c = ctxs.arrays(v, idx, ids, mats, build_mode=2)
    i0 = c.info()
    assert i0.max_depth < i0.stack_entries <= 128, (i0.max_depth, i0.stack_entries)
    along = random_rays(600, 61, lo=(50, 50, 0), hi=(450, 450, 250))
    along[:, 3:6] = along[:, 3:6] * np.float32([0.3, 0.3, 0.0]) + np.float32([0, 0, 1])
    along[:, 3:6] /= np.linalg.norm(along[:, 3:6], axis=1, keepdims=True)
    base_rays = np.ascontiguousarray(np.concatenate([along, _rays(v, idx, 63, n=4000, per_kind=200)]), np.float32)
    base = _Snapshot(c, base_rays)
    vn = v.copy()
    vn[:, 2] += (np.repeat(np.arange(n), 3) * 1e-3).astype(np.float32)
    rays = np.ascontiguousarray(np.concatenate([along, _rays(vn, idx, 65, n=4000, per_kind=200)]), np.float32)
    _refit_and_check(ctxs, oracle, c, vn, rays)
    i1 = c.info()
    assert i1.max_depth == i0.max_depth and i1.max_depth < i1.stack_entries <= 128
    hits = c.trace(rays)[1]
    assert (hits == 0).sum() > 50 and len(np.unique(hits[hits != MISS])) > 1
    _refit(c, v)
    base.restored(c)


# ---- D. degenerate targets ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_tris", [1, 2])
@pytest.mark.parametrize("variant", [None, 1])            # the default (fp16 nodes), fp32 nodes
def test_one_and_two_triangles(ctxs, oracle, n_tris, variant):
    """One triangle: k_rf_single; two: a tree of one node."""
    tris = np.array([[100, 100, 300, 0], [400, 120, 310, 0], [150, 400, 290, 0],
                     [200, 50, 400, 0], [450, 300, 420, 0], [300, 480, 380, 0]], np.float32)
    v = np.ascontiguousarray(tris[:3 * n_tris], np.float32)
    idx = np.arange(3 * n_tris, dtype=np.uint32).reshape(-1, 3)
    _, _, ids, mats = _box()
    ids = np.arange(n_tris, dtype=np.uint32) % len(mats)
    c = ctxs.arrays(v, idx, ids, mats, variant=variant)
    assert c.info().n_nodes == 1
    base = _Snapshot(c, _rays(v, idx, 71, n=3000, per_kind=200))
    moved = v.copy()
    moved[:, :3] += np.float32([130.0, -60.0, 90.0])                        # out of the old box
    scaled = v.copy()
    ctr = v[:, :3].mean(axis=0).astype(np.float32)
    scaled[:, :3] = (v[:, :3] - ctr) * np.float32(3.0) + ctr
    for vn in (moved, scaled):
        _refit_and_check(ctxs, oracle, c, vn, _rays(vn, idx, 73, n=3000, per_kind=200))
        assert (c.trace(_rays(vn, idx, 75, n=10, per_kind=200))[1] != MISS).any()
    _refit(c, v)
    base.restored(c)


def test_box_flattened_onto_a_plane(ctxs, oracle):
    v, idx, ids, mats = _box()
    c = ctxs.arrays(v, idx, ids, mats)
    base_rays = _rays(v, idx, 81)
    base = _Snapshot(c, base_rays)
    vn = v.copy()
    vn[:, 1] = np.float32(200.0)
    _refit_and_check(ctxs, oracle, c, vn, np.concatenate([base_rays, _rays(vn, idx, 83)]))
    lo, hi = _box_of(c)
    assert hi[1] - lo[1] < 1e-2 * (hi[0] - lo[0])                         # the per-axis fallback of the fp16 space
    _refit(c, v)
    base.restored(c)


def test_box_collapsed_to_a_point(ctxs, oracle):
    v, idx, ids, mats = _box()
    c = ctxs.arrays(v, idx, ids, mats)
    base_rays = _rays(v, idx, 91)
    base = _Snapshot(c, base_rays)
    vn = v.copy()
    vn[:, :3] = np.float32([278.0, 274.0, 280.0])
    imgs = _refit_and_check(ctxs, oracle, c, vn, base_rays)
    for bufs in imgs.values():
        assert np.all(np.isfinite(bufs[0].view(np.float32)))
    _refit(c, v)
    base.restored(c)


def test_half_the_triangles_zero_area(ctxs, oracle):
    """Every other triangle and the lamp's first triangle lose their area (one vertex moved onto another): light mode 1 drops the
    emissive ones exactly as a fresh build's list does, and the images stay finite."""
    v, idx, ids, mats = _box()
    c = ctxs.arrays(v, idx, ids, mats)
    base = _Snapshot(c, _rays(v, idx, 101))
    lamp = np.flatnonzero(_object_tris(BOX, idx, "lamp"))
    assert len(lamp) >= 2 and np.all(ids[lamp] == _light_material(mats))
    vn = v.copy()
    for t in sorted(set(range(0, len(idx), 2)) | {int(lamp[0])}):
        vn[idx[t, 1], :3] = vn[idx[t, 0], :3]
    e1 = vn[idx[:, 1], :3] - vn[idx[:, 0], :3]
    e2 = vn[idx[:, 2], :3] - vn[idx[:, 0], :3]
    zero = np.linalg.norm(np.cross(e1, e2), axis=1) == 0
    assert zero.mean() >= 0.5 and zero[lamp].any()
    imgs = _refit_and_check(ctxs, oracle, c, vn, _rays(vn, idx, 103))
    for bufs in imgs.values():
        assert np.all(np.isfinite(bufs[0].view(np.float32)))
    _refit(c, v)
    base.restored(c)


@pytest.mark.parametrize("s,off", [(1e6, (0.0, 0.0, 0.0)), (1e-6, (0.0, 0.0, 0.0)), (1.0, (1e7, 1e7, 1e7))], ids=["x1e6", "x1e-6", "plus1e7"])
def test_extreme_magnitudes(ctxs, oracle, s, off):
    v, idx, ids, mats = _box()
    c = ctxs.arrays(v, idx, ids, mats)
    rays = _rays(v, idx, 111)
    base = _Snapshot(c, rays)
    vn = v.copy()
    vn[:, :3] = vn[:, :3] * np.float32(s) + np.float32(off)
    mapped = _map_rays(rays, s, off)
    _refit_and_check(ctxs, oracle, c, vn, np.concatenate([mapped, _rays(vn, idx, 113, n=2000, per_kind=200)]), xform=(s, off))
    assert (c.trace(mapped)[1] != MISS).mean() > 0.1
    _refit(c, v)
    base.restored(c)


def test_unreferenced_vertex_moves_only_the_pad(ctxs, oracle):
    """A vertex no triangle uses, moved alone to (1e6, 0, 0): pad_abs is taken over every vertex, so every triangle box and the scene
    box grow by what refit_ref says, and nothing else changes."""
    v, idx, ids, mats = _box()
    v = np.ascontiguousarray(np.concatenate([v, np.float32([[278.0, 274.0, 280.0, 0.0]])]), np.float32)
    c = ctxs.arrays(v, idx, ids, mats)
    rays = _rays(v[:-1], idx, 121)
    base = _Snapshot(c, rays)
    lo0, hi0 = _box_of(c)
    vn = v.copy()
    vn[-1, :3] = np.float32([1e6, 0.0, 0.0])
    pa0, pa1 = refit_ref.pad_abs(v), refit_ref.pad_abs(vn)
    assert pa1 == np.float32(1e6) * np.float32(2.0 ** -19) and pa1 > 100 * pa0
    _refit_and_check(ctxs, oracle, c, vn, rays)
    lo1, hi1 = _box_of(c)
    want_lo, want_hi = refit_ref.scene_box(vn, idx)
    assert np.array_equal(lo1, want_lo) and np.array_equal(hi1, want_hi)
    assert np.all(lo1 < lo0) and np.all(hi1 > hi0)
    for x, y in zip(c.trace(rays), base.q):                                   # nor did any answer
        assert np.array_equal(x, y)
    _refit(c, v)
    base.restored(c)


# ---- E. derived arrays and variants ------------------------------------------------------------------------------------------------

def _variants(L):
    out = []
    for v in range(64):
        name = L.pt_variant_name(v)
        if name is None:
            break
        if not (name.startswith(b"DIAG") or name.startswith(b"LIGHTS")):
            out.append(v)
    return out


def test_variant_chosen_before_the_refit(ctxs):
    """(1) pt_set_tuning(v), refit, render: what a fresh context under v renders, and the same queries."""
    v, idx, ids, mats = _box()
    vn = _deformations(v)["scale"]
    rays = _rays(vn, idx, 131)
    L = _native.hip()
    tried = 0
    for var in _variants(L):
        c = ctxs.arrays(v, idx, ids, mats, variant=var)
        _refit(c, vn)
        fresh = ctxs.arrays(vn, idx, ids, mats, variant=var)
        _same_images(c, fresh, maths=(FAST,), lights=(0,))
        _same_queries(c, fresh, rays)
        c.close(); fresh.close()
        tried += 1
    assert tried >= 8


def test_variant_switched_after_the_refit(ctxs):
    """(2) default variant, refit, then pt_set_tuning(v), render: the fresh context's default image (every variant gives the same bits)."""
    v, idx, ids, mats = _box()
    vn = _deformations(v)["rigid"]
    L = _native.hip()
    fresh = ctxs.arrays(vn, idx, ids, mats)
    fresh.modes(FAST, 0)
    want = fresh.render()
    for var in _variants(L):
        c = ctxs.arrays(v, idx, ids, mats)
        c.render()
        _refit(c, vn)
        assert L.pt_set_tuning(c.ctx, 0, var) == 0, c.err()
        for x, y in zip(c.render(), want):
            assert np.array_equal(x, y), var
        c.close()


def test_derived_arrays_are_rebuilt_not_reused(ctxs, oracle):
    """(3) The four-wide records (stream format 1) and the fp16 {lo, hi} nodes (format 3) exist before the refit, and so does each render
    variant's own node array: after the refit all of them answer for the new vertices."""
    v, idx, ids, mats = _box()
    vn = _deformations(v)["drag"]
    vn[_object_vertices(BOX, "short_block"), :3] += np.float32([-90.0, 60.0, 120.0])
    rays = _rays(vn, idx, 141)
    old_rays = _rays(v, idx, 143)
    ref = _oracle_answers(oracle, _Arrays(idx, ids, mats).as_scene(), vn, rays)
    L = _native.hip()
    for var in [None] + _variants(L):
        c = ctxs.arrays(v, idx, ids, mats, variant=var)
        c.modes(FAST, 0)
        c.render()
        for fmt in (1, 3):
            c.bench(old_rays, fmt)
        assert c.info().wide_nodes > 0
        _refit(c, vn)
        for fmt in (1, 3):
            t, p = c.bench(rays, fmt)
            assert np.array_equal(p, ref[1]) and np.array_equal(t, ref[0]), (var, fmt)
        fresh = ctxs.arrays(vn, idx, ids, mats, variant=var)
        _same_images(c, fresh, maths=(FAST,), lights=(0,))
        c.close(); fresh.close()


# ---- F. material edits interleaved with refits ----------------------------------------------------------------------------------

def _material_edits(mats, ids, emissive_tris):
    """Two edits: (1) material 0 recoloured, a new emissive material on the triangles `emissive_tris`; (2) the lamp twice as bright,
    the new material's emission and colour changed."""
    light = _light_material(mats)
    m1 = [_native.Material.from_buffer_copy(m) for m in mats]
    m1[0].diffuse = _native.Float3(0.2, 0.3, 0.9)
    extra = _native.Material.from_buffer_copy(m1[0])
    extra.bsdfType, extra.diffuse, extra.emission = 0, _native.Float3(0.8, 0.8, 0.8), _native.Float3(3.0, 2.0, 1.0)
    m1.append(extra)
    ids1 = ids.copy()
    ids1[emissive_tris] = len(m1) - 1
    m2 = [_native.Material.from_buffer_copy(m) for m in m1]
    e = m2[light].emission
    m2[light].emission = _native.Float3(2 * e.x, 2 * e.y, 2 * e.z)
    m2[-1].emission, m2[-1].diffuse = _native.Float3(0.5, 4.0, 0.5), _native.Float3(0.9, 0.5, 0.1)
    return (m1, ids1), (m2, None)


def _same_as_fresh(c, v, light_modes=(1,)):
    fresh = _Ctx.from_arrays(v, c.idx, c.mid, c.mats)
    try:
        _same_images(c, fresh, maths=(IEEE,), lights=light_modes)
        c.modes(IEEE, 1); fresh.modes(IEEE, 1)
        assert np.array_equal(c.blend(), fresh.blend())
    finally:
        fresh.close()


@pytest.mark.parametrize("scene", ["box", "s82k"])
def test_material_edits_interleaved_with_refits(ctxs, tmp_path, scene):
    if scene == "box":
        path = BOX
        v, idx, ids, mats = _box()
        v1, v2 = _deformations(v)["rigid"], _deformations(v)["jitter"]
        emissive = _object_tris(BOX, idx, "short_block")
    else:
        path = str(tmp_path / "s82k.obj")
        v, idx, ids, mats = _stress(path, n_spheres=4, subdiv=5)
        v1 = _jitter_and_move(path, v)
        v2 = _jitter_and_move(path, v1, seed=9)
        emissive = _object_tris(path, idx, "s001")
    assert emissive.any()
    (m1, ids1), (m2, _) = _material_edits(mats, ids, emissive)
    c = ctxs.arrays(v, idx, ids, mats, light=1)
    c.update_materials(m1, ids1)
    _same_as_fresh(c, v)
    _refit(c, v1)
    _same_as_fresh(c, v1, light_modes=(0, 1))
    c.update_materials(m2)
    _same_as_fresh(c, v1)
    _refit(c, v2)
    _same_as_fresh(c, v2, light_modes=(0, 1))
