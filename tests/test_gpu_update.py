"""In-place vertex updates on the GPU (pt_update_vertices): after a refit every query answer and every image bit equals what a context
that received the same vertices through pt_set_scene computes — under deformations that move the scene box, in both math modes and
both light modes, on fp16 and fp32 nodes, on a scene large enough for the depth-first order and the device reinsertion —, a round
trip gives the old bits back, REBUILD equals a fresh build, AUTO picks by its threshold, the bookkeeping (handle, device bytes) and
the refusals hold, a group context updates every rank, TemporalHistory drops its history, and acgpt_main --move renders what a moved
OBJ renders."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
from scene_utils import adversarial_rays, make_params, random_rays

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")


def _object_vertices(path, prefix):
    """0-based indices of the vertices that the faces of the OBJ objects whose name starts with `prefix` reference."""
    out, obj, nv = set(), "", 0
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "o":
            obj = t[1]
        elif t[0] == "v":
            nv += 1
        elif t[0] == "f" and obj.startswith(prefix):
            for w in t[1:]:
                k = int(w.split("/")[0])
                out.add(k - 1 if k > 0 else nv + k)
    return np.array(sorted(out))


class _Ctx:
    """A context with one scene, through the C ABI only."""

    def __init__(self, obj, verts, math=None, light=None, variant=None, device_ids=None):
        self.L = L = _native.hip()
        self.ctx = C.c_void_p()
        if device_ids:
            ids = (C.c_int * len(device_ids))(*device_ids)
            assert L.pt_create_multi(C.byref(self.ctx), ids, len(device_ids)) == 0
        else:
            assert L.pt_create(C.byref(self.ctx), 0) == 0
        if math is not None:
            assert L.pt_set_math_mode(self.ctx, math) == 0
        if light is not None:
            assert L.pt_set_light_mode(self.ctx, light) == 0
        if variant is not None:
            assert L.pt_set_tuning(self.ctx, 0, variant) == 0
        self.idx = np.ascontiguousarray(obj.getIndexBuffer(), np.uint32)
        self.mid = np.ascontiguousarray(obj.getMaterialIndices(), np.uint32)
        self.mats = obj.getMaterials()
        self.set_scene(verts)

    def err(self):
        return self.L.pt_last_error(self.ctx)

    def set_scene(self, verts):
        v = np.ascontiguousarray(verts, np.float32)
        assert self.L.pt_set_scene(self.ctx, v.ctypes.data, v.size // 4, self.idx.ctypes.data, self.idx.size // 3, self.mid.ctypes.data,
                                   C.addressof(self.mats), len(self.mats)) == 0, self.err()

    def update(self, verts, mode=_native.UPDATE_REFIT, n=None):
        v = np.ascontiguousarray(verts, np.float32)
        info = _native.UpdateInfo()
        rc = self.L.pt_update_vertices(self.ctx, v.ctypes.data, v.size // 4 if n is None else n, mode, C.byref(info))
        return rc, info

    def handle(self):
        return self.L.pt_scene_handle(self.ctx)

    def info(self):
        b = _native.BvhInfo()
        assert self.L.pt_get_bvh_info(self.ctx, C.byref(b)) == 0
        return b

    def trace(self, rays):
        n = rays.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32); hit = np.zeros(n, np.uint8)
        assert self.L.pt_trace_closest(self.ctx, rays.ctypes.data, n, t.ctypes.data, prim.ctypes.data) == 0, self.err()
        assert self.L.pt_trace_any(self.ctx, rays.ctypes.data, n, hit.ctypes.data) == 0, self.err()
        return t.view(np.uint32), prim, hit

    def render(self, w=64, h=48, spp=8, frames=2, handle=None):
        """(accumulation, frame buffer, albedo_prim, normal_depth) as raw bits; or the return code if the launch is refused."""
        L, ctx = self.L, self.ctx
        bufs = []
        for nbytes in (w * h * 16, w * h * 4, w * h * 16, w * h * 16):
            p = C.c_void_p()
            assert L.pt_device_malloc(ctx, C.byref(p), nbytes) == 0
            assert L.pt_device_memset(ctx, p, 0, nbytes) == 0
            bufs.append(p.value)
        try:
            q = make_params(w, h, spp, 6, True, True)
            q.accumulationBuffer, q.frameBuffer = bufs[0], bufs[1]
            q.handle = self.handle() if handle is None else handle
            rc = L.pt_launch_frames(ctx, C.byref(q), frames)
            if rc != 0:
                return rc
            assert L.pt_render_features(ctx, C.byref(q), bufs[2], bufs[3]) == 0, self.err()
            out = []
            for p, nbytes in zip(bufs, (w * h * 16, w * h * 4, w * h * 16, w * h * 16)):
                a = np.zeros(nbytes // 4, np.uint32)
                assert L.pt_copy_to_host(ctx, a.ctypes.data, p, nbytes) == 0
                out.append(a)
            return out
        finally:
            for p in bufs:
                L.pt_device_free(ctx, p)

    def close(self):
        if self.ctx:
            self.L.pt_destroy(self.ctx)
            self.ctx = None


@pytest.fixture
def ctxs():
    made = []

    def make(*a, **kw):
        c = _Ctx(*a, **kw)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def _box_scene():
    obj = pt.TinyObjWrapper(BOX)
    return obj, np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)


def _deformations(v):
    """The four deformations of the Cornell box: rigid motion of the tall block, 1 % jitter, x8 scale plus offset, a dragged vertex."""
    out = {}
    tall = _object_vertices(BOX, "tall_block")
    a = v.copy()
    c = a[tall, :3].mean(axis=0)
    ang = np.float32(0.4)
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
    a[tall, :3] = ((a[tall, :3] - c) @ R.T + c + np.float32([-60.0, 25.0, 40.0])).astype(np.float32)
    out["rigid"] = a
    rng = np.random.default_rng(7)
    b = v.copy()
    b[:, :3] += rng.uniform(-5.56, 5.56, size=(len(b), 3)).astype(np.float32)       # 1 % of the box's 556 units
    out["jitter"] = b
    d = v.copy()
    d[:, :3] = d[:, :3] * np.float32(8.0) + np.float32([-1234.5, 333.25, 777.0])
    out["scale"] = d
    e = v.copy()
    e[tall[0], :3] = np.float32([4100.0, -2700.0, 3300.0])
    out["drag"] = e
    return out


def _rays_for(ctx, verts, idx, seed):
    info = ctx.info()
    lo, hi = np.array(info.scene_lo, np.float64), np.array(info.scene_hi, np.float64)
    ext = hi - lo
    r = random_rays(20000, seed, lo=tuple(lo - 0.1 * ext), hi=tuple(hi + 0.1 * ext))
    return np.ascontiguousarray(np.concatenate([r, adversarial_rays(verts, idx.reshape(-1, 3), seed + 1, n_per_kind=1000)]), np.float32)


def _same_queries(a, b, rays):
    for x, y in zip(a.trace(rays), b.trace(rays)):
        assert np.array_equal(x, y)


def _same_images(a, b):
    ra, rb = a.render(), b.render()
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind", ["rigid", "jitter", "scale", "drag"])
def test_refit_queries_equal_a_fresh_build(ctxs, kind):
    obj, v = _box_scene()
    vn = _deformations(v)[kind]
    upd = ctxs(obj, v)
    rc, info = upd.update(vn)
    assert rc == 0, upd.err()
    assert info.rebuilt == 0 and info.area_ratio > 0 and info.ms > 0
    fresh = ctxs(obj, vn)
    a, b = upd.info(), fresh.info()
    assert list(a.scene_lo) == list(b.scene_lo) and list(a.scene_hi) == list(b.scene_hi)
    assert a.n_nodes == b.n_nodes                   # (the trees differ: the refit keeps the old topology)
    _same_queries(upd, fresh, _rays_for(fresh, vn, upd.idx, 11))
    _same_images(upd, fresh)


@pytest.mark.parametrize("math", [_native.MATH_IEEE, _native.MATH_FAST])
@pytest.mark.parametrize("light", [0, 1])
def test_refit_images_equal_a_fresh_build(ctxs, math, light):
    obj, v = _box_scene()
    vn = _deformations(v)["rigid"]
    lamp = _object_vertices(BOX, "lamp")
    vn[lamp, 0] += np.float32(35.0)                # the emissive triangles move too: light mode 1's list is rebuilt
    vn[lamp, 2] -= np.float32(20.0)
    upd = ctxs(obj, v, math=math, light=light)
    assert upd.update(vn)[0] == 0, upd.err()
    _same_images(upd, ctxs(obj, vn, math=math, light=light))


@pytest.mark.parametrize("variant", [1, 7])          # fp32 nodes, fp16 nodes (pt_set_tuning)
def test_refit_on_forced_node_formats(ctxs, variant):
    obj, v = _box_scene()
    vn = _deformations(v)["scale"]
    upd = ctxs(obj, v, variant=variant)
    assert upd.update(vn)[0] == 0, upd.err()
    fresh = ctxs(obj, vn, variant=variant)
    _same_images(upd, fresh)
    _same_queries(upd, fresh, _rays_for(fresh, vn, upd.idx, 5))


def test_large_scene(ctxs, tmp_path):
    sys.path.insert(0, pt.SCENES)
    import make_scenes
    path = str(tmp_path / "big.obj")
    make_scenes.stress_scene(path, n_spheres=4, subdiv=5, mtl_name="big.mtl")      # 81 932 triangles: depth-first order, device reinsertion
    obj = pt.TinyObjWrapper(path)
    v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    assert len(obj.getIndexBuffer()) // 3 > 50000
    rng = np.random.default_rng(3)
    vn = v.copy()
    spheres, first = _object_vertices(path, "s0"), _object_vertices(path, "s000")
    vn[spheres, :3] += rng.normal(scale=0.3, size=(len(spheres), 3)).astype(np.float32)
    vn[first, :3] += np.float32([40.0, -25.0, 30.0])        # one sphere moves
    upd = ctxs(obj, v)
    rc, info = upd.update(vn)
    assert rc == 0 and info.rebuilt == 0, upd.err()
    fresh = ctxs(obj, vn)
    rays = random_rays(100000, 17, lo=(20, 20, 20), hi=(530, 530, 540))
    _same_queries(upd, fresh, rays)
    _same_images(upd, fresh)


def test_round_trip_and_unchanged_vertices(ctxs):
    obj, v = _box_scene()
    c = ctxs(obj, v)
    rays = _rays_for(c, v, c.idx, 23)
    q0, img0, i0 = c.trace(rays), c.render(), c.info()
    rc, info = c.update(v)
    assert rc == 0 and info.area_ratio == 1.0
    for kind, vn in _deformations(v).items():
        assert c.update(vn)[0] == 0
        assert c.update(v)[0] == 0
        for x, y in zip(c.trace(rays), q0):
            assert np.array_equal(x, y), kind
        for x, y in zip(c.render(), img0):
            assert np.array_equal(x, y), kind
        i1 = c.info()
        assert list(i1.scene_lo) == list(i0.scene_lo) and list(i1.scene_hi) == list(i0.scene_hi)
        assert i1.half_area_ratio == pytest.approx(i0.half_area_ratio, rel=1e-5)
        assert i1.half_box_inflation == pytest.approx(i0.half_box_inflation, rel=1e-5)
        rc, info = c.update(v)
        assert rc == 0 and info.area_ratio == 1.0


def test_rebuild_and_auto(ctxs):
    obj, v = _box_scene()
    vn = _deformations(v)["jitter"]
    c = ctxs(obj, v)
    rc, info = c.update(vn, _native.UPDATE_REBUILD)
    assert rc == 0 and info.rebuilt == 1 and info.area_ratio == 1.0
    fresh = ctxs(obj, vn)
    _same_images(c, fresh)
    a, b = c.info(), fresh.info()
    for name, _ in _native.BvhInfo._fields_:
        if name in ("build_ms", "wide_ms"):
            continue
        x, y = getattr(a, name), getattr(b, name)
        if name in ("half_area_ratio", "half_box_inflation"):
            assert x == pytest.approx(y, rel=1e-5), name
        else:
            assert list(x) == list(y) if hasattr(x, "__len__") else x == y, name
    # AUTO: a small move refits, a scramble of the vertices rebuilds
    c.update(v, _native.UPDATE_REBUILD)
    small = v.copy()
    small[:, :3] += np.random.default_rng(1).uniform(-0.5, 0.5, size=(len(v), 3)).astype(np.float32)
    rc, info = c.update(small, _native.UPDATE_AUTO)
    assert rc == 0 and info.rebuilt == 0 and info.area_ratio <= _native.UPDATE_AUTO_AREA_RATIO
    scrambled = v[np.random.default_rng(2).permutation(len(v))]
    rc, probe = c.update(scrambled, _native.UPDATE_REFIT)
    assert rc == 0 and probe.area_ratio > _native.UPDATE_AUTO_AREA_RATIO
    c.update(small, _native.UPDATE_REBUILD)
    rc, info = c.update(scrambled, _native.UPDATE_AUTO)
    assert rc == 0 and info.rebuilt == 1
    _same_images(c, ctxs(obj, scrambled))


def test_handle_and_device_bytes(ctxs):
    obj, v = _box_scene()
    vn = _deformations(v)["rigid"]
    c = ctxs(obj, v)
    n_tris = c.idx.size // 3
    built = c.info().device_bytes
    h0 = c.handle()
    assert c.update(vn)[0] == 0
    h1 = c.handle()
    assert h1 != h0
    assert c.render(handle=h0) != 0                  # a stale handle is refused
    assert c.info().device_bytes == built + 12 * n_tris
    for i in range(20):
        assert c.update(v if i % 2 else vn)[0] == 0
        assert c.info().device_bytes == built + 12 * n_tris
    assert len({h0, h1, c.handle()}) == 3
    c.set_scene(vn)
    assert c.info().device_bytes == built


def test_refusals_leave_the_scene_alone(ctxs):
    obj, v = _box_scene()
    c = ctxs(obj, v)
    before, h = c.render(), c.handle()
    L = c.L
    info = _native.UpdateInfo()
    assert c.update(v, n=len(v) - 1)[0] != 0
    assert c.update(v, n=len(v) + 1)[0] != 0
    assert L.pt_update_vertices(c.ctx, None, len(v), 0, C.byref(info)) != 0
    assert c.update(v, mode=3)[0] != 0 and c.update(v, mode=-1)[0] != 0
    assert L.pt_update_vertices(None, v.ctypes.data, len(v), 0, None) != 0
    assert c.handle() == h
    for x, y in zip(c.render(), before):
        assert np.array_equal(x, y)
    # no scene, and a scene without triangles
    bare = _Ctx.__new__(_Ctx)
    bare.L, bare.ctx = L, C.c_void_p()
    assert L.pt_create(C.byref(bare.ctx), 0) == 0
    try:
        assert L.pt_update_vertices(bare.ctx, v.ctypes.data, len(v), 0, None) != 0
        assert b"no scene" in L.pt_last_error(bare.ctx)
        assert L.pt_set_scene(bare.ctx, v.ctypes.data, len(v), None, 0, None, None, 0) == 0
        assert L.pt_update_vertices(bare.ctx, v.ctypes.data, len(v), 0, None) != 0
    finally:
        bare.close()


def test_group_context_updates_every_rank(ctxs, monkeypatch):
    obj, v = _box_scene()
    vn = _deformations(v)["scale"]
    single = ctxs(obj, v)
    monkeypatch.setenv("ACGPT_REHEARSE_SAME_GPU", "1")
    group = ctxs(obj, v, device_ids=[0, 0])
    assert single.update(vn)[0] == 0
    assert group.update(vn)[0] == 0, group.err()
    _same_images(single, group)


def test_python_update_and_temporal_history(gpu_state_factory):
    kw = dict(width=64, height=48, spp=8, max_depth=6, direct_lighting=True, importance_sampling=True)
    import temporal_ref as tr
    results = []
    for move in (False, True):
        state, obj = gpu_state_factory(BOX, **kw)
        v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
        hist = pt.TemporalHistory()
        try:
            state.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(None, state)
            state.params.currentFrameIdx = 1
            hist.update(state)
            if move:
                h = int(state.params.handle)
                out = pt.updateVertices(state, v.reshape(-1), mode="refit")
                assert out["rebuilt"] is False and out["area_ratio"] == 1.0
                assert int(state.params.handle) != h
            tr.set_camera(state.params, *tr.orbit_camera(64, 48, 20, 0))
            state.refreshAccumulationBuffer = True
            pt.updateState(None, state)
            pt.LaunchCurrentFrame(None, state)
            state.params.currentFrameIdx = 1
            results.append(hist.update(state))
        finally:
            hist.close()
    kept, dropped = results
    assert (kept[..., 3] > 8).mean() > 0.3              # the history carried over ...
    assert np.all(dropped[..., 3] == 8)                 # ... unless the scene changed


def test_cli_move(built, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    base = [exe, "--width", "96", "--height", "64", "--spp-per-launch", "8", "--frames", "2", "--max-depth", "6", "--direct-lighting"]
    d = (20.0, 0.0, -10.0)
    r = subprocess.run(base + ["--obj", BOX, "--out", str(tmp_path / "a.png"), "--move", "light:%g,%g,%g" % d],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Refit:" in r.stdout
    # the same move in an OBJ of its own: only the lamp's coordinates that change are rewritten
    lamp = set(_object_vertices(BOX, "lamp").tolist())
    lines, nv = [], 0
    for line in open(BOX):
        t = line.split()
        if t and t[0] == "v":
            if nv in lamp:
                xyz = [np.float32(float(x)) for x in t[1:4]]
                parts = ["%.9g" % (xyz[k] + np.float32(d[k])) if d[k] else t[1 + k] for k in range(3)]
                line = "v " + " ".join(parts) + "\n"
            nv += 1
        lines.append(line)
    moved = tmp_path / "moved.obj"
    moved.write_text("".join(lines))
    shutil.copy(os.path.join(pt.SCENES, "cornell_box.mtl"), tmp_path / "cornell_box.mtl")
    want = np.ascontiguousarray(pt.TinyObjWrapper(BOX).getVerticesFloat(), np.float32).reshape(-1, 4)
    want[sorted(lamp), :3] += np.float32(d)
    got = np.ascontiguousarray(pt.TinyObjWrapper(str(moved)).getVerticesFloat(), np.float32).reshape(-1, 4)
    assert np.array_equal(got, want)
    r = subprocess.run(base + ["--obj", str(moved), "--out", str(tmp_path / "b.png")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "a_moved.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    assert (tmp_path / "a.png").read_bytes() != (tmp_path / "b.png").read_bytes()
    r = subprocess.run(base + ["--obj", BOX, "--out", str(tmp_path / "c.png"), "--move", "no_such_material:1,0,0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and not (tmp_path / "c_moved.png").exists()
