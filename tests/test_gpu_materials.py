"""Material edits on the GPU (pt_update_materials): after an edit every image, feature, blend and query bit equals what a context that
received the same materials through pt_set_scene computes — for recolours, bsdf changes, new and raised emission and reassigned
faces, on both Cornell scenes, in both math modes and both light modes, on fp16 and fp32 nodes and on a group context —, the
bookkeeping (handle, pt_get_bvh_info, a later rebuild) and the refusals hold, TemporalHistory starts anew, and acgpt_main
--set-material renders what an edited .mtl renders."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
from scene_utils import make_params, random_rays

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
WHITE, RED, GREEN, LIGHT, GLASS, METAL = range(6)        # the scenes' material order (cornell_box.mtl)


def _copy(mats):
    return [_native.Material.from_buffer_copy(m) for m in mats]


def _table(mats):
    return (_native.Material * len(mats))(*mats)


def _edit(kind, mats, ids):
    """(new table, new ids or None) of one of the four edits."""
    m = _copy(mats)
    if kind == "recolour":
        m[RED].diffuse = _native.Float3(0.2, 0.3, 0.9)
        return m, None
    if kind == "bsdf":
        m[METAL].bsdfType, m[METAL].ior = 2, 1.4                  # metal -> glass
        m[GLASS].bsdfType = 0                                     # glass -> diffuse
        return m, None
    if kind == "emission":
        m[LIGHT].emission = _native.Float3(34.0, 24.0, 8.0)       # raised
        m[GREEN].emission = _native.Float3(1.0, 3.0, 0.5)         # added: light mode 1's list grows by the green wall
        return m, None
    if kind == "reassign":
        m.append(_native.Material.from_buffer_copy(m[WHITE]))     # a seventh material
        m[-1].diffuse = _native.Float3(0.9, 0.8, 0.1)
        n = ids.copy()
        n[ids == GREEN] = RED                                     # the right wall takes the left wall's material
        n[ids == RED] = len(m) - 1                                # the left wall the new one
        return m, n
    raise ValueError(kind)


class _Ctx:
    """A context with one scene, through the C ABI only."""

    def __init__(self, path, mats=None, ids=None, math=None, light=None, variant=None, device_ids=None):
        self.L = L = _native.hip()
        self.ctx = C.c_void_p()
        if device_ids:
            dev = (C.c_int * len(device_ids))(*device_ids)
            assert L.pt_create_multi(C.byref(self.ctx), dev, len(device_ids)) == 0
        else:
            assert L.pt_create(C.byref(self.ctx), 0) == 0
        if math is not None:
            assert L.pt_set_math_mode(self.ctx, math) == 0
        if light is not None:
            assert L.pt_set_light_mode(self.ctx, light) == 0
        if variant is not None:
            assert L.pt_set_tuning(self.ctx, 0, variant) == 0
        obj = pt.TinyObjWrapper(path)
        self.verts = np.ascontiguousarray(obj.getVerticesFloat(), np.float32)
        self.idx = np.ascontiguousarray(obj.getIndexBuffer(), np.uint32)
        self.mid = np.ascontiguousarray(obj.getMaterialIndices() if ids is None else ids, np.uint32)
        self.mats = _table(_copy(obj.getMaterials()) if mats is None else mats)
        assert L.pt_set_scene(self.ctx, self.verts.ctypes.data, self.verts.size // 4, self.idx.ctypes.data, self.idx.size // 3,
                              self.mid.ctypes.data, C.addressof(self.mats), len(self.mats)) == 0, self.err()

    def err(self):
        return self.L.pt_last_error(self.ctx)

    def update(self, mats, ids=None, n_tris=None, n_mats=None):
        t = None if mats is None else _table(mats)
        i = None if ids is None else np.ascontiguousarray(ids, np.uint32)
        nm = (0 if t is None else len(t)) if n_mats is None else n_mats
        nt = (0 if i is None else i.size) if n_tris is None else n_tris
        info = _native.UpdateInfo()
        rc = self.L.pt_update_materials(self.ctx, None if t is None else C.addressof(t), nm, None if i is None else i.ctypes.data, nt,
                                        C.byref(info))
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

    def render(self, w=64, h=48, spp=8, frames=2, handle=None):
        """[accumulation, frame buffer, albedo_prim, normal_depth] as raw bits; or the return code if the launch is refused."""
        L, ctx = self.L, self.ctx
        sizes = (w * h * 16, w * h * 4, w * h * 16, w * h * 16)
        bufs = self._alloc(sizes)
        try:
            q = make_params(w, h, spp, 6, True, True)
            q.accumulationBuffer, q.frameBuffer = bufs[0], bufs[1]
            q.handle = self.handle() if handle is None else handle
            rc = L.pt_launch_frames(ctx, C.byref(q), frames)
            if rc != 0:
                return rc
            assert L.pt_render_features(ctx, C.byref(q), bufs[2], bufs[3]) == 0, self.err()
            return [self._get(p, n) for p, n in zip(bufs, sizes)]
        finally:
            for p in bufs:
                L.pt_device_free(ctx, p)

    def blend(self, w=64, h=48, spp=8):
        """pt_temporal_blend of a 2-frame view (the history, {rgb, 16}) into a 1-frame view at the same camera: the output's bits."""
        L, ctx = self.L, self.ctx
        n = w * h * 16
        acc0, alb0, nd0, hist0, acc1, alb1, nd1, out = bufs = self._alloc((n,) * 8)
        try:
            p0 = make_params(w, h, spp, 6, True, True)
            p0.accumulationBuffer, p0.handle = acc0, self.handle()
            assert L.pt_launch_frames(ctx, C.byref(p0), 2) == 0, self.err()
            assert L.pt_render_features(ctx, C.byref(p0), alb0, nd0) == 0
            hist = self._get(acc0, n).view(np.float32).reshape(-1, 4).copy()
            hist[:, 3] = 2 * spp
            assert L.pt_copy_to_device(ctx, hist0, hist.ctypes.data, n) == 0
            p1 = make_params(w, h, spp, 6, True, True)
            p1.accumulationBuffer, p1.handle = acc1, self.handle()
            assert L.pt_launch_frames(ctx, C.byref(p1), 1) == 0, self.err()
            assert L.pt_render_features(ctx, C.byref(p1), alb1, nd1) == 0
            assert L.pt_temporal_blend(ctx, C.byref(p1), spp, alb1, nd1, C.byref(p0), hist0, alb0, nd0, 256.0, out) == 0, self.err()
            return self._get(out, n)
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


def _scene(path):
    obj = pt.TinyObjWrapper(path)
    return _copy(obj.getMaterials()), np.ascontiguousarray(obj.getMaterialIndices(), np.uint32)


def _same_outcome(a, b):
    """The same bits, or the same refusal."""
    ra, rb = a.render(), b.render()
    if isinstance(ra, int) or isinstance(rb, int):
        assert ra == rb
        return
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)


def _rays(c):
    info = c.info()
    lo, hi = np.array(info.scene_lo, np.float64), np.array(info.scene_hi, np.float64)
    ext = hi - lo
    return np.ascontiguousarray(random_rays(20000, 31, lo=tuple(lo - 0.1 * ext), hi=tuple(hi + 0.1 * ext)), np.float32)


EDITS = ["recolour", "bsdf", "emission", "reassign"]


@pytest.mark.parametrize("path", [BOX, BOX_DIFFUSE], ids=["box", "box_diffuse"])
@pytest.mark.parametrize("kind", EDITS)
@pytest.mark.parametrize("math", [_native.MATH_IEEE, _native.MATH_FAST])
@pytest.mark.parametrize("light", [0, 1])
def test_images_equal_a_fresh_scene(ctxs, path, kind, math, light):
    mats, ids = _scene(path)
    new_mats, new_ids = _edit(kind, mats, ids)
    upd = ctxs(path, math=math, light=light)
    before = upd.render()
    rc, info = upd.update(new_mats, new_ids)
    assert rc == 0, upd.err()
    assert info.rebuilt == 0 and info.area_ratio == 1.0 and info.ms > 0
    fresh = ctxs(path, new_mats, new_ids, math=math, light=light)
    after, want = upd.render(), fresh.render()
    for x, y in zip(after, want):
        assert np.array_equal(x, y)
    assert not np.array_equal(after[0], before[0])      # the edit shows


@pytest.mark.parametrize("math", [_native.MATH_IEEE, _native.MATH_FAST])
def test_no_emission_left(ctxs, math):
    mats, ids = _scene(BOX)
    dark = _copy(mats)
    for m in dark:
        m.emission = _native.Float3(0.0, 0.0, 0.0)
    for light in (0, 1):
        upd = ctxs(BOX, math=math, light=light)
        assert upd.update(dark)[0] == 0, upd.err()
        _same_outcome(upd, ctxs(BOX, dark, math=math, light=light))
        # and back: the light list is rebuilt from nothing
        assert upd.update(mats)[0] == 0, upd.err()
        _same_outcome(upd, ctxs(BOX, mats, math=math, light=light))


@pytest.mark.parametrize("variant", [1, 7])          # fp32 nodes, fp16 nodes (pt_set_tuning)
def test_forced_node_formats(ctxs, variant):
    mats, ids = _scene(BOX)
    for kind in EDITS:
        new_mats, new_ids = _edit(kind, mats, ids)
        upd = ctxs(BOX, variant=variant, light=1)
        assert upd.update(new_mats, new_ids)[0] == 0, upd.err()
        fresh = ctxs(BOX, new_mats, new_ids, variant=variant, light=1)
        _same_outcome(upd, fresh)
        rays = _rays(fresh)
        for x, y in zip(upd.trace(rays), fresh.trace(rays)):
            assert np.array_equal(x, y)


def test_group_context_updates_every_rank(ctxs, monkeypatch):
    mats, ids = _scene(BOX)
    new_mats, new_ids = _edit("reassign", mats, ids)
    new_mats[METAL].bsdfType = 2
    new_mats[GREEN].emission = _native.Float3(1.0, 2.0, 3.0)
    monkeypatch.setenv("ACGPT_REHEARSE_SAME_GPU", "1")
    group = ctxs(BOX, device_ids=[0, 0], light=1)
    assert group.update(new_mats, new_ids)[0] == 0, group.err()
    _same_outcome(group, ctxs(BOX, new_mats, new_ids, light=1))


def test_features_and_queries(ctxs):
    mats, ids = _scene(BOX)
    new_mats, new_ids = _edit("reassign", mats, ids)
    upd = ctxs(BOX)
    rays = _rays(upd)
    q0, img0 = upd.trace(rays), upd.render()
    assert upd.update(new_mats, new_ids)[0] == 0, upd.err()
    img1 = upd.render()
    fresh = ctxs(BOX, new_mats, new_ids)
    for x, y in zip(img1, fresh.render()):
        assert np.array_equal(x, y)
    alb0, alb1 = img0[2].view(np.float32).reshape(-1, 4), img1[2].view(np.float32).reshape(-1, 4)
    assert not np.array_equal(alb0[:, :3], alb1[:, :3])             # the albedo changes ...
    assert np.array_equal(img0[2].reshape(-1, 4)[:, 3], img1[2].reshape(-1, 4)[:, 3])      # ... the hit triangles do not
    assert np.array_equal(img0[3], img1[3])
    for x, y, z in zip(upd.trace(rays), q0, fresh.trace(rays)):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_temporal_blend_sees_the_new_bsdf(ctxs):
    mats, ids = _scene(BOX_DIFFUSE)
    metal = _copy(mats)
    metal[GLASS].bsdfType = 1                  # the diffuse scene's sphere turns metal: its pixels pass through
    upd = ctxs(BOX_DIFFUSE)
    old = upd.blend()                          # builds the per-triangle bsdfType array of the old table
    assert upd.update(metal)[0] == 0, upd.err()
    new = upd.blend()
    assert np.array_equal(new, ctxs(BOX_DIFFUSE, metal).blend())
    assert not np.array_equal(new, old)


def test_bookkeeping(ctxs):
    mats, ids = _scene(BOX)
    new_mats, new_ids = _edit("reassign", mats, ids)
    c = ctxs(BOX, light=1)
    h0 = c.handle()
    assert c.update(new_mats, new_ids)[0] == 0
    h1 = c.handle()
    assert h1 != h0
    assert c.render(handle=h0) != 0                   # a stale handle is refused
    fresh = ctxs(BOX, new_mats, new_ids, light=1)
    a, b = c.info(), fresh.info()
    for name, _ in _native.BvhInfo._fields_:
        if name == "build_ms":
            continue
        x, y = getattr(a, name), getattr(b, name)
        if name in ("half_area_ratio", "half_box_inflation"):      # summed with float atomics by every build
            assert x == pytest.approx(y, rel=1e-5), name
        else:
            assert (list(x) == list(y)) if hasattr(x, "__len__") else x == y, name
    # the new table without new ids, then a rebuild through pt_update_vertices keeps both
    assert c.update(_edit("recolour", new_mats, new_ids)[0])[0] == 0
    info = _native.UpdateInfo()
    assert c.L.pt_update_vertices(c.ctx, c.verts.ctypes.data, c.verts.size // 4, _native.UPDATE_REBUILD, C.byref(info)) == 0, c.err()
    assert info.rebuilt == 1 and c.handle() not in (h0, h1)
    _same_outcome(c, ctxs(BOX, _edit("recolour", new_mats, new_ids)[0], new_ids, light=1))


def test_refusals_leave_the_scene_alone(ctxs):
    mats, ids = _scene(BOX)
    c = ctxs(BOX, light=1)
    before, h = c.render(), c.handle()
    L = c.L
    n = len(ids)
    bad_type, bad_neg = _copy(mats), _copy(mats)
    bad_type[RED].bsdfType, bad_neg[RED].bsdfType = 3, -1
    out_of_range = ids.copy()
    out_of_range[7] = len(mats)
    refusals = [
        lambda: c.update(None),                                 # mats null, the scene has triangles
        lambda: c.update(None, n_mats=3),
        lambda: c.update(mats, ids, n_tris=n - 1),
        lambda: c.update(mats, ids, n_tris=n + 1),
        lambda: c.update(mats, out_of_range),
        lambda: c.update(mats[:METAL]),                         # a kept id (METAL) not below n_mats
        lambda: c.update(bad_type),
        lambda: c.update(bad_neg),
        lambda: c.update(mats[:1], n_mats=(1 << 24) + 1),       # refused on the count, before the table is read
    ]
    for i, f in enumerate(refusals):
        rc, _ = f()
        assert rc != 0, i
        assert b"pt_update_materials" in c.err(), i
        assert c.handle() == h, i
    for x, y in zip(c.render(), before):
        assert np.array_equal(x, y)
    assert L.pt_update_materials(None, None, 0, None, 0, None) != 0
    assert b"pt_update_materials" in L.pt_last_error(None)
    bare = _Ctx.__new__(_Ctx)
    bare.L, bare.ctx = L, C.c_void_p()
    assert L.pt_create(C.byref(bare.ctx), 0) == 0
    try:
        t = _table(mats)
        assert L.pt_update_materials(bare.ctx, C.addressof(t), len(t), None, 0, None) != 0
        assert b"no scene" in L.pt_last_error(bare.ctx)
    finally:
        bare.close()


def test_python_update_and_temporal_history(gpu_state_factory):
    kw = dict(width=64, height=48, spp=8, max_depth=6, direct_lighting=True, importance_sampling=True)
    import temporal_ref as tr
    results = []
    for motion in (False, True):
        for edit in (False, True):
            state, obj = gpu_state_factory(BOX, **kw)
            hist = pt.TemporalHistory(motion=motion)
            try:
                state.params.currentFrameIdx = 0
                pt.LaunchCurrentFrame(None, state)
                state.params.currentFrameIdx = 1
                hist.update(state)
                if edit:
                    h, serial = int(state.params.handle), state._mats_serial
                    mats = _copy(obj.getMaterials())
                    mats[RED].diffuse = _native.Float3(0.1, 0.7, 0.7)
                    out = pt.updateMaterials(state, mats, np.asarray(obj.getMaterialIndices(), np.int64))
                    assert out["rebuilt"] is False and out["area_ratio"] == 1.0
                    assert int(state.params.handle) != h and state._mats_serial == serial + 1
                tr.set_camera(state.params, *tr.orbit_camera(64, 48, 20, 0))
                state.refreshAccumulationBuffer = True
                pt.updateState(None, state)
                pt.LaunchCurrentFrame(None, state)
                state.params.currentFrameIdx = 1
                results.append(hist.update(state))
            finally:
                hist.close()
    for kept, dropped in (results[0:2], results[2:4]):
        assert (kept[..., 3] > 8).mean() > 0.3              # the history carried over ...
        assert np.all(dropped[..., 3] == 8)                 # ... unless the materials changed


def test_cli_set_material(built, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    base = [exe, "--width", "96", "--height", "64", "--spp-per-launch", "8", "--frames", "2", "--max-depth", "6", "--direct-lighting",
            "--light-mode", "1"]
    edits = ["--set-material", "red:kd=0.25,0.5,0.875", "--set-material", "light:ke=30,20,10,kd=0.5,0.5,0.5"]
    r = subprocess.run(base + ["--obj", BOX, "--out", str(tmp_path / "a.png")] + edits, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Material update:" in r.stdout
    # the same edits in a .mtl of its own
    mtl = open(os.path.join(pt.SCENES, "cornell_box.mtl")).read().split("\n")
    out, cur = [], None
    for line in mtl:
        t = line.split()
        if t and t[0] == "newmtl":
            cur = t[1]
        elif t and cur == "red" and t[0] == "Kd":
            line = "Kd 0.25 0.5 0.875"
        elif t and cur == "light" and t[0] == "Kd":
            line = "Kd 0.5 0.5 0.5"
        elif t and cur == "light" and t[0] == "Ke":
            line = "Ke 30 20 10"
        out.append(line)
    (tmp_path / "cornell_box.mtl").write_text("\n".join(out))
    shutil.copy(BOX, tmp_path / "box.obj")
    r = subprocess.run(base + ["--obj", str(tmp_path / "box.obj"), "--out", str(tmp_path / "b.png")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "a_material.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    assert (tmp_path / "a.png").read_bytes() != (tmp_path / "b.png").read_bytes()
    r = subprocess.run(base + ["--obj", BOX, "--out", str(tmp_path / "c.png"), "--set-material", "no_such_material:kd=1,1,1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "no material named" in r.stderr and not (tmp_path / "c.png").exists()
