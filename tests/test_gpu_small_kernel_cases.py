"""The small-scene render path (csrc/render_small.hip) outside the corridor of tests/test_gpu_small_kernel.py.  Every comparison is the
library's own choice (AUTO) against variant 7 named through pt_set_tuning, on the same context and inputs: accumulation bytes,
framebuffer bytes, the radiance / shadow / path / culled counters, and the path taken (BOTH for AUTO, OLD for variant 7) — over the
cameras, sample shapes and toggles of tests/small_kernel_cases.py, a changed light, grids as large as the device, trees of other
stack depths, edits of a live scene, a caller's stream; and once against the CPU oracle with the path asserted."""
import ctypes as C

import numpy as np
import pytest

import small_kernel_cases as sk
import tree_ref
from acgpathtracing_amd import _native
from scene_utils import make_params
from test_gpu_small_kernel import AUTO, BIG, BOTH, DIFFUSE, FAST, FULL, IEEE, LITTLE, OLD, ONLY_BIG, ONLY_LITTLE, Ctx, _budget, same

pytestmark = pytest.mark.gpu

PATH_OF = {AUTO: BOTH, ONLY_BIG: BIG, ONLY_LITTLE: LITTLE}
ALL_MODES = (AUTO, ONLY_BIG, ONLY_LITTLE)
W, H = 96, 64


def _f3(v):
    return _native.Float3(float(v[0]), float(v[1]), float(v[2]))


def params(cam, w=W, h=H, spp=16, depth=8, dl=True, imp=True):
    """make_params with a camera of small_kernel_cases: a name or an (eye, U, V, W)"""
    p = make_params(w, h, spp, depth, dl, imp)
    if cam != "reference":
        eye, U, V, Wv = sk.camera(cam, w, h) if isinstance(cam, str) else cam
        p.cameraEye, p.cameraU, p.cameraV, p.cameraW = _f3(eye), _f3(U), _f3(V), _f3(Wv)
    return p


def _materials(*diffuse):
    out = []
    for d in diffuse:
        m = _native.Material()
        m.diffuse = _native.Float3(*d); m.ior = 1.5; m.bsdfType = 0
        out.append(m)
    return out


THREE = ((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15))


class Scene(Ctx):
    """Ctx with scene replacement, vertex and material edits"""

    @classmethod
    def arrays(cls, scene, **kw):
        v, idx, ids = scene
        return cls(v, idx, _materials(*THREE), ids, **kw)

    def set_scene(self, verts, idx, mats, mat_ids):
        self.verts, self.idx = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(idx, np.uint32)
        self.mid = np.ascontiguousarray(mat_ids, np.uint32)
        self.mats = (_native.Material * len(mats))(*mats)
        assert self.L.pt_set_scene(self.ctx, self.verts.ctypes.data, self.verts.size // 4, self.idx.ctypes.data, self.idx.size // 3,
                                   self.mid.ctypes.data, C.addressof(self.mats), len(self.mats)) == 0, self.err()

    def update(self, verts, mode=_native.UPDATE_REFIT):
        v = np.ascontiguousarray(verts, np.float32)
        assert v.shape == self.verts.shape
        info = _native.UpdateInfo()
        assert self.L.pt_update_vertices(self.ctx, v.ctypes.data, v.size // 4, mode, C.byref(info)) == 0, self.err()
        self.verts = v
        return info

    def update_materials(self, mats, ids):
        t = (_native.Material * len(mats))(*mats)
        i = np.ascontiguousarray(ids, np.uint32)
        assert self.L.pt_update_materials(self.ctx, C.addressof(t), len(t), i.ctypes.data, i.size, None) == 0, self.err()
        self.mats, self.mid = t, i

    def render_windowed(self, p):
        """one launch under the library's own choice where that is variant 9 (Ctx.render holds every launch to variant 7):
        (accumulation, framebuffer, counters, path)"""
        L, n = self.L, p.width * p.height
        self.select(AUTO)
        acc, fb = C.c_void_p(), C.c_void_p()
        assert L.pt_device_malloc(self.ctx, C.byref(acc), n * 16) == 0 and L.pt_device_malloc(self.ctx, C.byref(fb), n * 4) == 0
        try:
            assert L.pt_device_memset(self.ctx, acc, 0, n * 16) == 0 and L.pt_device_memset(self.ctx, fb, 0, n * 4) == 0
            p.accumulationBuffer, p.frameBuffer, p.handle, p.currentFrameIdx = acc.value, fb.value, L.pt_scene_handle(self.ctx), 0
            assert L.pt_launch(self.ctx, C.byref(p)) == 0, self.err()
            st = self.stats()
            assert st.variant == 9
            a, b = np.zeros(n * 4, np.float32), np.zeros(n, np.uint32)
            assert L.pt_copy_to_host(self.ctx, a.ctypes.data, acc, n * 16) == 0 and L.pt_copy_to_host(self.ctx, b.ctypes.data, fb, n * 4) == 0
            return (a.view(np.uint32), b, np.array([st.radiance_rays, st.shadow_rays, st.paths, st.culled_rays], np.uint64),
                    L.pt_debug_small_kernel_path(self.ctx))
        finally:
            L.pt_device_free(self.ctx, acc); L.pt_device_free(self.ctx, fb)

    def stats(self):
        st = _native.Stats()
        assert self.L.pt_get_stats(self.ctx, C.byref(st)) == 0
        return st

    def fits(self):
        b = self.info()
        return _budget(b.n_nodes, b.stack_entries)

    def validate_tree(self):
        """the arrays the scene holds, read back and held to its triangles by tests/tree_ref.py"""
        import test_gpu_tree as tt
        arrays, ti = tt._read_held(self), tt._info(self)
        b = self.info()
        vs = tree_ref.validate(arrays, tree_ref.Info.of(ti), self.verts.reshape(-1, 4), self.idx.reshape(-1, 3), self.mid, morton=tt._morton(self),
                               stack_entries=b.stack_entries)
        assert vs == [], vs[:8]
        assert 3 in arrays                    # the fp16 centre / half-extent nodes the small kernel stages


def obj_scene(path, **kw):
    import acgpathtracing_amd as pt
    o = pt.TinyObjWrapper(path)
    mats = [_native.Material.from_buffer_copy(m) for m in o.getMaterials()]
    return Scene(o.getVerticesFloat(), o.getIndexBuffer(), mats, o.getMaterialIndices(), **kw)


def check(c, p, modes=(AUTO,), want=None, expect=None, **kw):
    """variant 7's answer on c (or `want`), and every mode's answer held to it; expect: the path AUTO must take (default BOTH).
    Returns variant 7's answer."""
    if want is None:
        want = c.render(p, "v7", **kw)
        assert want[3] == OLD
    for mode in modes:
        got = c.render(p, mode, **kw)
        path = PATH_OF[mode] if expect is None else expect
        assert got[3] == path, "mode %d took path %d, expected %d" % (mode, got[3], path)
        assert same(got, want), (mode, got[2], want[2], int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()))
    return want


@pytest.fixture(scope="module")
def box():
    """a context on cornell_box_diffuse.obj per math mode"""
    out = {m: obj_scene(DIFFUSE, math=m) for m in (IEEE, FAST)}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def stock(box):
    """variant 7's answer at the reference view, FAST"""
    return box[FAST].render(params("reference"), "v7")


# ---- a. cameras ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", [IEEE, FAST], ids=["ieee", "fast"])
@pytest.mark.parametrize("cam", sk.CAMERAS)
def test_cameras(box, cam, math):
    p = params(cam)
    want = check(box[math], p, ALL_MODES if cam in sk.PARTIAL_CAMERAS else (AUTO,))
    total, culled = W * H * 16, int(want[2][3])
    print(cam, "culled %d of %d" % (culled, total))
    assert int(want[2][2]) == total
    if cam == "away":
        assert culled == total and int(want[2][0]) == total and int(want[2][1]) == 0 and not want[0].view(np.float32).reshape(-1, 4)[:, :3].any()
    elif cam == "inside":
        assert culled == 0
    elif cam in sk.PARTIAL_CAMERAS:
        assert 0 < culled < total


def test_pulled_back_under_every_queue_order_and_pixel_class_setting(box):
    """rows that miss whole, rows that reach whole: the tile-strip orders and the host's row spans, on or off, change neither image nor counters"""
    c = box[FAST]
    L = c.L
    p = params("pulled_back")
    want = check(c, p)
    try:
        for order in range(4):
            for classes in (0, 1):
                assert L.pt_debug_queue_order(c.ctx, order) == 0 and L.pt_debug_pixel_classes(c.ctx, classes) == 0
                check(c, p, want=want)
    finally:
        assert L.pt_debug_queue_order(c.ctx, 1) == 0 and L.pt_debug_pixel_classes(c.ctx, 1) == 0


# ---- b. toggles and depths -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dl,imp,depth", sk.TOGGLES, ids=["dl%d-is%d-depth%d" % t for t in sk.TOGGLES])
def test_toggles_and_depths(box, dl, imp, depth):
    want = check(box[FAST], params("reference", depth=depth, dl=dl, imp=imp))
    assert (int(want[2][1]) > 0) == dl and int(want[2][2]) == W * H * 16
    assert int(want[2][0]) > int(want[2][2]) or depth == 1


@pytest.mark.parametrize("dl,imp,depth", [(False, False, 4), (True, True, 28)])
def test_toggles_with_glass_and_metal(dl, imp, depth):
    c = obj_scene(FULL)
    try:
        want = check(c, params("reference", depth=depth, dl=dl, imp=imp))
        assert (int(want[2][1]) > 0) == dl
    finally:
        c.close()


# ---- c. sample shapes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spp,chunks,frames", sk.SAMPLE_SHAPES, ids=["spp%d-chunks%d-frames%d" % s for s in sk.SAMPLE_SHAPES])
def test_sample_shapes_continue_an_accumulation(box, spp, chunks, frames):
    c = box[FAST]
    L = c.L
    assert L.pt_set_sample_chunks(c.ctx, chunks) == 0
    try:
        p = params("reference", spp=spp)
        first = c.render(p, "v7", frames=2)
        start = first[0].view(np.float32).copy()
        want = check(c, p, frames=frames, batch=True, frame0=2, start=start)
        assert c.stats().sample_chunks == 1 << sk.shifts(spp, chunks, frames)[0]
        assert int(want[2][2]) == W * H * spp * frames and not np.array_equal(want[0], first[0])
    finally:
        assert L.pt_set_sample_chunks(c.ctx, 0) == 0


# ---- d. a changed light ----------------------------------------------------------------------------------------------------------------

def _light(p, which):
    al = p.areaLight
    if which == "small":          # moved towards the left wall, a hundredth of the area, tinted
        al.corner = _native.Float3(140.0, 500.0, 300.0)
        al.v1, al.v2 = _native.Float3(0.0, 0.0, 10.5), _native.Float3(-13.0, 0.0, 0.0)
        al.emission = _native.Float3(900.0, 600.0, 300.0)
    else:                         # under the ceiling and facing it: the floor is behind the light
        al.corner = _native.Float3(343.0, 400.0, 227.0)
        al.v1, al.v2 = _native.Float3(-130.0, 0.0, 0.0), _native.Float3(0.0, 0.0, 105.0)
        al.normal = _native.Float3(0.0, 1.0, 0.0)
    return p


@pytest.mark.parametrize("which", ["small", "facing_up"])
def test_changed_light(box, stock, which):
    want = check(box[FAST], _light(params("reference"), which))
    assert not np.array_equal(want[0], stock[0]) and int(want[2][1]) > 0


# ---- e. full grids ---------------------------------------------------------------------------------------------------------------------

def _loaded_image(n_cus, cs, grants, h):
    """(w, h) of an image whose items are `grants` full first refills (64 items) of every wave of both grids at their cap of one
    workgroup per CU, 1280 threads a CU: neither grid can empty the queue before the other has started.  Neither side a multiple of
    the 8 x 4 tile."""
    items = grants * 1280 * n_cus * 64
    w = ((items >> cs) + h - 1) // h
    while w % 8 == 0:
        w += 1
    assert (w * h << cs) >= items >= 1024 * n_cus and w % 8 and h % 4 and w <= 65535
    return w, h


@pytest.mark.parametrize("spp,chunks,grants,h", [(16, 0, 1, 2046), (64, 32, 3, 1022)], ids=["4-runs", "32-runs"])
def test_grids_as_large_as_the_device(box, spp, chunks, grants, h):
    """Both grids at their cap of one workgroup per CU, 20 waves a CU numbered through wave0 into one fold scratch, and enough items
    that both work side by side: a wave's first refill takes at least 64 items, so a launch of 64 items a wave of the first grid is
    gone before the second grid has staged its nodes, whatever grid_blocks says.  Here every wave of both grids comes back to the
    queue many times (grants of 128 and 256 items).  With 32 runs a pixel a wave holds two groups at a time, in the same two fold
    slots from the first grant to the last."""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    cs = sk.shifts(spp, chunks, 1, pixels=1 << 21)[0]
    w, h = _loaded_image(n_cus, cs, grants, h)
    c = box[FAST]
    assert c.L.pt_set_sample_chunks(c.ctx, chunks) == 0
    try:
        p = params("reference", w=w, h=h, spp=spp)
        want = c.render(p, "v7")
        assert want[3] == OLD and c.stats().sample_chunks == 1 << cs
        for mode, blocks in ((AUTO, 2 * n_cus), (ONLY_BIG, n_cus), (ONLY_LITTLE, n_cus)):
            check(c, p, (mode,), want=want)
            assert c.stats().grid_blocks == blocks, (mode, c.stats().grid_blocks, n_cus)
    finally:
        assert c.L.pt_set_sample_chunks(c.ctx, 0) == 0


# ---- f. stack depths -------------------------------------------------------------------------------------------------------------------
# name: (scene, build mode (None: the default), camera); N and S as measured are in DESIGN.md section 4.2
def _blob(nu, nv):
    """Ctx.blob's scene as arrays"""
    from acgpathtracing_amd.scenes import make_scenes
    v, f = make_scenes.blob(nu, nv)
    verts = np.ones((len(v), 4), np.float32)
    verts[:, :3] = v * 150.0 + np.array([278.0, 274.0, 280.0])
    return verts, f.astype(np.uint32).reshape(-1, 3), np.zeros(len(f), np.uint32)


STACK_SCENES = {
    "lattice": (lambda: sk.lattice(28, 28), None, lambda: sk.aimed((278.0, 60.0, 280.0), (278.0, 420.0, -250.0), 520.0, W, H)),      # S 16
    "blob": (lambda: _blob(80, 9), None, lambda: sk.aimed((278.0, 274.0, 280.0), (278.0, 274.0, -250.0), 330.0, W, H)),                                                                      # S 20
    "box": (None, None, lambda: "reference"),                                                                                        # S 24
    "tail": (lambda: sk.tail(18, 800), None, lambda: sk.tail_camera(18, W, H)),                                                      # S 28
}
# a tree the budget admits (N 733 at S 36) and the gate does not: five workgroups of variant 7 no longer fit a CU from S = 32 on, the
# library's own choice there is the windowed-stack kernel, variant 9, and the small path stands in for variant 7 alone
TOO_DEEP = (lambda: sk.tail(24, 700), None, lambda: sk.tail_camera(24, W, H))
# N 1227 at S 28 in build mode 0, N 1227 at S 16 once its tail is spread over the floor: both inside the budget
REBUILT = (lambda: sk.tail(18, 1200), 0, lambda: sk.tail_camera(18, W, H))


def _stack_scene(name):
    make, mode, cam = STACK_SCENES[name] if isinstance(name, str) else name
    c = obj_scene(DIFFUSE, build_mode=mode) if make is None else Scene.arrays(make(), build_mode=mode)
    return c, cam()


@pytest.fixture(scope="module")
def stack_scenes():
    out = {name: _stack_scene(name) for name in STACK_SCENES}
    yield out
    for c, _ in out.values():
        c.close()


@pytest.mark.parametrize("name", list(STACK_SCENES))
def test_stack_depths(stack_scenes, name):
    c, cam = stack_scenes[name]
    b = c.info()
    print("%s: N %d, S %d, depth %d" % (name, b.n_nodes, b.stack_entries, b.max_depth))
    assert c.fits(), (b.n_nodes, b.stack_entries)
    c.validate_tree()
    for math in (FAST, IEEE):
        assert c.L.pt_set_math_mode(c.ctx, math) == 0
        want = check(c, params(cam, depth=6), ALL_MODES)
        assert int(want[2][0]) > int(want[2][3]) and int(want[2][3]) < W * H * 16 // 2       # most camera rays enter the tree


def test_stack_depths_differ(stack_scenes):
    seen = {name: c.info().stack_entries for name, (c, _) in stack_scenes.items()}
    s = set(seen.values())
    assert len(s) >= 4 and min(s) < 24 < max(s) and 24 in s, seen


def test_tree_too_deep_for_the_default_kernel_keeps_the_old_path():
    c, cam = _stack_scene(TOO_DEEP)
    try:
        b = c.info()
        print("too deep: N %d, S %d, depth %d" % (b.n_nodes, b.stack_entries, b.max_depth))
        assert c.fits() and b.stack_entries >= 32
        c.validate_tree()
        p = params(cam, depth=6)
        want = c.render(p, "v7")
        got = c.render_windowed(p)
        assert got[3] == OLD and want[3] == OLD and same(got, want), (got[2], want[2])
    finally:
        c.close()


# ---- g. edits on the default path --------------------------------------------------------------------------------------------------------

def _box_arrays():
    import acgpathtracing_amd as pt
    o = pt.TinyObjWrapper(DIFFUSE)
    mats = [_native.Material.from_buffer_copy(m) for m in o.getMaterials()]
    return (np.ascontiguousarray(o.getVerticesFloat(), np.float32).reshape(-1, 4), np.ascontiguousarray(o.getIndexBuffer(), np.uint32).reshape(-1, 3),
            mats, np.ascontiguousarray(o.getMaterialIndices(), np.uint32))


def _fresh_v7(v, idx, mats, ids, p, build_mode=None):
    """variant 7's answer of a context that received the data through pt_set_scene"""
    f = Scene(v, idx, mats, ids, build_mode=build_mode)
    try:
        out = f.render(p, "v7")
        assert out[3] == OLD
        return out, f.info().stack_entries
    finally:
        f.close()


def _auto_is(c, p, want):
    got = c.render(p, AUTO)
    assert got[3] == (BOTH if c.fits() else OLD), (got[3], c.info().n_nodes, c.info().stack_entries)
    assert same(got, want), (got[2], want[2], int((got[0] != want[0]).sum()))
    return got


def test_refits_on_the_default_path():
    from test_gpu_update import _object_vertices
    v, idx, mats, ids = _box_arrays()
    short = _object_vertices(DIFFUSE, "short_block")
    moved = v.copy(); moved[short, :3] += np.float32([-90.0, 60.0, 120.0])          # inside the room
    grown = v.copy(); grown[short, :3] += np.float32([420.0, 0.0, -160.0])           # out through a side wall and the open front: the scene box
    assert np.abs(grown[:, :3]).max() > np.abs(v[:, :3]).max() + 100                # grows (cull box, row spans), and so does the largest
    assert grown[:, 2].min() < v[:, 2].min()                                        # coordinate (skip_base)
    p = params("reference")
    c = Scene(v, idx, mats, ids)
    try:
        first = _auto_is(c, p, _fresh_v7(v, idx, mats, ids, p)[0])
        box_of = lambda: tuple(c.info().scene_lo) + tuple(c.info().scene_hi)
        lo0 = box_of()
        for target in (moved, grown):
            c.update(target)
            want, _ = _fresh_v7(target, idx, mats, ids, p)
            got = _auto_is(c, p, want)
            assert got[3] == BOTH and not np.array_equal(got[0], first[0])
        assert box_of()[2] < lo0[2] and box_of()[3] > lo0[3] + 100
        c.update(v)                                                                 # the round trip
        back = c.render(p, AUTO)
        assert back[3] == BOTH and same(back, first) and box_of() == lo0
        check(c, p, ALL_MODES)
    finally:
        c.close()


def test_rebuild_that_changes_the_stack_depth():
    make, mode, cam = REBUILT
    v, idx, ids = make()
    mats = _materials(*THREE)
    flat = sk.spread(v)
    c = Scene(v, idx, mats, ids, build_mode=mode)
    try:
        s0 = c.info().stack_entries
        assert c.fits()
        for target, view in ((flat, "reference"), (v, cam())):
            info = c.update(target, _native.UPDATE_REBUILD)
            assert info.rebuilt == 1
            p = params(view, depth=6)
            want, s_fresh = _fresh_v7(target, idx, mats, ids, p, build_mode=mode)
            assert c.info().stack_entries == s_fresh
            print("after the rebuild: N %d, S %d, small path %s" % (c.info().n_nodes, s_fresh, c.fits()))
            assert _auto_is(c, p, want)[3] == BOTH          # other stack sizes, other dynamic LDS, the same context
            assert (s_fresh != s0) if target is flat else (s_fresh == s0)
    finally:
        c.close()


def test_material_edits_on_the_default_path():
    from test_gpu_update import _object_vertices
    v, idx, mats, ids = _box_arrays()
    tall = np.all(np.isin(idx, _object_vertices(DIFFUSE, "tall_block")), axis=1)
    assert 0 < tall.sum() < len(idx)
    glass = [_native.Material.from_buffer_copy(m) for m in mats]
    m = _native.Material()                       # a material of the tall block's own, at the end of a longer table
    m.diffuse = _native.Float3(1.0, 1.0, 1.0); m.ior = 1.5; m.bsdfType = 2
    glass.append(m)
    new_ids = ids.copy()
    new_ids[tall] = len(glass) - 1
    p = params("reference", depth=12)
    c = Scene(v, idx, mats, ids)
    try:
        first = _auto_is(c, p, _fresh_v7(v, idx, mats, ids, p)[0])
        c.update_materials(glass, new_ids)
        got = _auto_is(c, p, _fresh_v7(v, idx, glass, new_ids, p)[0])
        assert got[3] == BOTH and not np.array_equal(got[0], first[0])
        c.update_materials(mats, ids)
        back = c.render(p, AUTO)
        assert back[3] == BOTH and same(back, first)
    finally:
        c.close()


def test_scenes_replaced_across_the_gate(stock):
    """diffuse box -> a blob too large for the path -> the box with glass and metal -> diffuse box, on one context"""
    import acgpathtracing_amd as pt
    from acgpathtracing_amd.scenes import make_scenes
    v, idx, mats, ids = _box_arrays()
    full = pt.TinyObjWrapper(FULL)
    bv, bf = make_scenes.blob(144, 9)
    blob_v = np.ones((len(bv), 4), np.float32)
    blob_v[:, :3] = bv * 150.0 + np.array([278.0, 274.0, 280.0])
    p = params("reference")
    c = Scene(v, idx, mats, ids)
    try:
        assert same(check(c, p), stock)
        c.set_scene(blob_v, bf.astype(np.uint32).ravel(), _materials((0.6, 0.5, 0.4)), np.zeros(len(bf), np.uint32))
        assert not c.fits()
        blob = (blob_v, bf.astype(np.uint32).ravel(), _materials((0.6, 0.5, 0.4)), np.zeros(len(bf), np.uint32))
        check(c, p, expect=OLD, want=_fresh_v7(*blob, p)[0])
        check(c, p, expect=OLD)
        c.set_scene(full.getVerticesFloat(), full.getIndexBuffer(), [_native.Material.from_buffer_copy(m) for m in full.getMaterials()], full.getMaterialIndices())
        assert c.fits()
        glassy = _fresh_v7(full.getVerticesFloat(), full.getIndexBuffer(), [_native.Material.from_buffer_copy(m) for m in full.getMaterials()],
                           full.getMaterialIndices(), p)[0]
        check(c, p, want=glassy)
        assert same(check(c, p), glassy) and not np.array_equal(glassy[0], stock[0])
        c.set_scene(v, idx, mats, ids)
        assert same(check(c, p, ALL_MODES), stock)
    finally:
        c.close()


def test_back_from_fp32_nodes():
    """pt_set_tuning(0, 1) holds fp32 nodes and refits them in place; back on the library's choice the fp16 nodes are the refitted tree's"""
    from test_gpu_update import _object_vertices
    v, idx, mats, ids = _box_arrays()
    moved = v.copy(); moved[_object_vertices(DIFFUSE, "short_block"), :3] += np.float32([-90.0, 60.0, 120.0])
    p = params("reference")
    c = Scene(v, idx, mats, ids)
    try:
        L = c.L
        n = W * H
        acc = C.c_void_p()
        assert L.pt_device_malloc(c.ctx, C.byref(acc), n * 16) == 0
        try:
            assert L.pt_set_tuning(c.ctx, 0, 1) == 0
            p.accumulationBuffer, p.frameBuffer, p.handle, p.currentFrameIdx = acc.value, None, L.pt_scene_handle(c.ctx), 0
            assert L.pt_launch(c.ctx, C.byref(p)) == 0, c.err()
            assert c.stats().variant == 1 and L.pt_debug_small_kernel_path(c.ctx) == OLD
            c.update(moved)
        finally:
            L.pt_device_free(c.ctx, acc)
        got = _auto_is(c, p, _fresh_v7(moved, idx, mats, ids, p)[0])
        assert got[3] == BOTH
    finally:
        c.close()


def test_two_live_contexts_take_turns():
    """two eligible scenes of different dynamic LDS sizes on one kernel symbol"""
    a, b = obj_scene(DIFFUSE), Scene.arrays(sk.lattice(28, 28))
    try:
        assert a.fits() and b.fits() and (a.info().n_nodes, a.info().stack_entries) != (b.info().n_nodes, b.info().stack_entries)
        p = params("reference")
        want = {a: a.render(p, "v7"), b: b.render(p, "v7")}
        for _ in range(3):
            for c in (a, b):
                check(c, p, want=want[c])
    finally:
        a.close(); b.close()


# ---- h. a caller's stream ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("classes", [1, 0], ids=["same-view", "one-pixel"])
def test_callers_stream(box, classes):
    """On a torch stream: a short launch, then torch work and the starting accumulation produced on the stream with no host
    synchronisation ahead of pt_launch_frames.  Both grids have to queue behind what the stream holds.  A 256-thread grid that ran
    ahead would take items of the new launch from where the short launch left the queue heads, before the launch's own reset of
    heads and counters; the image is large enough (test_grids_as_large_as_the_device) that it would still be at work when the reset
    comes, and what it had traced until then would be counted on top of the launch proper.  The short launch is one sample a pixel
    of the same view (the row spans stay; nothing in the launch waits for the stream), or, with the pixel classes off, a single
    pixel, which leaves the heads near zero."""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    spp = 32
    cs = sk.shifts(spp, 0, 1, pixels=1 << 21)[0]
    w, h = _loaded_image(n_cus, cs, 1, 1022)
    assert w * h >= 1 << 20
    c = box[FAST]
    L = c.L
    p = params("reference", w=w, h=h, spp=spp)
    first = c.render(p, "v7", frames=2)
    start = first[0].view(np.float32).copy()
    want = c.render(p, "v7", batch=True, frame0=2, start=start)
    assert c.stats().sample_chunks == 1 << cs and int(want[2][2]) == w * h * spp
    c.select(AUTO)
    dev = torch.device("cuda", 0)
    base = torch.from_numpy(start).to(dev)
    acc, fb = torch.empty_like(base), torch.zeros(w * h, dtype=torch.int32, device=dev)
    short_acc = torch.zeros_like(base)
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    short = params("reference", w=w, h=h, spp=1) if classes else params("reference", w=1, h=1, spp=1)

    def launch(q, a, f, frames, frame0):
        q.accumulationBuffer, q.frameBuffer, q.handle, q.currentFrameIdx = a.data_ptr(), (f.data_ptr() if f is not None else None), L.pt_scene_handle(c.ctx), frame0
        assert L.pt_launch_frames(c.ctx, C.byref(q), frames) == 0, c.err()
        st = c.stats()
        return np.array([st.radiance_rays, st.shadow_rays, st.paths, st.culled_rays], np.uint64), L.pt_debug_small_kernel_path(c.ctx)

    try:
        assert L.pt_debug_pixel_classes(c.ctx, classes) == 0
        with torch.cuda.stream(side):
            assert L.pt_set_stream(c.ctx, C.c_void_p(side.cuda_stream)) == 0
            for work in (0, 4):                                       # 4: milliseconds, less than the 256-thread grid alone would need for the image
                assert launch(short, short_acc, None, 1, 0)[1] == BOTH
                junk = big
                for _ in range(work):
                    junk = junk @ big * 1e-2                          # work the launch has to queue behind
                acc.fill_(float("nan"))
                acc.copy_(base + junk[0, 0] * 0.0)                    # depends on the work above
                acc.copy_(base)
                counts, path = launch(p, acc, fb, 1, 2)
                side.synchronize()
                got = acc.cpu().numpy().view(np.uint32), fb.cpu().numpy().view(np.uint32), counts, path
                assert got[3] == BOTH and same(got, want), (work, got[2], want[2])
        assert L.pt_set_stream(c.ctx, None) == 0
        torch.cuda.synchronize()
        check(c, p, batch=True, frame0=2, start=start, want=want)
    finally:
        assert L.pt_set_stream(c.ctx, None) == 0 and L.pt_debug_pixel_classes(c.ctx, 1) == 0


# ---- i. the oracle as a second witness ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", ["pulled_back", "reference"])
def test_oracle_witness(oracle, cam):
    """the library's own choice with the path asserted, against the CPU oracle at the bars of test_gpu_shapes.test_kernel_rows_at_edge_shapes"""
    from test_gpu_parity import MSE_TOL, SAME_BITS_MIN
    from test_gpu_shapes import oracle_render
    from scene_utils import image_mse
    c = obj_scene(DIFFUSE, math=IEEE)
    sc = oracle.scene(c.verts, c.idx, c.mid, c.mats)
    try:
        assert c.L.pt_set_sample_chunks(c.ctx, 1) == 0
        same_n = same_d = 0
        rays = [0, 0, 0, 0]
        for w, h in ((31, 33), (96, 64)):
            spp = 4
            p = params(cam, w=w, h=h, spp=spp, depth=6)
            a, _, counts, path = c.render(p, AUTO)
            assert path == BOTH
            acc = a.view(np.float32).reshape(h, w, 4)
            ref, _, ref_st = oracle_render(sc, p)
            mse = image_mse(acc, ref)
            assert np.isfinite(acc).all() and mse < MSE_TOL, (cam, w, h, mse)
            assert int(counts[2]) == ref_st["paths"] == w * h * spp
            same_n += int(np.all(acc.view(np.uint32) == ref.view(np.uint32), axis=-1).sum())
            same_d += w * h
            rays[0] += int(counts[0]); rays[1] += ref_st["radiance_rays"]
            rays[2] += int(counts[1]); rays[3] += ref_st["shadow_rays"]
        print("%s: %.4f of %d pixels bit-identical; radiance rays %d / %d, shadow rays %d / %d" % ((cam, same_n / same_d, same_d) + tuple(rays)))
        assert same_n / same_d > SAME_BITS_MIN
        assert abs(rays[0] - rays[1]) <= 2e-3 * rays[1] and abs(rays[2] - rays[3]) <= 2e-3 * max(1, rays[3])
    finally:
        c.close()
        sc.close()
