"""The small-scene render path (csrc/render_small.hip: BVH nodes from LDS, one 1024-thread and one 256-thread workgroup per CU) against
the kernel it stands in for, variant 7 named through pt_set_tuning: accumulation buffer, framebuffer and ray / path / culled counters
byte for byte — single launches in both math modes, frame batches onto an existing accumulation at 1 and 8 sample chunks, a rank's
partition, each grid alone, images smaller than a workgroup; which launches take the path and which do not; the references of the
real trees through the 16-bit encoding."""
import ctypes as C
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
from acgpathtracing_amd.scenes import make_scenes
from scene_utils import make_params

pytestmark = pytest.mark.gpu

DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
FULL = os.path.join(pt.SCENES, "cornell_box.obj")
IEEE, FAST = _native.MATH_IEEE, _native.MATH_FAST
OLD, BOTH, BIG, LITTLE = 0, 1, 2, 3                       # pt_debug_small_kernel_path
AUTO, OFF, ONLY_BIG, ONLY_LITTLE = 0, 1, 2, 3             # pt_debug_small_kernel
CU_LDS = 160 * 1024                                       # MI355X: LDS of a CU


class Ctx:
    def __init__(self, verts, idx, mats, mat_ids, math=FAST, build_mode=None):
        self.L = L = _native.hip()
        self.ctx = C.c_void_p()
        assert L.pt_create(C.byref(self.ctx), 0) == 0
        assert L.pt_set_math_mode(self.ctx, math) == 0
        if build_mode is not None:
            assert L.pt_set_build_mode(self.ctx, build_mode) == 0
        self.verts, self.idx = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(idx, np.uint32)
        self.mid = np.ascontiguousarray(mat_ids, np.uint32)
        self.mats = (_native.Material * len(mats))(*mats)
        assert L.pt_set_scene(self.ctx, self.verts.ctypes.data, self.verts.size // 4, self.idx.ctypes.data, self.idx.size // 3,
                              self.mid.ctypes.data, C.addressof(self.mats), len(self.mats)) == 0, self.err()

    @classmethod
    def obj(cls, path, **kw):
        o = pt.TinyObjWrapper(path)
        mats = [_native.Material.from_buffer_copy(m) for m in o.getMaterials()]
        return cls(o.getVerticesFloat(), o.getIndexBuffer(), mats, o.getMaterialIndices(), **kw)

    @classmethod
    def blob(cls, nu, nv, **kw):
        """make_scenes.blob(nu, nv) (2 nu (nv - 1) triangles, no randomness) hung in the middle of the reference's camera view"""
        v, f = make_scenes.blob(nu, nv)
        verts = np.ones((len(v), 4), np.float32)
        verts[:, :3] = v * 150.0 + np.array([278.0, 274.0, 280.0])
        m = _native.Material()
        m.diffuse = _native.Float3(0.6, 0.5, 0.4); m.ior = 1.5; m.bsdfType = 0
        return cls(verts, f.astype(np.uint32).ravel(), [m], np.zeros(len(f), np.uint32), **kw)

    def err(self):
        return self.L.pt_last_error(self.ctx)

    def info(self):
        b = _native.BvhInfo()
        assert self.L.pt_get_bvh_info(self.ctx, C.byref(b)) == 0
        return b

    def select(self, mode):
        """mode: a pt_debug_small_kernel mode, or "v7": variant 7 named through pt_set_tuning"""
        L = self.L
        if mode == "v7":
            assert L.pt_debug_small_kernel(self.ctx, AUTO) == 0 and L.pt_set_tuning(self.ctx, 0, 7) == 0
        else:
            assert L.pt_set_tuning(self.ctx, 0, -1) == 0 and L.pt_debug_small_kernel(self.ctx, mode) == 0

    def render(self, p, mode, frames=1, batch=False, frame0=0, start=None):
        """(accumulation bytes, framebuffer bytes, counters, path) of `frames` frames from frame0, onto `start` (accumulation of the
        frames before frame0) or a zeroed buffer"""
        L, n = self.L, p.width * p.height
        self.select(mode)
        acc, fb = C.c_void_p(), C.c_void_p()
        assert L.pt_device_malloc(self.ctx, C.byref(acc), n * 16) == 0 and L.pt_device_malloc(self.ctx, C.byref(fb), n * 4) == 0
        try:
            if start is None:
                assert L.pt_device_memset(self.ctx, acc, 0, n * 16) == 0
            else:
                assert L.pt_copy_to_device(self.ctx, acc, start.ctypes.data, n * 16) == 0
            assert L.pt_device_memset(self.ctx, fb, 0, n * 4) == 0
            p.accumulationBuffer, p.frameBuffer, p.handle = acc.value, fb.value, L.pt_scene_handle(self.ctx)
            counts = np.zeros(4, np.uint64)
            paths = []
            st = _native.Stats()
            for f in ([frame0] if batch else range(frame0, frame0 + frames)):
                p.currentFrameIdx = f
                rc = L.pt_launch_frames(self.ctx, C.byref(p), frames) if batch else L.pt_launch(self.ctx, C.byref(p))
                assert rc == 0, self.err()
                assert L.pt_get_stats(self.ctx, C.byref(st)) == 0
                counts += np.array([st.radiance_rays, st.shadow_rays, st.paths, st.culled_rays], np.uint64)
                paths.append(L.pt_debug_small_kernel_path(self.ctx))
                assert st.variant == 7
            assert len(set(paths)) == 1
            a, b = np.zeros(n * 4, np.float32), np.zeros(n, np.uint32)
            assert L.pt_copy_to_host(self.ctx, a.ctypes.data, acc, n * 16) == 0 and L.pt_copy_to_host(self.ctx, b.ctypes.data, fb, n * 4) == 0
            return a.view(np.uint32), b, counts, paths[0]
        finally:
            L.pt_device_free(self.ctx, acc); L.pt_device_free(self.ctx, fb)

    def close(self):
        self.L.pt_destroy(self.ctx)


def same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


@pytest.fixture(scope="module")
def diffuse():
    """one context on cornell_box_diffuse.obj per math mode, with variant 7's answer at 96 x 64, 16 spp, depth 8, DL + IS"""
    out = {}
    for math in (IEEE, FAST):
        c = Ctx.obj(DIFFUSE, math=math)
        out[math] = (c, c.render(make_params(96, 64, 16, 8, True, True), "v7"))
        assert out[math][1][3] == OLD
    yield out
    for c, _ in out.values():
        c.close()


@pytest.mark.parametrize("math", [IEEE, FAST])
@pytest.mark.parametrize("mode,path", [(AUTO, BOTH), (ONLY_BIG, BIG), (ONLY_LITTLE, LITTLE)])
def test_single_launch_matches_variant_7(diffuse, math, mode, path):
    """both grids together, and each alone (two independent consumers of one queue): the same bytes and counters"""
    c, want = diffuse[math]
    got = c.render(make_params(96, 64, 16, 8, True, True), mode)
    assert got[3] == path and same(got, want), (got[2], want[2])
    assert want[2][0] > 96 * 64 * 16 and want[2][1] > 0


@pytest.mark.parametrize("chunks", [1, 8])
def test_frame_batch_continues_an_accumulation(diffuse, chunks):
    c, _ = diffuse[FAST]
    L = c.L
    assert L.pt_set_sample_chunks(c.ctx, chunks) == 0
    try:
        p = make_params(96, 64, 16, 8, True, True)
        first = c.render(p, "v7", frames=2)
        start = first[0].view(np.float32).copy()
        want = c.render(p, "v7", frames=3, batch=True, frame0=2, start=start)
        got = c.render(p, AUTO, frames=3, batch=True, frame0=2, start=start)
        assert got[3] == BOTH and want[3] == OLD and same(got, want)
        assert not np.array_equal(want[0], first[0])
    finally:
        assert L.pt_set_sample_chunks(c.ctx, 0) == 0


def test_partition_of_a_rank(diffuse):
    """pt_set_partition(1, 4): a quarter of the tiles"""
    c, _ = diffuse[FAST]
    L = c.L
    assert L.pt_set_partition(c.ctx, 1, 4) == 0
    try:
        p = make_params(96, 64, 16, 8, True, True)
        want = c.render(p, "v7")
        got = c.render(p, AUTO)
        assert same(got, want) and got[3] == BOTH and want[3] == OLD
    finally:
        assert L.pt_set_partition(c.ctx, 0, 1) == 0


@pytest.mark.parametrize("w,h", [(1, 64), (1, 1)])
def test_less_work_than_a_workgroup(diffuse, w, h):
    c, _ = diffuse[FAST]
    p = make_params(w, h, 16, 8, True, True)
    want = c.render(p, "v7")
    for mode, path in ((AUTO, BOTH), (ONLY_BIG, BIG), (ONLY_LITTLE, LITTLE)):
        got = c.render(p, mode)
        assert got[3] == path and same(got, want), mode
    assert want[2][2] == w * h * 16


def test_glass_and_metal():
    """cornell_box.obj at depth 16: shade_hit is shared, so config 3's materials come with it"""
    c = Ctx.obj(FULL)
    try:
        p = make_params(64, 64, 16, 16, True, True)
        want = c.render(p, "v7")
        got = c.render(p, AUTO)
        assert got[3] == BOTH and want[3] == OLD and same(got, want)
    finally:
        c.close()


def _budget(n_nodes, stack_entries):
    """the LDS budget of DESIGN.md section 4.2, stated here on its own: two copies of the nodes, 20 waves of 16-bit stacks, 20 books, two LCG tables;
    a workgroup's share counted in whole KB where it has to fit"""
    big = 16 * stack_entries * 128 + n_nodes * 32 + 256 + 16 * 320
    little = 4 * stack_entries * 128 + n_nodes * 32 + 256 + 4 * 320
    kb = lambda b: (b + 1023) // 1024 * 1024
    return n_nodes <= 2048 and kb(big) + kb(little) <= CU_LDS and big + 2 * little > CU_LDS


def test_gate_on_scene_size():
    """blobs of 1024 ... 2304 triangles straddle the LDS limit (and the last one the node limit): on each, the path taken is what the
    budget says, on both sides of it, and the bytes are variant 7's"""
    seen = set()
    for nu in (64, 80, 88, 96, 112, 144):
        c = Ctx.blob(nu, 9)
        try:
            b = c.info()
            fits = _budget(b.n_nodes, b.stack_entries)
            out = np.zeros(5, np.uint64)
            assert c.L.pt_debug_small_budget(b.n_nodes, b.n_tris, b.stack_entries, CU_LDS, out.ctypes.data) == 0 and bool(out[2]) == fits
            p = make_params(48, 32, 4, 6, True, True)
            want = c.render(p, "v7")
            got = c.render(p, AUTO)
            assert got[3] == (BOTH if fits else OLD) and same(got, want), (nu, b.n_nodes, b.stack_entries)
            assert c.render(p, OFF)[3] == OLD
            seen.add(fits)
        finally:
            c.close()
    assert seen == {True, False}


def test_gate_on_what_the_caller_chose(diffuse):
    """automatic mode on an eligible scene; an environment map, light mode 1, a named variant or the hook's "off" keep today's kernels"""
    c, want = diffuse[FAST]
    L = c.L
    p = make_params(96, 64, 16, 8, True, True)
    got = c.render(p, AUTO)
    assert got[3] == BOTH and same(got, want)
    assert c.render(p, OFF)[3] == OLD
    st = _native.Stats()

    def launch(mode):
        assert L.pt_debug_small_kernel(c.ctx, mode) == 0
        n = p.width * p.height * 16
        buf = C.c_void_p()
        assert L.pt_device_malloc(c.ctx, C.byref(buf), n) == 0
        try:
            p.accumulationBuffer, p.frameBuffer, p.handle, p.currentFrameIdx = buf.value, None, L.pt_scene_handle(c.ctx), 0
            assert L.pt_launch(c.ctx, C.byref(p)) == 0, c.err()
            assert L.pt_get_stats(c.ctx, C.byref(st)) == 0
            return L.pt_debug_small_kernel_path(c.ctx), int(st.variant)
        finally:
            L.pt_device_free(c.ctx, buf)

    try:
        assert L.pt_set_tuning(c.ctx, 0, -1) == 0
        sky = np.full((8, 16, 3), 0.5, np.float32)
        assert L.pt_set_environment(c.ctx, sky.ctypes.data, 16, 8, _native.Float3(1.0, 1.0, 1.0)) == 0
        assert launch(AUTO) == (OLD, 10)
        assert L.pt_set_environment(c.ctx, None, 0, 0, _native.Float3(1.0, 1.0, 1.0)) == 0
        assert L.pt_set_light_mode(c.ctx, 1) == 0
        assert launch(AUTO) == (OLD, 8)
        assert L.pt_set_light_mode(c.ctx, 0) == 0
        assert launch(AUTO) == (BOTH, 7)
        for v in (7, 9, 1):
            assert L.pt_set_tuning(c.ctx, 0, v) == 0
            assert launch(AUTO) == (OLD, v)
        assert L.pt_set_tuning(c.ctx, 2, -1) == 0       # blocks per CU named: the caller is tuning the variant table's kernel
        assert launch(AUTO) == (OLD, 7)
    finally:
        assert L.pt_set_environment(c.ctx, None, 0, 0, _native.Float3(1.0, 1.0, 1.0)) == 0
        assert L.pt_set_light_mode(c.ctx, 0) == 0 and L.pt_set_tuning(c.ctx, 0, -1) == 0 and L.pt_debug_small_kernel(c.ctx, AUTO) == 0


@pytest.mark.parametrize("scene", [DIFFUSE, FULL])
def test_references_of_the_real_trees_round_trip(scene):
    """every child word of the fp16 nodes as the device holds them, and the sentinel"""
    c = Ctx.obj(scene)
    try:
        L = c.L
        info = _native.TreeInfo()
        assert L.pt_debug_read_tree(c.ctx, 0, None, 0, C.byref(info)) == 0
        nodes = np.zeros((info.n_nodes, 8), np.uint32)
        assert L.pt_debug_read_tree(c.ctx, 3, nodes.ctypes.data, nodes.nbytes, None) == 0, c.err()
        refs = np.concatenate([nodes[:, 3], nodes[:, 7], np.array([0x7FFFFFFF], np.uint32)]).view(np.int32).copy()
        inner, leaf = refs[(refs >= 0) & (refs != 0x7FFFFFFF)], refs[refs < 0]
        assert len(inner) == info.n_nodes - 1 and len(leaf) == info.n_tris and (inner % 32 == 0).all() and inner.max() == 32 * (info.n_nodes - 1)
        assert sorted(~leaf) == list(range(info.n_tris))
        enc, dec, loc = np.zeros(len(refs), np.uint16), np.zeros(len(refs), np.int32), np.zeros(len(refs), np.int32)
        assert L.pt_debug_small_ref(refs.ctypes.data, len(refs), enc.ctypes.data, dec.ctypes.data, loc.ctypes.data) == 0
        assert np.array_equal(dec, refs) and len(set(enc.tolist())) == len(refs)
        assert np.array_equal(loc, enc.view(np.int16).astype(np.int32)) and loc[-1] == 0x7FFF
    finally:
        c.close()
