"""Triangle-against-mesh queries on the GPU: pt_query_triangles and pt_query_triangles_any against tests/tritri_ref.py's brute force
(every count, index and any byte, bits) on every scene, size, query set and list length, the triangles that are a miss before any
traversal, the outputs' bounds, the scene's memory, scene edits, the render state, the refusals, the counting twin, torch tensors,
meshCollisions and acgpt_main --intersect."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import nearest_ref as nr
import tritri_ref as tt
from test_gpu_overlap import BOX, BOX_DIFFUSE, PARENT_KERNEL_HASH, GUARD, _L, _err, _camera, _host_closest, _fresh_state

F = np.float32
pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
MAX_PRIMS = (0, 1, 3, 4, 8)


class _DeviceTris:
    """query triangles in a device buffer, and buffers for the three outputs with a guard behind each; the C ABI called as a C caller
    would.  Every call may take a prefix of the triangles."""
    def __init__(self, state, recs):
        self.state, self.n = state, recs.shape[0]
        self.recs = np.ascontiguousarray(recs, np.float32)
        assert self.recs.shape == (self.n, 12)
        m = max(self.n, 1)
        self.bufs = pt.pathtracer._device_buffers(state, 1, m * 48) + pt.pathtracer._device_buffers(state, 1, m * 32 + GUARD) + \
            pt.pathtracer._device_buffers(state, 1, m * 4 + GUARD) + pt.pathtracer._device_buffers(state, 1, m + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.recs.ctypes.data, self.recs.nbytes) == 0

    def _fill(self, buf, nbytes):
        assert _L().pt_device_memset(self.state.context, buf, 0xCD, nbytes + GUARD) == 0

    def _read(self, buf, nbytes, what):
        raw = np.zeros(nbytes + GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, buf, raw.nbytes) == 0
        assert (raw[nbytes:] == 0xCD).all(), "%s: written past its end" % what
        return raw[:nbytes]

    def triangles(self, k, counts=True, n=None):
        """(prims uint32 [n, k] or None, counts uint32 [n] or None)"""
        n = self.n if n is None else n
        L, s = _L(), self.state
        _, d_prims, d_counts, _ = self.bufs
        self._fill(d_prims, n * k * 4)
        self._fill(d_counts, n * 4)
        assert L.pt_query_triangles(s.context, self.bufs[0], n, k, d_prims if k else None, d_counts if counts else None) == 0, _err(s)
        prims = self._read(d_prims, n * k * 4, "prims").view(np.uint32).reshape(n, k)
        cnt = self._read(d_counts, n * 4 if counts else 0, "counts").view(np.uint32)
        return (prims if k else None), (cnt if counts else None)

    def any(self, n=None):
        n = self.n if n is None else n
        self._fill(self.bufs[3], n)
        assert _L().pt_query_triangles_any(self.state.context, self.bufs[0], n, self.bufs[3]) == 0, _err(self.state)
        return self._read(self.bufs[3], n, "hit")

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _check_all(state, recs, ref, sizes=SIZES, ks=MAX_PRIMS, what=()):
    """Every count, index and any byte of the device equals ref = (counts, prims at 8, any) at every n and max_prims, with and without
    counts"""
    counts, prims, hit = ref
    d = _DeviceTris(state, recs)
    try:
        for n in sorted(set(min(n, recs.shape[0]) for n in sizes)):
            got = d.any(n)
            assert np.array_equal(got, hit[:n]), what + ("any", n, np.flatnonzero(got != hit[:n])[:4])
            for k in ks:
                for with_counts in ((True,) if k == 0 else (True, False)):
                    p, c = d.triangles(k, with_counts, n)
                    if with_counts:
                        assert np.array_equal(c, counts[:n]), what + ("counts", n, k, np.flatnonzero(c != counts[:n])[:4], c[c != counts[:n]][:4], counts[:n][c != counts[:n]][:4])
                    if k:
                        bad = np.flatnonzero((p != prims[:n, :k]).any(axis=1))
                        assert bad.size == 0, what + ("prims", n, k, with_counts, bad[:4], p[bad][:2], prims[:n, :k][bad][:2])
    finally:
        d.free()


def _reference(obj, recs, chunk=1024):
    ref = tt.triangle_records(recs, obj.getVerticesFloat(), obj.getIndexBuffer(), tt.MAX_PRIMS, chunk=chunk)
    for a in ref:
        a.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def scenes(gpu_state_factory):
    """The three scenes, each set up once: the Cornell fixtures under the default variant (fp16 centre / half-extent nodes) and the
    box under an fp32-node variant.  name -> (state, obj)"""
    made = {}
    extra = []

    def get(name):
        if name not in made:
            if name == "fp32":
                base, obj = get("box")
                state = _fresh_state(base, obj, tuning=1)           # variant 1: fp32 nodes
                extra.append(state)
                made[name] = (state, obj)
            else:
                made[name] = gpu_state_factory({"box": BOX, "diffuse": BOX_DIFFUSE}[name], width=97, height=61, max_depth=4, spp=8)
        return made[name]

    yield get
    for s in extra:
        pt.CleanAllTheThings(s)


@pytest.fixture(scope="module")
def references(scenes):
    """(scene, set) -> (records, (counts, prims at 8, any)) by the brute force on the whole set: computed once, shared, never written.
    The fp32-node scene is the box: it shares the box's."""
    cache = {}

    def get(scene, name):
        key = ("box" if scene == "fp32" else scene, name)
        if key not in cache:
            state, obj = scenes(key[0])
            recs = tt.query_set(name, obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state), first_hits=lambda rays: _host_closest(state, rays))
            recs.setflags(write=False)
            cache[key] = (recs, _reference(obj, recs))
        return cache[key]

    return get


def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@pytest.mark.parametrize("name", tt.QUERY_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_counts_lists_and_any_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    recs, ref = references(scene, name)
    counts = ref[0]
    # the set still does what it is there for, by the reference's own answers: a set that lost its finds must not pass vacuously
    if name == "random":
        assert (counts == 0).mean() >= 0.10 and (counts != 0).mean() >= 0.25 and min((counts > k).mean() for k in (1, 4, 8)) >= 0.01
    if name in ("self", "edge"):
        assert (counts >= 1).all() and (name != "self" or (counts > 8).mean() >= 0.5)
    if name in ("coplanar", "wall_touch", "degenerate", "far"):
        assert (counts != 0).mean() >= 0.25 and (counts == 0).mean() >= 0.10, (name, (counts != 0).mean())
    if name == "whole":
        assert (counts > 8).mean() >= 0.5 and counts.max() >= 100
    if name == "outside":
        assert not counts.any()
    before = pt.getBvhInfo(state).device_bytes
    _check_all(state, recs, ref, what=(scene, name))
    assert pt.getBvhInfo(state).device_bytes == before


def test_bad_triangles_between_good_ones(scenes, references):
    state, obj = scenes("box")
    recs, ref = references("box", "self")
    good = recs[:64]
    bad, why = tt.bad_triangles(good[0])
    assert bad.shape[0] < 32
    mixed = good.copy()
    where = 2 * np.arange(bad.shape[0]) + 1                 # every other lane of the first wave
    mixed[where] = bad
    still_good = np.ones(64, bool); still_good[where] = False
    d = _DeviceTris(state, mixed)
    try:
        p, c = d.triangles(8)
        hit = d.any()
    finally:
        d.free()
    wrong = (c[where] != 0) | (p[where] != 0xFFFFFFFF).any(axis=1) | (hit[where] != 0)
    assert not wrong.any(), [why[i] for i in np.flatnonzero(wrong)]
    assert np.array_equal(c[still_good], ref[0][:64][still_good]) and np.array_equal(p[still_good], ref[1][:64][still_good]) and (hit[still_good] == 1).all()
    _check_all(state, mixed, _reference(obj, mixed), sizes=(64,))
    # triangles that look odd and are triangles: junk in the reserved floats, a point on a vertex, a segment along an edge, the
    # largest finite coordinates
    v = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)[:, :3][np.asarray(obj.getIndexBuffer()[:3], np.int64)]
    odd = tt.as_records(np.array([v, [v[0]] * 3, [v[0], v[1], v[1]], [[-3e38, -3e38, -3e38], [3e38, 3e38, 3e38], [3e38, -3e38, 3e38]]], np.float32))
    odd[0, [3, 7, 11]] = (np.nan, np.inf, -7.0)
    assert tt.searchable(odd).all()
    ref_odd = _reference(obj, odd)
    assert (ref_odd[0][:3] >= 1).all()
    _check_all(state, odd, ref_odd, sizes=(4,))


def test_two_calls_give_the_same_bits_and_nothing_is_written_past_n(scenes, references):
    state, obj = scenes("diffuse")
    recs, ref = references("diffuse", "wall_touch")
    d = _DeviceTris(state, recs[:257])
    try:
        a, b = d.triangles(8), d.triangles(8)                  # triangles() checks the 0xCD guard behind each output
        h1, h2 = d.any(), d.any()
    finally:
        d.free()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(h1, h2)
    assert np.array_equal(a[0], ref[1][:257]) and np.array_equal(a[1], ref[0][:257]) and np.array_equal(h1, ref[2][:257])


def test_scene_memory_is_what_it_was(gpu_state_factory):
    """A default scene holds the fp16 nodes only, and the calls leave it so."""
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    before = pt.getBvhInfo(state).device_bytes
    recs = tt.query_set("random", obj.getVerticesFloat(), obj.getIndexBuffer())[:256]
    _check_all(state, recs, _reference(obj, recs), sizes=(256,))
    assert pt.getBvhInfo(state).device_bytes == before
    _host_closest(state, np.array([[0, 0, 0, 0, 0, 1, 0, 1]], np.float32))   # now the fp32 nodes come
    assert pt.getBvhInfo(state).device_bytes > before


def test_queries_leave_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    recs = tt.query_set("random", obj.getVerticesFloat(), obj.getIndexBuffer())
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        pt.queryTriangles(state, recs)
        pt.queryTrianglesAny(state, recs)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_after_a_refit_and_a_material_edit_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    recs = np.concatenate([tt.query_set(name, verts0, idx)[:400] for name in ("random", "self", "coplanar", "wall_touch")])
    old = _reference(obj, recs)
    _check_all(state, recs, old, sizes=(recs.shape[0],), ks=(8,))             # the queries have run on the scene before it changes
    # a material edit: the tree and the triangles stay, and so do the answers
    ids = (np.asarray(obj.getMaterialIndices(), np.uint32)[::-1]).copy()
    pt.updateMaterials(state, material_ids=ids)
    _check_all(state, recs, old, sizes=(recs.shape[0],), ks=(0, 8), what=("materials",))
    fresh = None
    try:
        # a refit: the tall block's and the short block's vertices (everything strictly inside the room) move
        verts = np.array(verts0, np.float32).reshape(-1, 4).copy()
        lo, hi = nr.scene_box(verts, idx)
        inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)
        assert 8 <= inner.sum() < verts.shape[0]
        verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
        info = pt.updateVertices(state, verts, "refit")
        assert not info["rebuilt"]
        moved = pt.TinyObjWrapper(BOX)
        moved._vertices = verts.reshape(-1).copy()
        fresh = _fresh_state(state, moved)
        ref = _reference(moved, recs)
        assert (ref[0] != old[0]).any()                        # the move shows in the answers
        _check_all(state, recs, ref, sizes=(recs.shape[0],), ks=(0, 8), what=("refitted",))
        _check_all(fresh, recs, ref, sizes=(recs.shape[0],), ks=(0, 8), what=("fresh",))
    finally:
        if fresh is not None:
            pt.CleanAllTheThings(fresh)


def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    recs, ref = references("box", "random")
    L = _L()
    d = _DeviceTris(state, recs[:256])
    try:
        expected = d.triangles(8)
        b, p, c, h = d.bufs
        ctx = state.context
        refused = {
            "null triangles": L.pt_query_triangles(ctx, None, 256, 8, p, c),
            "too many": L.pt_query_triangles(ctx, b, 0x80000000, 8, p, c),
            "prims and counts both null": L.pt_query_triangles(ctx, b, 256, 0, None, None),
            "prims null with max_prims != 0": L.pt_query_triangles(ctx, b, 256, 4, None, c),
            "prims with max_prims == 0": L.pt_query_triangles(ctx, b, 256, 0, p, c),
            "max_prims too large": L.pt_query_triangles(ctx, b, 256, 9, p, c),
            "triangles not aligned": L.pt_query_triangles(ctx, b + 4, 16, 8, p, c),
            "prims not aligned": L.pt_query_triangles(ctx, b, 16, 8, p + 8, c),
            "counts not aligned": L.pt_query_triangles(ctx, b, 16, 8, p, c + 2),
            "prims are the triangles": L.pt_query_triangles(ctx, b, 256, 8, b, c),
            "prims overlap the triangles' end": L.pt_query_triangles(ctx, b, 256, 8, b + 255 * 48, c),
            "counts lie inside the triangles": L.pt_query_triangles(ctx, b, 256, 8, p, b + 1024),
            "counts begin in the last triangle": L.pt_query_triangles(ctx, b, 256, 8, p, b + 256 * 48 - 16),
            "the triangles lie inside prims": L.pt_query_triangles(ctx, p + 1024, 64, 8, p, c),
            "counts lie inside prims": L.pt_query_triangles(ctx, b, 256, 8, p, p + 64),
            "prims lie inside counts": L.pt_query_triangles(ctx, b, 8, 4, c + 16, c),
            "null context": L.pt_query_triangles(None, b, 256, 8, p, c),
            "any: null triangles": L.pt_query_triangles_any(ctx, None, 256, h),
            "any: null hit": L.pt_query_triangles_any(ctx, b, 256, None),
            "any: too many": L.pt_query_triangles_any(ctx, b, 0x80000000, h),
            "any: triangles not aligned": L.pt_query_triangles_any(ctx, b + 8, 16, h),
            "any: hit is the triangles": L.pt_query_triangles_any(ctx, b, 256, b),
            "any: hit inside the triangles": L.pt_query_triangles_any(ctx, b, 256, b + 256 * 48 - 1),
            "any: null context": L.pt_query_triangles_any(None, b, 256, h),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_triangles(ctx, None, 256, 8, p, c) != 0 and _err(state).startswith("pt_query_triangles: ")
        assert L.pt_query_triangles(ctx, b, 0x80000000, 8, p, c) != 0 and "too many triangles" in _err(state)
        assert L.pt_query_triangles(ctx, b, 256, 8, b, c) != 0 and "overlaps the triangles" in _err(state)
        assert L.pt_query_triangles(ctx, b + 4, 16, 8, p, c) != 0 and "aligned" in _err(state)
        assert L.pt_query_triangles(ctx, b, 256, 9, p, c) != 0 and "max_prims" in _err(state)
        assert L.pt_query_triangles(ctx, b, 256, 0, None, None) != 0 and "nothing to write" in _err(state)
        assert L.pt_query_triangles_any(ctx, b, 256, None) != 0 and _err(state).startswith("pt_query_triangles_any: ")
        assert L.pt_query_triangles_any(ctx, b, 255, h + 1) == 0, _err(state)           # hit may have any alignment
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_triangles(bare, b, 256, 8, p, c) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_triangles_any(bare, b, 256, h) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_triangles(bare, None, 0, 8, None, None) == 0          # no triangles: nothing to do, nothing to refuse
            assert L.pt_query_triangles_any(bare, None, 0, None) == 0
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_triangles(ctx, None, 0, 0, None, None) == 0 and L.pt_query_triangles_any(ctx, None, 0, None) == 0
        again = d.triangles(8)                                                      # the next valid call
        assert np.array_equal(again[0], expected[0]) and np.array_equal(again[1], expected[1])
        assert np.array_equal(expected[0], ref[1][:256]) and np.array_equal(expected[1], ref[0][:256])
    finally:
        d.free()


def _visits(state, recs):
    """(counts, visits [n, 2]) of pt_debug_triangles_visits"""
    L = _L()
    n = recs.shape[0]
    d = _DeviceTris(state, recs)
    vis = pt.pathtracer._device_buffers(state, 1, n * 8)
    try:
        assert L.pt_debug_triangles_visits(state.context, d.bufs[0], n, d.bufs[2], vis[0]) == 0, _err(state)
        counts = np.zeros(n, np.uint32); visits = np.zeros((n, 2), np.uint32)
        assert L.pt_copy_to_host(state.context, counts.ctypes.data, d.bufs[2], counts.nbytes) == 0
        assert L.pt_copy_to_host(state.context, visits.ctypes.data, vis[0], visits.nbytes) == 0
        assert L.pt_debug_triangles_visits(state.context, d.bufs[0], n, d.bufs[2], None) != 0 and "null argument" in _err(state)
        assert L.pt_debug_triangles_visits(state.context, d.bufs[0], n, None, vis[0]) != 0 and "null argument" in _err(state)
        return counts, visits
    finally:
        pt.pathtracer._free_device_buffers(state, vis)
        d.free()


@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_visit_counts_of_the_test_hook(scenes, references, scene):
    """pt_debug_triangles_visits: the same counts, at least `count` and at most n_tris triangles tested, at most n_nodes nodes visited,
    a mean far below a brute force's — a walk that prunes nothing must not pass — and the root at most for a query whose box misses
    the scene box"""
    state, obj = scenes(scene)
    info = pt.getBvhInfo(state)
    n_tris = len(obj.getIndexBuffer()) // 3
    for name in ("random", "whole", "outside"):
        recs, ref = references(scene, name)
        counts, visits = _visits(state, recs)
        assert np.array_equal(counts, ref[0]), name
        assert (visits[:, 1] >= counts).all() and (visits[:, 1] <= n_tris).all() and (visits[:, 0] <= info.n_nodes).all() and (visits[:, 0] >= 1).all()
        print("%s %s: %.1f inner nodes and %.1f triangles per query (max %d / %d), %.1f intersect" % (scene, name, visits[:, 0].mean(), visits[:, 1].mean(), visits[:, 0].max(), visits[:, 1].max(), counts.mean()))
        if name == "random":
            assert visits[:, 1].mean() < n_tris / 4
        if name == "outside":
            assert (visits[:, 0] == 1).all() and not visits[:, 1].any()


def test_querytriangles_numpy_path(scenes, references):
    state, obj = scenes("diffuse")
    recs, ref = references("diffuse", "random")
    got = pt.queryTriangles(state, recs)
    assert got["prim"].dtype == np.uint32 and got["prim"].shape == (recs.shape[0], 8) and got["count"].dtype == np.uint32
    assert np.array_equal(got["prim"], ref[1]) and np.array_equal(got["count"], ref[0])
    tri = tt.vertices_of(recs)
    got = pt.queryTriangles(state, tri.tolist(), max_prims=3, counts=False)                             # anything np.asarray takes, (n, 3, 3)
    assert sorted(got) == ["prim"] and np.array_equal(got["prim"], ref[1][:, :3])
    got = pt.queryTriangles(state, tri.reshape(-1, 9), max_prims=0)                                     # (n, 9)
    assert got["prim"].shape == (recs.shape[0], 0) and np.array_equal(got["count"], ref[0])
    hit = pt.queryTrianglesAny(state, tri)
    assert hit.dtype == np.bool_ and np.array_equal(hit.view(np.uint8), ref[2])


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    recs, ref = references("box", "random")
    L = _L()
    seen = {}
    real, real_any = L.pt_query_triangles, L.pt_query_triangles_any
    monkeypatch.setattr(L, "pt_query_triangles", lambda ctx, b, n, k, p, c: seen.update(call=(b, n, k, p, c)) or real(ctx, b, n, k, p, c))
    monkeypatch.setattr(L, "pt_query_triangles_any", lambda ctx, b, n, h: seen.update(any=(b, n, h)) or real_any(ctx, b, n, h))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(recs.copy()).to(dev)
    got = pt.queryTriangles(state, x, max_prims=4)
    assert seen["call"][:3] == (x.data_ptr(), recs.shape[0], 4)
    assert seen["call"][3] == got["prim"].data_ptr() and seen["call"][4] == got["count"].data_ptr()      # the tensors the library wrote
    assert all(v.device == dev for v in got.values()) and got["prim"].dtype == torch.int32 and got["count"].dtype == torch.int32
    assert np.array_equal(got["prim"].cpu().numpy().view(np.uint32), ref[1][:, :4]) and np.array_equal(got["count"].cpu().numpy().view(np.uint32), ref[0])
    assert (got["prim"].cpu().numpy()[ref[1][:, :4] == 0xFFFFFFFF] == -1).all()
    only = pt.queryTriangles(state, x, max_prims=0)
    assert seen["call"][3] is None and only["prim"].shape == (recs.shape[0], 0) and torch.equal(only["count"], got["count"])
    assert sorted(pt.queryTriangles(state, x, counts=False)) == ["prim"] and seen["call"][4] is None
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    hit = pt.queryTrianglesAny(state, y)
    assert seen["any"][0] == y.data_ptr() and seen["any"][2] == hit.data_ptr() and hit.dtype == torch.bool and hit.device == dev
    assert np.array_equal(hit.cpu().numpy().view(np.uint8), ref[2])
    for fn in (pt.queryTriangles, pt.queryTrianglesAny):
        for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :9].contiguous(), "expected an")):
            with pytest.raises(pt.PathTracerError, match=what):
                fn(state, bad)
    assert pt.queryTriangles(state, x[:0])["prim"].shape == (0, 8) and pt.queryTrianglesAny(state, x[:0]).shape == (0,)


def _link_mesh():
    """A robot link of twelve triangles: a box 60 x 40 x 160, and eight poses of it in and around the Cornell room — through the tall
    block, in free air, through the floor, outside the room"""
    c = np.array([[x, y, z] for x in (-30, 30) for y in (-20, 20) for z in (-80, 80)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.uint32)
    poses = []
    for k, (t, deg) in enumerate([((368, 165, 351), 0), ((278, 400, 100), 30), ((100, 10, 100), 75), ((1500, 100, 100), 10),
                                  ((185, 82, 169), 45), ((278, 274, 280), 60), ((278, 548, 280), 20), ((-300, 274, 280), 0)]):
        a = np.deg2rad(deg)
        r = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) if k % 2 else np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        poses.append(np.concatenate([r, np.array(t, np.float64)[:, None]], axis=1))
    return c, idx, np.array(poses, np.float32)


def test_mesh_collisions_agree_with_the_reference(scenes):
    state, obj = scenes("box")
    verts, idx, poses = _link_mesh()
    P, T = poses.shape[0], idx.shape[0]
    recs = np.concatenate([pt.triangleRecords(verts, idx, p) for p in poses])
    ref = _reference(obj, recs)
    want = ref[2].reshape(P, T).any(axis=1)
    assert want.sum() >= 3 and (~want).sum() >= 3
    got = pt.meshCollisions(state, verts, idx, poses)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert pt.meshCollisions(state, verts, idx).shape == (1,)                                  # the mesh as it is: one pose
    pairs = pt.meshCollisions(state, verts, idx, poses, pairs=True)
    assert np.array_equal(pairs["counts"], ref[0].reshape(P, T))
    rows, cols = np.nonzero(ref[1] != 0xFFFFFFFF)
    assert np.array_equal(pairs["pairs"], np.stack([rows // T, rows % T, ref[1][rows, cols].astype(np.int64)], axis=1)) and rows.size >= 20
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        tv, ti, tp = torch.from_numpy(verts).to(dev), torch.from_numpy(idx.astype(np.int64)).to(dev), torch.from_numpy(poses).to(dev)
        trec = pt.triangleRecords(tv, ti, tp[1])
        assert trec.device == dev and trec.shape == (T, 12) and np.abs(trec.cpu().numpy() - recs[T:2 * T]).max() <= 1e-3
        all_recs = torch.cat([pt.triangleRecords(tv, ti, p) for p in tp])
        tref = _reference(obj, all_recs.cpu().numpy())                     # held to the reference on the records torch made
        thit = pt.meshCollisions(state, tv, ti, tp)
        assert thit.device == dev and thit.dtype == torch.bool and np.array_equal(thit.cpu().numpy(), tref[2].reshape(P, T).any(axis=1))
        tpairs = pt.meshCollisions(state, tv, ti, tp, pairs=True)
        assert np.array_equal(tpairs["counts"].cpu().numpy().view(np.uint32), tref[0].reshape(P, T))
        rows, cols = np.nonzero(tref[1] != 0xFFFFFFFF)
        assert np.array_equal(tpairs["pairs"].cpu().numpy(), np.stack([rows // T, rows % T, tref[1][rows, cols].astype(np.int64)], axis=1))


def test_cli_intersect_prints_what_querytriangles_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (F(0.5) * (lo + hi)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    tris = np.array([[[c[0] - 300, c[1], c[2] - 300], [c[0] + 300, c[1] + 10, c[2]], [c[0], c[1] - 10, c[2] + 300]],       # across the room, through the blocks
                     [[lo[0], c[1], c[2]], [lo[0] - 50, c[1] + 20, c[2]], [lo[0] - 50, c[1], c[2] + 20]],                  # touching a wall's plane from outside
                     [[c[0], lo[1], c[2]], [c[0] + 40, lo[1], c[2]], [c[0], lo[1], c[2] + 40]],                            # coplanar with the floor
                     [[hi[0] + 100, c[1], c[2]], [hi[0] + 120, c[1], c[2]], [hi[0] + 100, c[1] + 20, c[2]]],               # outside
                     [[c[0] - 2000, c[1], c[2] - 2000], [c[0] + 2000, c[1] + 1, c[2]], [c[0], c[1] - 1, c[2] + 2000]]], np.float32)
    ks = [None, 3, 0, 8, 5]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for t, k in zip(tris, ks):
        cmd += ["--intersect", ",".join("%r" % float(a) for a in t.reshape(-1)) + ("" if k is None else ",%d" % k)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"intersect"')]
    assert len(lines) == len(ks)
    got = pt.queryTriangles(state, tris)
    assert got["count"][0] > 8 and got["count"][1] >= 1 and got["count"][2] >= 1 and got["count"][3] == 0 and got["count"][4] > 8
    for i, line in enumerate(lines):
        k = 8 if ks[i] is None else ks[i]
        assert np.array_equal(np.array(line["intersect"], np.float32), tris[i].reshape(-1))
        assert line["count"] == int(got["count"][i])
        want = [int(t) for t in got["prim"][i, :k] if t != 0xFFFFFFFF]
        assert line["triangles"] == want and len(want) == min(k, int(got["count"][i]))
    for arg in ("1,2,3,4,5,6,7,8", "1,2,nan,1,1,1,2,2,2", "1,2,3,1,1,inf,2,2,2", "1,2,3,1,1,1,2,2,2,9", "1,2,3,1,1,1,2,2,2,-1"):
        bad = subprocess.run([exe, "--obj", BOX, "--intersect", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--intersect" in bad.stderr, arg
