"""Triangle-to-mesh distance on the GPU: pt_query_triangle_distance against tests/tridist_ref.py's brute force (the whole record, bits)
on every scene, size, query set and radius, the queries that are a miss before any traversal, the ignored eighth and twelfth float,
the output's bounds, the scene's memory, scene edits, the render state, the refusals, the counting twin, queries without area beside
pt_query_segments and pt_query_nearest, torch tensors, meshClearance, acgpt_main --tri-distance and the kernels' registers."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import nearest_ref as nr
import tridist_ref as tr
from test_tridist_host import DIST_BOUND

F = np.float32
gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
GUARD = 64                                         # bytes of 0xCD kept behind the records
MISS = 0xFFFFFFFF


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


class _DeviceTriangles:
    """queries in a device buffer with room for the records and a guard behind them; the C ABI called as a C caller would"""
    def __init__(self, state, records):
        self.state, self.n = state, records.shape[0]
        self.records = np.ascontiguousarray(records, np.float32)
        assert self.records.shape == (self.n, 12)
        self.bufs = pt.pathtracer._device_buffers(state, 2, max(self.n * 48, 48) + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.records.ctypes.data, self.records.nbytes) == 0

    def _read(self):
        raw = np.zeros(self.n * 12 + GUARD // 4, np.uint32)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, self.bufs[1], raw.nbytes) == 0
        assert (raw[self.n * 12:] == 0xCDCDCDCD).all(), "written past record %d" % self.n
        return raw[:self.n * 12].reshape(self.n, 12)

    def query(self):
        L, s = _L(), self.state
        assert L.pt_device_memset(s.context, self.bufs[1], 0xCD, self.n * 48 + GUARD) == 0
        assert L.pt_query_triangle_distance(s.context, self.bufs[0], self.n, self.bufs[1]) == 0, _err(s)
        return self._read()

    def visits(self, flags=0):
        """(records, counts [n, 2]) of the counting twin"""
        L, s = _L(), self.state
        vis = pt.pathtracer._device_buffers(s, 1, self.n * 8 + GUARD)
        try:
            assert L.pt_device_memset(s.context, self.bufs[1], 0xCD, self.n * 48 + GUARD) == 0
            assert L.pt_device_memset(s.context, vis[0], 0xCD, self.n * 8 + GUARD) == 0
            assert L.pt_debug_triangle_distance_visits(s.context, self.bufs[0], self.n, self.bufs[1], vis[0], flags) == 0, _err(s)
            raw = np.zeros(self.n * 2 + GUARD // 4, np.uint32)
            assert L.pt_copy_to_host(s.context, raw.ctypes.data, vis[0], raw.nbytes) == 0
            assert (raw[self.n * 2:] == 0xCDCDCDCD).all(), "written past the visit counts"
            return self._read(), raw[:self.n * 2].reshape(self.n, 2)
        finally:
            pt.pathtracer._free_device_buffers(s, vis)

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _query(state, records):
    d = _DeviceTriangles(state, records)
    try:
        return d.query()
    finally:
        d.free()


def _reference(obj, records, **kw):
    return tr.triangle_distance_records(records, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), **kw)


def _diff(rec, ref):
    bad = np.flatnonzero((rec != ref).any(axis=1))
    return (bad.size, bad[:4], rec[bad][:2], rec[bad][:2].view(np.float32), ref[bad][:2], ref[bad][:2].view(np.float32))


def _fresh_state(like, obj, tuning=None):
    """A context of its own with like's parameters and obj's scene; tuning: pt_set_tuning's variant, set before the build"""
    state = pt.PathTracerState()
    C.memmove(C.byref(state.params), C.byref(like.params), C.sizeof(state.params))
    state.params.accumulationBuffer = None
    pt.createDeviceContext(state)
    if tuning is not None:
        assert _L().pt_set_tuning(state.context, 0, tuning) == 0
    pt.buildTheAccelarationStructure(state, obj)
    return state


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
    """(scene, set) -> (triangles [n, 9], radius, records at +inf, records at the radius) by the brute force on the whole set: computed
    once, shared, never written.  The fp32-node scene is the box: it shares the box's."""
    cache = {}

    def get(scene, name):
        key = ("box" if scene == "fp32" else scene, name)
        if key not in cache:
            state, obj = scenes(key[0])
            verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
            tris = tr.query_set(name, verts, idx)
            radius = tr.set_radius(name, verts, idx)
            rec_inf, d2 = _reference(obj, tr.as_records(tris, np.inf), return_d2=True)
            out = (tris, radius, rec_inf, tr.records_within(rec_inf, d2, radius))
            for a in (out[0], out[2], out[3]):
                a.setflags(write=False)
            cache[key] = out
        return cache[key]

    return get


@gpu
def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@gpu
@pytest.mark.parametrize("name", tr.QUERY_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_records_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    tris, radius, ref_inf, ref_r = references(scene, name)
    # the set still does what it is there for, by the reference's own answers: a set that lost its finds must not pass vacuously
    found = ref_r[:, 1] != MISS
    assert found.mean() >= 0.25 and (~found).mean() >= 0.10, (name, found.mean())
    assert np.unique(ref_r[found, 1]).size >= 8 and (ref_inf[:, 1] != MISS).all()
    if name in ("large", "touching"):
        groups = np.bincount(tr.group_of(ref_inf.view(np.float32)[:, 2]), minlength=5) / ref_inf.shape[0]
        assert groups[3] >= 0.05 and groups[4] >= 0.05, groups
    before = pt.getBvhInfo(state).device_bytes
    for r, ref in ((np.inf, ref_inf), (radius, ref_r)):
        g = tr.as_records(tris, r)
        for n in SIZES:
            rec = _query(state, g[:n])
            assert np.array_equal(rec, ref[:n]), (scene, name, float(r), n) + _diff(rec, ref[:n])
    assert pt.getBvhInfo(state).device_bytes == before


@gpu
def test_bad_triangles_between_good_ones(scenes, references):
    state, obj = scenes("box")
    tris, radius, ref_inf, ref_r = references("box", "large")
    good = tr.as_records(tris[:64], np.inf)
    bad, why = tr.bad_triangles(good[0])
    assert bad.shape[0] < 32
    mixed = good.copy()
    where = 2 * np.arange(bad.shape[0]) + 1                 # every other lane of the first wave
    mixed[where] = bad
    still_good = np.ones(64, bool); still_good[where] = False
    rec = _query(state, mixed)
    wrong = (rec[where] != tr.miss_records(where.size)).any(axis=1)
    assert not wrong.any(), [why[i] for i in np.flatnonzero(wrong)]
    assert np.array_equal(rec[still_good], ref_inf[:64][still_good])
    assert np.array_equal(rec, _reference(obj, mixed))
    # queries that look odd and are queries: a radius of +-0 on a touching triangle and beside it, a huge radius whose square overflows
    v = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)[obj.getIndexBuffer()[0], :3]
    t0 = [v[0], v[1], v[2], v[0] + 7.0, v[1] + 3.0, v[2] + 5.0, v[0] - 2.0, v[1] + 6.0, v[2] + 1.0]
    t1 = [v[0] + 1.0, v[1] + 1.0, v[2] + 1.0, v[0] + 2.0, v[1] + 1.5, v[2] + 1.0, v[0] + 1.0, v[1] + 2.0, v[2] + 3.0]
    odd = np.concatenate([tr.as_records([t0], 0.0), tr.as_records([t0], -0.0), tr.as_records([t1], 0.0), tr.as_records([t0], 1e30)])
    assert tr.searchable(odd).all()
    rec, ref = _query(state, odd), _reference(obj, odd)
    assert np.array_equal(rec, ref), _diff(rec, ref)
    assert rec[0, 1] != MISS and rec[0, 0] == 0 and rec[1, 1] == rec[0, 1] and rec[3, 1] == rec[0, 1]


@gpu
def test_the_eighth_and_twelfth_float_are_ignored(scenes, references):
    state, obj = scenes("diffuse")
    tris, radius, ref_inf, ref_r = references("diffuse", "offset")
    g = tr.as_records(tris[:257], radius)
    for k, val in enumerate((np.nan, np.inf, -np.inf, -1.0, 3e38)):
        g[k::5, 7] = val
        g[(k + 2)::5, 11] = val
    rec = _query(state, g)
    assert np.array_equal(rec, ref_r[:257]), _diff(rec, ref_r[:257])
    g[:, 7] = np.nan
    g[:, 11] = np.nan
    assert np.array_equal(_query(state, g), ref_r[:257])


@gpu
def test_two_calls_give_the_same_bits_and_nothing_is_written_past_n(scenes, references):
    state, obj = scenes("diffuse")
    tris, radius, ref_inf, ref_r = references("diffuse", "touching")
    d = _DeviceTriangles(state, tr.as_records(tris[:257], np.inf))
    try:
        a, b = d.query().copy(), d.query().copy()          # query() checks the 0xCD guard behind record n
    finally:
        d.free()
    assert np.array_equal(a, b) and np.array_equal(a, ref_inf[:257])
    assert not a[:, 7].any() and not a[:, 11].any()        # the pad words are written, as 0


@gpu
def test_scene_memory_is_what_it_was(gpu_state_factory):
    """A default scene holds the fp16 nodes only, and the call leaves it so."""
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    before = pt.getBvhInfo(state).device_bytes
    g = tr.as_records(tr.query_set("small", obj.getVerticesFloat(), obj.getIndexBuffer())[:256], np.inf)
    rec = _query(state, g)
    assert pt.getBvhInfo(state).device_bytes == before
    assert np.array_equal(rec, _reference(obj, g))
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@gpu
def test_queries_leave_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    tris = tr.query_set("large", obj.getVerticesFloat(), obj.getIndexBuffer())
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        _query(state, tr.as_records(tris, np.inf))
        pt.queryTriangleDistance(state, tris, 50.0)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


@gpu
def test_after_scene_edits_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    tris = np.concatenate([tr.query_set(name, verts0, idx)[:200] for name in ("small", "large", "touching")])
    g = np.concatenate([tr.as_records(tris, np.inf), tr.as_records(tris, tr.set_radius("small", verts0, idx))])
    _query(state, g)                                         # the queries have run on the scene before it changes
    fresh = []
    try:
        # 1. a refit: the tall block's and the short block's vertices (everything strictly inside the room) move
        verts = np.array(verts0, np.float32).reshape(-1, 4).copy()
        lo, hi = nr.scene_box(verts, idx)
        inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)
        assert 8 <= inner.sum() < verts.shape[0]
        verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
        info = pt.updateVertices(state, verts, "refit")
        assert not info["rebuilt"]
        moved = pt.TinyObjWrapper(BOX)
        moved._vertices = verts.reshape(-1).copy()
        fresh.append(_fresh_state(state, moved))
        rec, rec2 = _query(state, g), _query(fresh[-1], g)
        ref = _reference(moved, g)
        assert np.array_equal(rec, rec2), _diff(rec, rec2)
        assert np.array_equal(rec, ref), _diff(rec, ref)
        assert (ref != _reference(obj, g)).any()              # the move shows in the answers
        # 2. new material assignments on top: the ids rotate by one
        n_mats = obj.getNumMaterials()
        ids = ((np.asarray(obj.getMaterialIndices(), np.uint32) + 1) % n_mats).astype(np.uint32)
        pt.updateMaterials(state, material_ids=ids)
        moved._materialIndices = ids
        fresh.append(_fresh_state(state, moved))
        rec3, rec4 = _query(state, g), _query(fresh[-1], g)
        found = rec[:, 1] != MISS
        want = ref.copy()
        want[found, 3] = ids[ref[found, 1]]
        assert np.array_equal(rec3, rec4) and np.array_equal(rec3, want)
        keep = [0, 1, 2] + list(range(4, 12))
        assert np.array_equal(rec3[:, keep], rec[:, keep]) and (rec3[:, 3] != rec[:, 3])[found].all() and found.mean() >= 0.25
    finally:
        for s in fresh:
            pt.CleanAllTheThings(s)


@gpu
def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    tris, radius, ref_inf, ref_r = references("box", "small")
    L = _L()
    d = _DeviceTriangles(state, tr.as_records(tris[:256], np.inf))
    try:
        expected = d.query().copy()
        p, o = d.bufs
        fn = L.pt_query_triangle_distance
        refused = {
            "null triangles": fn(state.context, None, 256, o),
            "null output": fn(state.context, p, 256, None),
            "too many": fn(state.context, p, 0x80000000, o),
            "the output is the triangles": fn(state.context, p, 256, p),
            "the output overlaps the triangles' end": fn(state.context, p, 256, p + 255 * 48),
            "the triangles lie inside the output": fn(state.context, o + 1024, 64, o),
            "triangles not aligned": fn(state.context, p + 4, 16, o),
            "output not aligned": fn(state.context, p, 16, o + 8),
            "null context": fn(None, p, 256, o),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert fn(None, p, 256, o) != 0 and L.pt_last_error(None).decode().startswith("pt_query_triangle_distance: ") and b"null context" in L.pt_last_error(None)
        assert fn(state.context, None, 256, o) != 0 and _err(state).startswith("pt_query_triangle_distance: ") and "null argument" in _err(state)
        assert fn(state.context, p, 0x80000000, o) != 0 and "too many triangles" in _err(state)
        assert fn(state.context, p, 256, p) != 0 and "overlaps" in _err(state)
        assert fn(state.context, p + 4, 16, o) != 0 and "aligned" in _err(state)
        # the order: a null pointer before the count, the count before the alignment, the alignment before the overlap
        assert fn(state.context, None, 0x80000000, o) != 0 and "null argument" in _err(state)
        assert fn(state.context, p + 4, 0x80000000, o) != 0 and "too many triangles" in _err(state)
        assert fn(state.context, p + 4, 16, p + 4) != 0 and "aligned" in _err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert fn(bare, p, 256, o) != 0 and b"no scene" in L.pt_last_error(bare) and L.pt_last_error(bare).startswith(b"pt_query_triangle_distance: ")
            assert fn(bare, p, 256, p) != 0 and b"overlaps" in L.pt_last_error(bare)      # the overlap before the missing scene
            assert fn(bare, None, 0, None) == 0                                         # no queries: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert fn(state.context, None, 0, None) == 0
        assert np.array_equal(d.query(), expected)                             # the next valid call
        assert np.array_equal(expected, ref_inf[:256])
    finally:
        d.free()


@gpu
@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_visit_counts_of_the_test_hook(scenes, references, scene):
    """pt_debug_triangle_distance_visits: the same records, with the second bound and without it, and counts that make sense — no query
    visits more nodes or tests more triangles than the scene has, every searchable one tests at least one, a miss before any traversal
    none; on the large set the second bound saves visits."""
    state, obj = scenes(scene)
    info = pt.getBvhInfo(state)
    n_tris = len(obj.getIndexBuffer()) // 3
    L = _L()
    for name, r in (("large", np.inf), ("touching", 0.0), ("shell", None)):
        tris, radius, ref_inf, ref_r = references(scene, name)
        n = 257
        g = tr.as_records(tris[:n], radius if r is None else r)
        g[5, 0] = np.nan                                   # one miss before any traversal
        want = np.array(ref_inf[:n] if r is not None and np.isinf(r) else (ref_r[:n] if r is None else _reference(obj, g)))
        want[5] = tr.miss_records(1)[0]
        d = _DeviceTriangles(state, g)
        try:
            rec, counts = d.visits(0)
            rec_off, counts_off = d.visits(1)
            assert np.array_equal(rec, want), (name,) + _diff(rec, want)
            assert np.array_equal(rec_off, want), (name,) + _diff(rec_off, want)
            ok = tr.searchable(g)
            assert not ok[5] and not counts[~ok].any() and not counts_off[~ok].any()
            for c in (counts, counts_off):
                assert (c[ok, 0] >= 1).all() and (c[:, 0] <= info.n_nodes).all() and (c[:, 1] <= n_tris).all()
                assert (c[ok & (want[:, 1] != MISS), 1] >= 1).all()
            print("%s %s: nodes %.1f / %.1f, triangles %.1f / %.1f per query with / without bound (b)" % (
                scene, name, counts[:, 0].mean(), counts_off[:, 0].mean(), counts[:, 1].mean(), counts_off[:, 1].mean()))
            if r is not None and np.isinf(r):
                assert (counts[ok, 1] >= 1).all()
                assert counts[:, 1].mean() < n_tris / 4           # the boxes prune: far from a brute force
            if name == "large":           # what the second bound is for: a large diagonal triangle no longer enters every box of its own box
                assert counts[:, 0].sum() < counts_off[:, 0].sum()
            assert L.pt_debug_triangle_distance_visits(state.context, d.bufs[0], n, d.bufs[1], None, 0) != 0 and "null argument" in _err(state)
            assert L.pt_debug_triangle_distance_visits(state.context, d.bufs[0], n, d.bufs[1], d.bufs[1], 2) != 0 and "flags" in _err(state)
        finally:
            d.free()


@gpu
def test_queries_without_area_beside_the_segment_and_the_closest_point_query(scenes, references):
    """a2 == a1 is a segment and three equal vertices are a point.  The triangle statement holds every sub-test of the segment's (and the
    point's) and more — the scene's vertices against the degenerate face may give a NaN or another rounding of the same point —, so
    its distance is never above theirs, and within the host test's fp32 bar of it: the bar was measured on coordinates up to 10 and
    errors grow with the coordinates, so it is taken times S / 10."""
    import segment_ref as sr
    state, obj = scenes("box")
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    lo, hi = nr.scene_box(verts, idx)
    scale = float(np.abs(np.concatenate([lo, hi])).max())
    bar = DIST_BOUND * scale / 10.0
    segs = np.concatenate([sr.segment_set(name, verts, idx)[:300] for name in ("short", "long", "touching")])
    seg = pt.querySegments(state, segs)
    got = pt.queryTriangleDistance(state, np.concatenate([segs, segs[:, 3:6]], axis=1))
    assert (got["prim"] != MISS).all() and (seg["prim"] != MISS).all()
    assert (got["distance"] <= seg["distance"]).all()
    worst = np.abs(got["distance"].astype(np.float64) - seg["distance"]).max()
    print("largest |triangle - segment| distance on %d segments: %.3e (bar %.3e)" % (segs.shape[0], worst, bar))
    assert worst <= bar
    assert (seg["distance"] == 0).mean() >= 0.1
    pts = np.concatenate([nr.point_set("inside", verts, idx, None)[:512], nr.feature_points(verts, idx)[::17][:512]])
    near = pt.queryNearest(state, pts)
    got = pt.queryTriangleDistance(state, np.concatenate([pts, pts, pts], axis=1))
    assert (got["prim"] != MISS).all() and (got["distance"] <= near["distance"]).all()
    worst = np.abs(got["distance"].astype(np.float64) - near["distance"]).max()
    print("largest |triangle - nearest| distance on %d points: %.3e (bar %.3e)" % (pts.shape[0], worst, bar))
    assert worst <= bar
    assert (got["feature"] < 15).all() and (got["feature"] == 0.0).mean() >= 0.5
    same = got["feature"] == 0.0
    assert np.array_equal(got["distance"][same].view(np.uint32), near["distance"][same].view(np.uint32))
    assert np.array_equal(got["on_query"][same], pts[same])


def _packed(got):
    n = got["distance"].shape[0]
    zero = np.zeros((n, 1), np.uint32)
    return np.concatenate([got["distance"].view(np.uint32)[:, None], got["prim"][:, None], got["feature"].view(np.uint32)[:, None], got["material"][:, None],
                           got["on_query"].view(np.uint32), zero, got["point"].view(np.uint32), zero], axis=1)


@gpu
def test_querytriangledistance_numpy_path(scenes, references):
    state, obj = scenes("diffuse")
    tris, radius, ref_inf, ref_r = references("diffuse", "large")
    got = pt.queryTriangleDistance(state, tris, float(radius))
    assert got["distance"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32 and got["feature"].dtype == np.float32
    assert got["point"].shape == (tris.shape[0], 3) and got["on_query"].shape == (tris.shape[0], 3)
    assert np.array_equal(_packed(got), ref_r)
    assert np.array_equal(_packed(pt.queryTriangleDistance(state, tris.reshape(-1, 3, 3))), ref_inf)          # (n, 3, 3), no radius
    got = pt.queryTriangleDistance(state, tr.as_records(tris, radius).tolist(), 0.0)      # anything np.asarray takes; records carry their own radius
    assert np.array_equal(_packed(got), ref_r)


@gpu
def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    tris, radius, ref_inf, ref_r = references("box", "large")
    g = tr.as_records(tris, radius)
    L = _L()
    seen = {}
    real = L.pt_query_triangle_distance
    monkeypatch.setattr(L, "pt_query_triangle_distance", lambda ctx, p, n, out: seen.update(call=(p, n, out)) or real(ctx, p, n, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(g.copy()).to(dev)
    got = pt.queryTriangleDistance(state, x)
    assert seen["call"][0] == x.data_ptr() and seen["call"][1] == g.shape[0]
    assert all(v.device == dev for v in got.values())
    assert seen["call"][2] == got["distance"].data_ptr()                   # the columns are views of the tensor the library wrote
    assert got["distance"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32
    assert got["point"].shape == (g.shape[0], 3) and got["on_query"].shape == (g.shape[0], 3)
    cols = {"distance": ref_r[:, 0], "prim": ref_r[:, 1], "feature": ref_r[:, 2], "material": ref_r[:, 3]}
    for k, want in cols.items():
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), k
    assert np.array_equal(got["on_query"].cpu().numpy().view(np.uint32), ref_r[:, 4:7])
    assert np.array_equal(got["point"].cpu().numpy().view(np.uint32), ref_r[:, 8:11])
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.queryTriangleDistance(state, y)
    assert seen["call"][0] == y.data_ptr() and torch.equal(again["prim"], got["prim"]) and torch.equal(again["distance"], got["distance"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :9].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.queryTriangleDistance(state, bad)
    assert pt.queryTriangleDistance(state, x[:0])["distance"].shape == (0,)


def _tetrahedron(size):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) * F(size)
    return v, np.array([0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3], np.uint32)


@gpu
def test_mesh_clearance(scenes):
    """P poses of a tetrahedron: each pose's closest pair is the reduction of the reference's records over the pose's triangles, ties to
    the lowest mesh triangle; the tensor path says the same."""
    state, obj = scenes("box")
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    lo, hi = nr.scene_box(verts, idx)
    v, tri = _tetrahedron(40.0)
    rng = np.random.default_rng(77)
    P = 48
    poses = np.zeros((P, 3, 4), np.float32)
    for k in range(P):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        poses[k, :, :3] = q
    poses[:, :, 3] = lo + rng.random((P, 3)).astype(np.float32) * (hi - lo)
    poses[-4:, :, 3] += 3.0 * (hi - lo)                      # four poses far outside
    radius = F(0.08) * F(np.linalg.norm(hi - lo))
    for r in (np.inf, radius):
        got = pt.meshClearance(state, v, tri, poses, max_radius=float(r))
        rec = pt.pathtracer._posed_records("test", v, tri, poses)
        assert np.array_equal(rec[5], pt.triangleRecords(v, tri, poses[5]))
        rec[:, :, 3] = r
        ref = _reference(obj, rec.reshape(-1, 12)).reshape(P, 4, 12)
        dist = ref.view(np.float32)[:, :, 0]
        d = np.where(ref[:, :, 1] != MISS, dist, np.inf)
        win = d.argmin(axis=1)
        rows = np.arange(P)
        found = np.isfinite(d[rows, win])
        assert np.array_equal(got["clearance"], d[rows, win].astype(np.float32))
        assert np.array_equal(got["query_triangle"], np.where(found, win, -1))
        assert np.array_equal(got["prim"], ref[rows, win, 1])
        assert np.array_equal(got["on_query"].view(np.uint32), ref[rows, win, 4:7]) and np.array_equal(got["on_mesh"].view(np.uint32), ref[rows, win, 8:11])
        if np.isinf(r):
            assert found.all() and (got["clearance"] == 0).sum() >= 4 and (got["clearance"] > 0).sum() >= 8
        else:
            assert (~found).sum() >= 4 and found.sum() >= 8 and np.isinf(got["clearance"][~found]).all() and (got["prim"][~found] == MISS).all()
    one = pt.meshClearance(state, v, tri, poses[3], max_radius=float(radius))                 # one matrix is one pose
    assert one["clearance"].shape == (1,) and np.array_equal(one["clearance"], got["clearance"][3:4]) and np.array_equal(one["prim"], got["prim"][3:4])
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        want = pt.meshClearance(state, v, tri, poses, max_radius=float(radius))
        t = pt.meshClearance(state, torch.from_numpy(v).to(dev), torch.from_numpy(tri.astype(np.int64)).to(dev), torch.from_numpy(poses).to(dev), max_radius=float(radius))
        assert all(x.device == dev for x in t.values())
        # torch forms the posed vertices with its own matmul: the same poses, another rounding — the pairs agree where the clearance is not a near tie
        assert np.array_equal(np.isinf(t["clearance"].cpu().numpy()), np.isinf(want["clearance"]))
        assert np.allclose(t["clearance"].cpu().numpy(), want["clearance"], rtol=0, atol=1e-2)
        assert (t["query_triangle"].cpu().numpy() == want["query_triangle"]).mean() >= 0.9


@gpu
def test_cli_tri_distance_prints_what_querytriangledistance_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (F(0.5) * (lo + hi)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    queries = [(c[0], c[1], c[2], c[0] + F(20.0), c[1] + F(5.0), c[2] - F(10.0), c[0] - F(4.0), c[1] + F(9.0), c[2] + F(2.0), None),
               (c[0], hi[1] - F(50.0), c[2], c[0] + F(3.0), hi[1] + F(50.0), c[2] + F(2.0), c[0] + F(30.0), hi[1] - F(20.0), c[2] - F(9.0), F(4.5)),     # through the ceiling
               (lo[0] - F(60.0), c[1] - F(80.0), c[2] - F(70.0), lo[0] - F(60.0), c[1] + F(90.0), c[2] - F(60.0), lo[0] - F(60.0), c[1], c[2] + F(95.0), F(100.0)),
               (hi[0] + F(100.0), hi[1] + F(50.0), hi[2], hi[0] + F(130.0), hi[1], hi[2], hi[0] + F(110.0), hi[1], hi[2] + F(15.0), F(0.0))]      # nothing within 0
    queries = [tuple(None if a is None else float(np.float32(a)) for a in q) for q in queries]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for q in queries:
        cmd += ["--tri-distance", ",".join("%r" % a for a in q if a is not None)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"tri_distance"')]
    assert len(lines) == len(queries)
    rec = tr.as_records(np.array([q[:9] for q in queries], np.float32))
    rec[:, 3] = [np.inf if q[9] is None else q[9] for q in queries]
    got = pt.queryTriangleDistance(state, rec)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    assert (got["prim"][:3] != MISS).all() and got["prim"][3] == MISS and got["distance"][1] == 0 and got["feature"][1] >= 15 and got["distance"][2] > 0
    for i, line in enumerate(lines):
        assert np.array_equal(np.array(line["tri_distance"], np.float32), np.array(queries[i][:9], np.float32))
        found = got["prim"][i] != MISS
        assert line["found"] is bool(found)
        assert (line["radius"] is None) == (queries[i][9] is None) and (line["radius"] is None or np.float32(line["radius"]) == rec[i, 3])
        if not found:
            continue
        assert line["triangle"] == int(got["prim"][i]) and np.float32(line["distance"]) == got["distance"][i]
        assert line["material"] == names[int(got["material"][i])] and line["feature"] == int(got["feature"][i])
        assert np.array_equal(np.array(line["on_query"], np.float32), got["on_query"][i])
        assert np.array_equal(np.array(line["point"], np.float32), got["point"][i])
    for arg in ("1,2,3,4,5,6,7,8", "1,2,nan,4,5,6,7,8,9", "1,2,3,4,5,inf,7,8,9", "1,2,3,4,5,6,7,8,9,-1", "1,2,3,4,5,6,7,8,9,nan", "1,2,3,4,5,6,7,8,9,10,11", "1,2,3,4,5,6,7,8,x"):
        bad = subprocess.run([exe, "--obj", BOX, "--tri-distance", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--tri-distance" in bad.stderr, arg


def test_triangle_distance_kernels_keep_their_register_budget(built):
    """Read from the built code object (no GPU): the four k_query_triangle_distance instantiations (two node formats, each with its
    counting twin) use no scratch memory, spill nothing and stay within 128 vector registers — four waves per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_query_triangle_distance<" in k["name"]]
    assert len(rows) == 4, [k["name"] for k in rows]
    for k in rows:
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 128, k
        assert k["sgpr_spill_count"] == 0, k
