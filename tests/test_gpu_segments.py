"""Segment-to-mesh distance on the GPU: pt_query_segments against tests/segment_ref.py's brute force (the whole record, bits) on every
scene, size, segment set and radius, the segments that are a miss before any traversal, the ignored eighth float, the output's
bounds, the scene's memory, scene edits, the render state, the refusals, the counting twin, zero-length segments beside
pt_query_nearest, torch tensors, capsuleClearance and acgpt_main --clearance."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import nearest_ref as nr
import segment_ref as sr
from test_segment_host import DIST_BOUND

F = np.float32
pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
GUARD = 64                                         # bytes of 0xCD kept behind the records


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


class _DeviceSegments:
    """segments in a device buffer with room for the records and a guard behind them; the C ABI called as a C caller would"""
    def __init__(self, state, segments):
        self.state, self.n = state, segments.shape[0]
        self.segments = np.ascontiguousarray(segments, np.float32)
        assert self.segments.shape == (self.n, 8)
        self.bufs = pt.pathtracer._device_buffers(state, 2, max(self.n * 32, 32) + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.segments.ctypes.data, self.segments.nbytes) == 0

    def _read(self):
        raw = np.zeros(self.n * 8 + GUARD // 4, np.uint32)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, self.bufs[1], raw.nbytes) == 0
        assert (raw[self.n * 8:] == 0xCDCDCDCD).all(), "written past record %d" % self.n
        return raw[:self.n * 8].reshape(self.n, 8)

    def query(self):
        L, s = _L(), self.state
        assert L.pt_device_memset(s.context, self.bufs[1], 0xCD, self.n * 32 + GUARD) == 0
        assert L.pt_query_segments(s.context, self.bufs[0], self.n, self.bufs[1]) == 0, _err(s)
        return self._read()

    def visits(self, flags=0):
        """(records, counts [n, 2]) of the counting twin"""
        L, s = _L(), self.state
        vis = pt.pathtracer._device_buffers(s, 1, self.n * 8 + GUARD)
        try:
            assert L.pt_device_memset(s.context, self.bufs[1], 0xCD, self.n * 32 + GUARD) == 0
            assert L.pt_device_memset(s.context, vis[0], 0xCD, self.n * 8 + GUARD) == 0
            assert L.pt_debug_segments_visits(s.context, self.bufs[0], self.n, self.bufs[1], vis[0], flags) == 0, _err(s)
            raw = np.zeros(self.n * 2 + GUARD // 4, np.uint32)
            assert L.pt_copy_to_host(s.context, raw.ctypes.data, vis[0], raw.nbytes) == 0
            assert (raw[self.n * 2:] == 0xCDCDCDCD).all(), "written past the visit counts"
            return self._read(), raw[:self.n * 2].reshape(self.n, 2)
        finally:
            pt.pathtracer._free_device_buffers(s, vis)

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _query(state, segments):
    d = _DeviceSegments(state, segments)
    try:
        return d.query()
    finally:
        d.free()


def _reference(obj, segments, **kw):
    return sr.segment_records(segments, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), **kw)


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
    """(scene, set) -> (segments, radius, records at +inf, records at the radius) by the brute force on the whole set: computed once,
    shared, never written.  The fp32-node scene is the box: it shares the box's."""
    cache = {}

    def get(scene, name):
        key = ("box" if scene == "fp32" else scene, name)
        if key not in cache:
            state, obj = scenes(key[0])
            verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
            segs = sr.segment_set(name, verts, idx)
            radius = sr.set_radius(name, verts, idx)
            rec_inf, d2 = _reference(obj, sr.with_radius(segs, np.inf), return_d2=True)
            out = (segs, radius, rec_inf, sr.records_within(rec_inf, d2, radius))
            for a in (out[0], out[2], out[3]):
                a.setflags(write=False)
            cache[key] = out
        return cache[key]

    return get


def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@pytest.mark.parametrize("name", sr.SEGMENT_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_records_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    segs, radius, ref_inf, ref_r = references(scene, name)
    # the set still does what it is there for, by the reference's own answers: a set that lost its finds must not pass vacuously
    found = ref_r[:, 1] != 0xFFFFFFFF
    assert found.mean() >= 0.25 and (~found).mean() >= 0.10, (name, found.mean())
    assert np.unique(ref_r[found, 1]).size >= 8 and (ref_inf[:, 1] != 0xFFFFFFFF).all()
    if name in ("long", "axis", "touching"):
        assert (ref_inf.view(np.float32)[:, 3] == 5).mean() >= 0.05
    before = pt.getBvhInfo(state).device_bytes
    for r, ref in ((np.inf, ref_inf), (radius, ref_r)):
        g = sr.with_radius(segs, r)
        for n in SIZES:
            rec = _query(state, g[:n])
            assert np.array_equal(rec, ref[:n]), (scene, name, float(r), n) + _diff(rec, ref[:n])
    assert pt.getBvhInfo(state).device_bytes == before


def test_bad_segments_between_good_ones(scenes, references):
    state, obj = scenes("box")
    segs, radius, ref_inf, ref_r = references("box", "long")
    good = sr.with_radius(segs[:64], np.inf)
    bad, why = sr.bad_segments(good[0])
    assert bad.shape[0] < 32
    mixed = good.copy()
    where = 2 * np.arange(bad.shape[0]) + 1                 # every other lane of the first wave
    mixed[where] = bad
    still_good = np.ones(64, bool); still_good[where] = False
    rec = _query(state, mixed)
    wrong = (rec[where] != sr.miss_records(where.size)).any(axis=1)
    assert not wrong.any(), [why[i] for i in np.flatnonzero(wrong)]
    assert np.array_equal(rec[still_good], ref_inf[:64][still_good])
    assert np.array_equal(rec, _reference(obj, mixed))
    # segments that look odd and are segments: a radius of +-0 on a touching segment and beside it, a huge radius whose square overflows
    v = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)[obj.getIndexBuffer()[0], :3]
    odd = np.array([[v[0], v[1], v[2], 0.0, v[0] + 7.0, v[1] + 3.0, v[2] + 5.0, 0.0], [v[0], v[1], v[2], -0.0, v[0] + 7.0, v[1] + 3.0, v[2] + 5.0, 0.0],
                    [v[0] + 1.0, v[1] + 1.0, v[2] + 1.0, 0.0, v[0] + 2.0, v[1] + 1.5, v[2] + 1.0, 0.0], [v[0], v[1], v[2], 1e30, v[0] + 7.0, v[1] + 3.0, v[2] + 5.0, 0.0]], np.float32)
    assert sr.searchable(odd).all()
    rec, ref = _query(state, odd), _reference(obj, odd)
    assert np.array_equal(rec, ref), _diff(rec, ref)
    assert rec[0, 1] != 0xFFFFFFFF and rec[0, 0] == 0 and rec[1, 1] == rec[0, 1] and rec[3, 1] == rec[0, 1]


def test_the_eighth_float_is_ignored(scenes, references):
    state, obj = scenes("diffuse")
    segs, radius, ref_inf, ref_r = references("diffuse", "axis")
    g = sr.with_radius(segs[:257], radius)
    for k, val in enumerate((np.nan, np.inf, -np.inf, -1.0, 3e38)):
        g[k::5, 7] = val
    rec = _query(state, g)
    assert np.array_equal(rec, ref_r[:257]), _diff(rec, ref_r[:257])
    g[:, 7] = np.nan
    assert np.array_equal(_query(state, g), ref_r[:257])


def test_two_calls_give_the_same_bits_and_nothing_is_written_past_n(scenes, references):
    state, obj = scenes("diffuse")
    segs, radius, ref_inf, ref_r = references("diffuse", "touching")
    d = _DeviceSegments(state, sr.with_radius(segs[:257], np.inf))
    try:
        a, b = d.query().copy(), d.query().copy()          # query() checks the 0xCD guard behind record n
    finally:
        d.free()
    assert np.array_equal(a, b) and np.array_equal(a, ref_inf[:257])


def test_scene_memory_is_what_it_was(gpu_state_factory):
    """A default scene holds the fp16 nodes only, and the call leaves it so."""
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    before = pt.getBvhInfo(state).device_bytes
    g = sr.with_radius(sr.segment_set("short", obj.getVerticesFloat(), obj.getIndexBuffer())[:256], np.inf)
    rec = _query(state, g)
    assert pt.getBvhInfo(state).device_bytes == before
    assert np.array_equal(rec, _reference(obj, g))
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


def test_queries_leave_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    segs = sr.segment_set("long", obj.getVerticesFloat(), obj.getIndexBuffer())
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        _query(state, sr.with_radius(segs, np.inf))
        pt.querySegments(state, segs, 50.0)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_after_scene_edits_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    segs = np.concatenate([sr.segment_set(name, verts0, idx)[:300] for name in ("short", "long", "touching")])
    g = np.concatenate([sr.with_radius(segs, np.inf), sr.with_radius(segs, sr.set_radius("short", verts0, idx))])
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
        found = rec[:, 1] != 0xFFFFFFFF
        want = ref.copy()
        want[found, 7] = ids[ref[found, 1]]
        assert np.array_equal(rec3, rec4) and np.array_equal(rec3, want)
        assert np.array_equal(rec3[:, :7], rec[:, :7]) and (rec3[:, 7] != rec[:, 7])[found].all() and found.mean() >= 0.25
    finally:
        for s in fresh:
            pt.CleanAllTheThings(s)


def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    segs, radius, ref_inf, ref_r = references("box", "short")
    L = _L()
    d = _DeviceSegments(state, sr.with_radius(segs[:256], np.inf))
    try:
        expected = d.query().copy()
        p, o = d.bufs
        refused = {
            "null segments": L.pt_query_segments(state.context, None, 256, o),
            "null output": L.pt_query_segments(state.context, p, 256, None),
            "too many": L.pt_query_segments(state.context, p, 0x80000000, o),
            "the output is the segments": L.pt_query_segments(state.context, p, 256, p),
            "the output overlaps the segments' end": L.pt_query_segments(state.context, p, 256, p + 255 * 32),
            "the segments lie inside the output": L.pt_query_segments(state.context, o + 1024, 64, o),
            "segments not aligned": L.pt_query_segments(state.context, p + 4, 16, o),
            "output not aligned": L.pt_query_segments(state.context, p, 16, o + 8),
            "null context": L.pt_query_segments(None, p, 256, o),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_segments(state.context, None, 256, o) != 0 and _err(state).startswith("pt_query_segments: ")
        assert L.pt_query_segments(state.context, p, 0x80000000, o) != 0 and "too many segments" in _err(state)
        assert L.pt_query_segments(state.context, p, 256, p) != 0 and "overlaps" in _err(state)
        assert L.pt_query_segments(state.context, p + 4, 16, o) != 0 and "aligned" in _err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_segments(bare, p, 256, o) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_segments(bare, None, 0, None) == 0               # no segments: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_segments(state.context, None, 0, None) == 0
        assert np.array_equal(d.query(), expected)                             # the next valid call
        assert np.array_equal(expected, ref_inf[:256])
    finally:
        d.free()


@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_visit_counts_of_the_test_hook(scenes, references, scene):
    """pt_debug_segments_visits: the same records, with the second bound and without it, and counts that make sense — no query visits
    more nodes or tests more triangles than the scene has, every searchable one tests at least one, a miss before any traversal
    none; on the long set the second bound saves visits."""
    state, obj = scenes(scene)
    info = pt.getBvhInfo(state)
    n_tris = len(obj.getIndexBuffer()) // 3
    L = _L()
    for name, r in (("long", np.inf), ("touching", 0.0), ("shell", None)):
        segs, radius, ref_inf, ref_r = references(scene, name)
        n = 257
        g = sr.with_radius(segs[:n], radius if r is None else r)
        g[5, 0] = np.nan                                   # one miss before any traversal
        want = _reference(obj, g)
        d = _DeviceSegments(state, g)
        try:
            rec, counts = d.visits(0)
            rec_off, counts_off = d.visits(1)
            assert np.array_equal(rec, want), (name,) + _diff(rec, want)
            assert np.array_equal(rec_off, want), (name,) + _diff(rec_off, want)
            ok = sr.searchable(g)
            assert not counts[~ok].any() and not counts_off[~ok].any()
            for c in (counts, counts_off):
                assert (c[ok, 0] >= 1).all() and (c[:, 0] <= info.n_nodes).all() and (c[:, 1] <= n_tris).all()
                assert (c[ok & (want[:, 1] != 0xFFFFFFFF), 1] >= 1).all()
            if r is not None and np.isinf(r):
                assert (counts[ok, 1] >= 1).all()
                assert counts[:, 1].mean() < n_tris / 4           # the boxes prune: far from a brute force
            if name == "long":           # what the second bound is for: a long diagonal segment no longer enters every box of its own box
                assert counts[:, 0].sum() < counts_off[:, 0].sum() and counts[:, 1].sum() <= counts_off[:, 1].sum()
            assert L.pt_debug_segments_visits(state.context, d.bufs[0], n, d.bufs[1], None, 0) != 0 and "null argument" in _err(state)
            assert L.pt_debug_segments_visits(state.context, d.bufs[0], n, d.bufs[1], d.bufs[1], 2) != 0 and "flags" in _err(state)
        finally:
            d.free()


def test_zero_length_segments_beside_the_closest_point_query(scenes):
    """A segment without length is a point.  Feature 0 is pt_query_nearest's statement at that point; an edge test may come out below
    it by the rounding of another way to the same point of the edge, never above, and nothing can cross.  The distance is within the
    host test's fp32 bar of pt_query_nearest's on the same point: the bar was measured on coordinates up to 10 and errors grow with
    the coordinates, so it is taken times S / 10."""
    state, obj = scenes("box")
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    pts = nr.point_set("inside", verts, idx, None)[:512]
    pts = np.concatenate([pts, nr.feature_points(verts, idx)[::17][:512]])
    near = pt.queryNearest(state, pts)
    got = pt.querySegments(state, np.concatenate([pts, pts], axis=1))
    lo, hi = nr.scene_box(verts, idx)
    scale = float(np.abs(np.concatenate([lo, hi])).max())
    assert (got["prim"] != 0xFFFFFFFF).all() and (got["s"] == 0).all()
    assert (got["distance"] <= near["distance"]).all()
    worst = np.abs(got["distance"].astype(np.float64) - near["distance"]).max()
    print("largest |segment - nearest| distance on %d points: %.3e (bar %.3e)" % (pts.shape[0], worst, DIST_BOUND * scale / 10.0))
    assert worst <= DIST_BOUND * scale / 10.0
    assert np.isin(got["feature"], (0.0, 2.0, 3.0, 4.0)).all() and (got["feature"] == 0.0).mean() >= 0.5
    same = got["feature"] == 0.0
    assert np.array_equal(got["distance"][same].view(np.uint32), near["distance"][same].view(np.uint32))


def test_querysegments_numpy_path(scenes, references):
    state, obj = scenes("diffuse")
    segs, radius, ref_inf, ref_r = references("diffuse", "long")
    got = pt.querySegments(state, segs, float(radius))
    assert got["distance"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32 and got["feature"].dtype == np.float32
    assert got["point"].shape == (segs.shape[0], 3) and got["s"].shape == (segs.shape[0],)
    packed = np.concatenate([got["distance"].view(np.uint32)[:, None], got["prim"][:, None], got["s"].view(np.uint32)[:, None], got["feature"].view(np.uint32)[:, None],
                             got["point"].view(np.uint32), got["material"][:, None]], axis=1)
    assert np.array_equal(packed, ref_r)
    got = pt.querySegments(state, sr.with_radius(segs, np.inf).tolist())          # anything np.asarray takes; the radius in the fourth column
    assert np.array_equal(got["prim"], ref_inf[:, 1]) and np.array_equal(got["distance"].view(np.uint32), ref_inf[:, 0])


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    segs, radius, ref_inf, ref_r = references("box", "long")
    g = sr.with_radius(segs, radius)
    L = _L()
    seen = {}
    real = L.pt_query_segments
    monkeypatch.setattr(L, "pt_query_segments", lambda ctx, p, n, out: seen.update(call=(p, n, out)) or real(ctx, p, n, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(g.copy()).to(dev)
    got = pt.querySegments(state, x)
    assert seen["call"][0] == x.data_ptr() and seen["call"][1] == g.shape[0]
    assert all(v.device == dev for v in got.values())
    assert seen["call"][2] == got["distance"].data_ptr()                   # the columns are views of the tensor the library wrote
    assert got["distance"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32
    assert got["point"].shape == (g.shape[0], 3)
    cols = {"distance": ref_r[:, 0], "prim": ref_r[:, 1], "s": ref_r[:, 2], "feature": ref_r[:, 3], "material": ref_r[:, 7]}
    for k, want in cols.items():
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), k
    assert np.array_equal(got["point"].cpu().numpy().view(np.uint32), ref_r[:, 4:7])
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.querySegments(state, y)
    assert seen["call"][0] == y.data_ptr() and torch.equal(again["prim"], got["prim"]) and torch.equal(again["distance"], got["distance"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :6].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.querySegments(state, bad)
    assert pt.querySegments(state, x[:0])["distance"].shape == (0,)


def test_capsule_clearance(scenes, references):
    state, obj = scenes("box")
    segs, radius, ref_inf, ref_r = references("box", "long")
    n = 400
    rng = np.random.default_rng(9)
    r = rng.uniform(0.0, 30.0, n).astype(np.float32)
    got = pt.capsuleClearance(state, segs[:n, 0:3], segs[:n, 3:6], r)
    f = ref_inf.view(np.float32)[:n]
    assert np.array_equal(got["prim"], ref_inf[:n, 1])
    assert np.array_equal(got["clearance"].view(np.uint32), (f[:, 0] - r).astype(np.float32).view(np.uint32))
    crossing = f[:, 3] == 5
    assert crossing.mean() >= 0.05 and np.array_equal(got["clearance"][crossing], -r[crossing])        # the axis passes through the surface
    assert (got["clearance"] < 0).mean() >= 0.1 and (got["clearance"] > 0).mean() >= 0.1
    assert np.array_equal(got["on_mesh"].view(np.uint32), ref_inf[:n, 4:7])
    want_axis = (segs[:n, 0:3] + (segs[:n, 3:6] - segs[:n, 0:3]) * f[:, 2:3]).astype(np.float32)
    assert np.array_equal(got["on_axis"], want_axis)
    # the witness points are as far apart as the distance says, to the rounding of forming them
    gap = np.linalg.norm(got["on_axis"].astype(np.float64) - got["on_mesh"], axis=1)
    assert np.abs(gap - f[:, 0]).max() <= 1e-3
    one = pt.capsuleClearance(state, segs[:5, 0:3], segs[:5, 3:6], 2.5)                                # one radius for all
    assert np.array_equal(one["clearance"], (f[:5, 0] - F(2.5)).astype(np.float32))


def test_cli_clearance_prints_what_querysegments_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (F(0.5) * (lo + hi)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    queries = [(c[0], c[1], c[2], c[0] + F(20.0), c[1] + F(5.0), c[2] - F(10.0), None),
               (c[0], hi[1] - F(50.0), c[2], c[0] + F(3.0), hi[1] + F(50.0), c[2] + F(2.0), F(4.5)),           # through the ceiling
               (lo[0] + F(10.0), c[1] + F(3.25), c[2] - F(7.5), lo[0] + F(12.0), c[1], c[2], F(25.0)),         # a fat capsule by the wall: penetrates
               (hi[0] + F(100.0), hi[1] + F(50.0), hi[2], hi[0] + F(130.0), hi[1], hi[2], F(0.0))]
    queries = [tuple(None if a is None else float(np.float32(a)) for a in q) for q in queries]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for q in queries:
        cmd += ["--clearance", ",".join("%r" % a for a in q if a is not None)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"clearance"')]
    assert len(lines) == len(queries)
    p0 = np.array([q[0:3] for q in queries], np.float32)
    p1 = np.array([q[3:6] for q in queries], np.float32)
    radii = np.array([0.0 if q[6] is None else q[6] for q in queries], np.float32)
    got = pt.querySegments(state, np.concatenate([p0, p1], axis=1))
    cap = pt.capsuleClearance(state, p0, p1, radii)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    assert (got["prim"] != 0xFFFFFFFF).all() and got["feature"][1] == 5 and got["distance"][1] == 0 and cap["clearance"][2] < 0
    for i, line in enumerate(lines):
        assert np.array_equal(np.array(line["clearance"], np.float32), np.concatenate([p0[i], p1[i]]))
        assert np.float32(line["radius"]) == radii[i]
        assert line["found"] is True and line["triangle"] == int(got["prim"][i])
        assert np.float32(line["distance"]) == got["distance"][i] and np.float32(line["clear"]) == cap["clearance"][i]
        assert line["material"] == names[int(got["material"][i])]
        assert np.float32(line["s"]) == got["s"][i] and line["feature"] == int(got["feature"][i])
        assert np.array_equal(np.array(line["point"], np.float32), got["point"][i])
        assert np.array_equal(np.array(line["on_segment"], np.float32), cap["on_axis"][i])
    for arg in ("1,2,3,4,5", "1,2,nan,4,5,6", "1,2,3,4,5,inf", "1,2,3,4,5,6,-1", "1,2,3,4,5,6,nan", "1,2,3,4,5,6,inf"):
        bad = subprocess.run([exe, "--obj", BOX, "--clearance", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--clearance" in bad.stderr, arg
