"""Closest-point queries on the GPU: pt_query_nearest against tests/nearest_ref.py's brute force (the whole record, bits) on every
scene, size, point set and radius, the points that are a miss before any traversal, the output's bounds, the scene's memory, scene
edits, the render state, the refusals, torch tensors, bakeDistanceField and acgpt_main --nearest."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import nearest_ref as nr

F = np.float32
pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


def _camera(state):
    p = state.params
    return p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple()


def _host_closest(state, rays):
    rays = np.ascontiguousarray(rays, np.float32)
    n = rays.shape[0]
    t = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32)
    assert _L().pt_trace_closest(state.context, rays.ctypes.data, n, t.ctypes.data, prim.ctypes.data) == 0, _err(state)
    return t, prim


GUARD = 64          # bytes of 0xCD kept behind the records


class _DevicePoints:
    """points in a device buffer with room for the records and a guard behind them; the C ABI called as a C caller would"""
    def __init__(self, state, points):
        self.state, self.n = state, points.shape[0]
        self.points = np.ascontiguousarray(points, np.float32)
        assert self.points.shape == (self.n, 4)
        self.bufs = pt.pathtracer._device_buffers(state, 2, max(self.n * 32, 32) + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.points.ctypes.data, self.points.nbytes) == 0

    def nearest(self):
        L, s = _L(), self.state
        assert L.pt_device_memset(s.context, self.bufs[1], 0xCD, self.n * 32 + GUARD) == 0
        assert L.pt_query_nearest(s.context, self.bufs[0], self.n, self.bufs[1]) == 0, _err(s)
        raw = np.zeros(self.n * 8 + GUARD // 4, np.uint32)
        assert L.pt_copy_to_host(s.context, raw.ctypes.data, self.bufs[1], raw.nbytes) == 0
        assert (raw[self.n * 8:] == 0xCDCDCDCD).all(), "written past record %d" % self.n
        return raw[:self.n * 8].reshape(self.n, 8)

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _query(state, points):
    d = _DevicePoints(state, points)
    try:
        return d.nearest()
    finally:
        d.free()


def _reference(obj, points):
    return nr.nearest_records(points, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices())


def _diff(rec, ref):
    bad = np.flatnonzero((rec != ref).any(axis=1))
    return (bad[:4], rec[bad][:2], rec[bad][:2].view(np.float32), ref[bad][:2], ref[bad][:2].view(np.float32))


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
    """(scene, set) -> (points, radius, records at +inf, records at the radius) by the brute force on the whole set: computed once,
    shared, never written.  The fp32-node scene is the box: it shares the box's."""
    cache = {}

    def get(scene, name):
        key = ("box" if scene == "fp32" else scene, name)
        if key not in cache:
            state, obj = scenes(key[0])
            verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
            pts = nr.point_set(name, verts, idx, _camera(state), first_hits=lambda rays: _host_closest(state, rays))
            radius = nr.set_radius(name, verts, idx)
            out = (pts, radius, _reference(obj, nr.with_radius(pts, np.inf)), _reference(obj, nr.with_radius(pts, radius)))
            for a in (out[0], out[2], out[3]):
                a.setflags(write=False)
            cache[key] = out
        return cache[key]

    return get


def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@pytest.mark.parametrize("name", nr.POINT_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_records_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    pts, radius, ref_inf, ref_r = references(scene, name)
    # the set still does what it is there for, by the reference's own answers: a set that lost its finds must not pass vacuously
    found = ref_r[:, 1] != 0xFFFFFFFF
    assert found.mean() >= 0.25 and (~found).mean() >= 0.10, (name, found.mean())
    assert np.unique(ref_r[found, 1]).size >= 8 and (ref_inf[:, 1] != 0xFFFFFFFF).all()
    before = pt.getBvhInfo(state).device_bytes
    for r, ref in ((np.inf, ref_inf), (radius, ref_r)):
        points = nr.with_radius(pts, r)
        for n in SIZES:
            rec = _query(state, points[:n])
            assert np.array_equal(rec, ref[:n]), (scene, name, float(r), n) + _diff(rec, ref[:n])
    assert pt.getBvhInfo(state).device_bytes == before


@pytest.fixture(scope="module")
def feature_reference(scenes):
    """(points, records) of every vertex, edge midpoint and centroid of the box: computed once, shared, never written"""
    state, obj = scenes("box")
    pts = nr.feature_points(obj.getVerticesFloat(), obj.getIndexBuffer())
    assert pts.shape[0] == 7 * (len(obj.getIndexBuffer()) // 3) > 5000
    points = nr.with_radius(pts, np.inf)
    ref = _reference(obj, points)
    points.setflags(write=False); ref.setflags(write=False)
    return points, ref


@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_every_vertex_edge_midpoint_and_centroid(scenes, feature_reference, scene):
    """All of them, 7 per triangle, on both node formats: points on the surface whose winner is decided among the triangles that share
    the vertex or the edge, d2 equal or an ulp apart"""
    state, obj = scenes(scene)
    points, ref = feature_reference
    assert (ref.view(np.float32)[:, 0] <= 1e-3).all() and (ref.view(np.float32)[:, 0] == 0).mean() > 0.5
    rec = _query(state, points)
    assert np.array_equal(rec, ref), _diff(rec, ref)


def test_bad_points_between_good_ones(scenes, references):
    state, obj = scenes("box")
    pts, radius, ref_inf, ref_r = references("box", "inside")
    good = nr.with_radius(pts[:64], np.inf)
    bad, why = nr.bad_points(good[0])
    assert bad.shape[0] < 32
    mixed = good.copy()
    where = 2 * np.arange(bad.shape[0]) + 1                 # every other lane of the first wave
    mixed[where] = bad
    still_good = np.ones(64, bool); still_good[where] = False
    rec = _query(state, mixed)
    wrong = (rec[where] != nr.miss_records(where.size)).any(axis=1)
    assert not wrong.any(), [why[i] for i in np.flatnonzero(wrong)]
    assert np.array_equal(rec[still_good], ref_inf[:64][still_good])
    assert np.array_equal(rec, _reference(obj, mixed))
    # points that look odd and are points: a radius of +-0 on a surface point and beside it, a huge radius whose square overflows
    v = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)[obj.getIndexBuffer()[0], :3]
    odd = np.array([[v[0], v[1], v[2], 0.0], [v[0], v[1], v[2], -0.0], [v[0] + 1.0, v[1] + 1.0, v[2] + 1.0, 0.0], [v[0], v[1], v[2], 1e30]], np.float32)
    assert nr.searchable(odd).all()
    rec, ref = _query(state, odd), _reference(obj, odd)
    assert np.array_equal(rec, ref), _diff(rec, ref)
    assert rec[0, 1] != 0xFFFFFFFF and rec[0, 0] == 0 and rec[1, 1] == rec[0, 1] and rec[3, 1] == rec[0, 1]


def test_two_calls_give_the_same_bits_and_nothing_is_written_past_n(scenes, references):
    state, obj = scenes("diffuse")
    pts, radius, ref_inf, ref_r = references("diffuse", "wall_planes")
    d = _DevicePoints(state, nr.with_radius(pts[:257], radius))
    try:
        a, b = d.nearest().copy(), d.nearest().copy()          # nearest() checks the 0xCD guard behind record n
    finally:
        d.free()
    assert np.array_equal(a, b) and np.array_equal(a, ref_r[:257])


def test_scene_memory_is_what_it_was(gpu_state_factory):
    """A default scene holds the fp16 nodes only, and the call leaves it so."""
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    before = pt.getBvhInfo(state).device_bytes
    pts = nr.point_set("inside", obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))[:256]
    rec = _query(state, nr.with_radius(pts, np.inf))
    assert pt.getBvhInfo(state).device_bytes == before
    assert np.array_equal(rec, _reference(obj, nr.with_radius(pts, np.inf)))
    _host_closest(state, np.array([[0, 0, 0, 0, 0, 1, 0, 1]], np.float32))   # now the fp32 nodes come
    assert pt.getBvhInfo(state).device_bytes > before


def test_queries_leave_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    pts = nr.point_set("inside", obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        _query(state, nr.with_radius(pts, np.inf))
        pt.queryNearest(state, pts, 50.0)
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
    cam = _camera(state)
    pts = np.concatenate([nr.point_set(name, verts0, idx, cam, first_hits=lambda rays: _host_closest(state, rays))[:400] for name in ("surface", "inside", "wall_planes")])
    points = np.concatenate([nr.with_radius(pts, np.inf), nr.with_radius(pts, nr.set_radius("inside", verts0, idx))])
    _query(state, points)                                    # the queries have run on the scene before it changes
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
        rec, rec2 = _query(state, points), _query(fresh[-1], points)
        ref = _reference(moved, points)
        assert np.array_equal(rec, rec2), _diff(rec, rec2)
        assert np.array_equal(rec, ref), _diff(rec, ref)
        assert (ref != _reference(obj, points)).any()         # the move shows in the answers
        # 2. new material assignments on top: the ids rotate by one
        n_mats = obj.getNumMaterials()
        ids = ((np.asarray(obj.getMaterialIndices(), np.uint32) + 1) % n_mats).astype(np.uint32)
        pt.updateMaterials(state, material_ids=ids)
        moved._materialIndices = ids
        fresh.append(_fresh_state(state, moved))
        rec3, rec4 = _query(state, points), _query(fresh[-1], points)
        assert np.array_equal(rec3, rec4) and np.array_equal(rec3, _reference(moved, points))
        found = rec[:, 1] != 0xFFFFFFFF
        assert np.array_equal(rec3[:, :7], rec[:, :7]) and (rec3[:, 7] != rec[:, 7])[found].all() and found.mean() >= 0.25
    finally:
        for s in fresh:
            pt.CleanAllTheThings(s)


def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    pts, radius, ref_inf, ref_r = references("box", "inside")
    L = _L()
    d = _DevicePoints(state, nr.with_radius(pts[:256], np.inf))
    try:
        expected = d.nearest().copy()
        p, o = d.bufs
        refused = {
            "null points": L.pt_query_nearest(state.context, None, 256, o),
            "null output": L.pt_query_nearest(state.context, p, 256, None),
            "too many": L.pt_query_nearest(state.context, p, 0x80000000, o),
            "the output is the points": L.pt_query_nearest(state.context, p, 256, p),
            "the output overlaps the points' end": L.pt_query_nearest(state.context, p, 256, p + 255 * 16),
            "the points lie inside the output": L.pt_query_nearest(state.context, o + 1024, 64, o),
            "points not aligned": L.pt_query_nearest(state.context, p + 4, 16, o),
            "output not aligned": L.pt_query_nearest(state.context, p, 16, o + 8),
            "null context": L.pt_query_nearest(None, p, 256, o),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_nearest(state.context, None, 256, o) != 0 and _err(state).startswith("pt_query_nearest: ")
        assert L.pt_query_nearest(state.context, p, 0x80000000, o) != 0 and "too many points" in _err(state)
        assert L.pt_query_nearest(state.context, p, 256, p) != 0 and "overlaps" in _err(state)
        assert L.pt_query_nearest(state.context, p + 4, 16, o) != 0 and "aligned" in _err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_nearest(bare, p, 256, o) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_nearest(bare, None, 0, None) == 0                # no points: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_nearest(state.context, None, 0, None) == 0
        assert np.array_equal(d.nearest(), expected)                           # the next valid call
        assert np.array_equal(expected, ref_inf[:256])
    finally:
        d.free()


def test_visit_counts_of_the_test_hook(scenes, references):
    """pt_debug_nearest_visits: the same records, and counts that make sense — a point on the surface under radius 0 still reaches a
    leaf, and no query tests more triangles than the scene has."""
    state, obj = scenes("box")
    pts, radius, ref_inf, ref_r = references("box", "surface")
    n = 257
    d = _DevicePoints(state, nr.with_radius(pts[:n], np.inf))
    L = _L()
    vis = pt.pathtracer._device_buffers(state, 1, n * 8)
    try:
        assert L.pt_debug_nearest_visits(state.context, d.bufs[0], n, d.bufs[1], vis[0]) == 0, _err(state)
        rec = np.zeros((n, 8), np.uint32); counts = np.zeros((n, 2), np.uint32)
        assert L.pt_copy_to_host(state.context, rec.ctypes.data, d.bufs[1], rec.nbytes) == 0
        assert L.pt_copy_to_host(state.context, counts.ctypes.data, vis[0], counts.nbytes) == 0
        assert np.array_equal(rec, ref_inf[:n])
        n_tris = len(obj.getIndexBuffer()) // 3
        assert (counts[:, 0] >= 1).all() and (counts[:, 1] >= 1).all() and (counts[:, 1] <= n_tris).all() and (counts[:, 0] < n_tris).all()
        assert counts[:, 1].mean() < n_tris / 4           # the boxes prune: far from a brute force
        assert L.pt_debug_nearest_visits(state.context, d.bufs[0], n, d.bufs[1], None) != 0 and "null argument" in _err(state)
    finally:
        pt.pathtracer._free_device_buffers(state, vis)
        d.free()


def test_querynearest_numpy_path(scenes, references):
    state, obj = scenes("diffuse")
    pts, radius, ref_inf, ref_r = references("diffuse", "inside")
    got = pt.queryNearest(state, pts, float(radius))
    assert got["distance"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32
    assert got["point"].shape == (pts.shape[0], 3) and got["u"].shape == (pts.shape[0],)
    packed = np.concatenate([got["distance"].view(np.uint32)[:, None], got["prim"][:, None], got["u"].view(np.uint32)[:, None], got["v"].view(np.uint32)[:, None],
                             got["point"].view(np.uint32), got["material"][:, None]], axis=1)
    assert np.array_equal(packed, ref_r)
    got = pt.queryNearest(state, nr.with_radius(pts, np.inf).tolist())          # anything np.asarray takes; the radius in the fourth column
    assert np.array_equal(got["prim"], ref_inf[:, 1]) and np.array_equal(got["distance"].view(np.uint32), ref_inf[:, 0])


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    pts, radius, ref_inf, ref_r = references("box", "inside")
    points = nr.with_radius(pts, radius)
    L = _L()
    seen = {}
    real = L.pt_query_nearest
    monkeypatch.setattr(L, "pt_query_nearest", lambda ctx, p, n, out: seen.update(call=(p, n, out)) or real(ctx, p, n, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(points.copy()).to(dev)
    got = pt.queryNearest(state, x)
    assert seen["call"][0] == x.data_ptr() and seen["call"][1] == points.shape[0]
    assert all(v.device == dev for v in got.values())
    assert seen["call"][2] == got["distance"].data_ptr()                   # the columns are views of the tensor the library wrote
    assert got["distance"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32
    assert got["point"].shape == (points.shape[0], 3)
    cols = {"distance": ref_r[:, 0], "prim": ref_r[:, 1], "u": ref_r[:, 2], "v": ref_r[:, 3], "material": ref_r[:, 7]}
    for k, want in cols.items():
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), k
    assert np.array_equal(got["point"].cpu().numpy().view(np.uint32), ref_r[:, 4:7])
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.queryNearest(state, y)
    assert seen["call"][0] == y.data_ptr() and torch.equal(again["prim"], got["prim"]) and torch.equal(again["distance"], got["distance"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :3].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.queryNearest(state, bad)
    assert pt.queryNearest(state, x[:0])["distance"].shape == (0,)


def test_bake_distance_field_against_the_reference(scenes):
    state, obj = scenes("box")
    info = pt.getBvhInfo(state)
    lo, hi = [float(x) for x in info.scene_lo], [float(x) for x in info.scene_hi]
    dist, prims = pt.bakeDistanceField(state, (9, 7, 5), return_prims=True)
    assert dist.shape == (9, 7, 5) and dist.dtype == np.float32 and prims.shape == (9, 7, 5) and prims.dtype == np.uint32
    pts = pt.distanceFieldPoints((9, 7, 5), lo, hi)
    ref = _reference(obj, nr.with_radius(pts, np.inf))
    assert np.array_equal(dist.reshape(-1).view(np.uint32), ref[:, 0]) and np.array_equal(prims.reshape(-1), ref[:, 1])
    assert (dist >= 0).all() and np.unique(prims).size >= 8
    # a grid of the caller's, with a radius: cells beyond it hold -1
    bounds = ((lo[0], lo[1], lo[2]), (0.5 * (lo[0] + hi[0]), hi[1], hi[2]))
    r = 0.05 * float(np.sqrt(sum((hi[k] - lo[k]) ** 2 for k in range(3))))
    near = pt.bakeDistanceField(state, (5, 7, 9), bounds=bounds, max_radius=r)
    ref = _reference(obj, nr.with_radius(pt.distanceFieldPoints((5, 7, 9), *bounds), r))
    assert np.array_equal(near.reshape(-1).view(np.uint32), ref[:, 0])
    assert (near == -1).mean() >= 0.1 and (near >= 0).mean() >= 0.1


def test_cli_nearest_prints_what_querynearest_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (F(0.5) * (lo + hi)).astype(np.float32)
    far = (hi + np.array([100.0, 50.0, 0.0], np.float32)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    queries = [(c[0], c[1], c[2], None), (lo[0] + F(10.0), c[1] + F(3.25), c[2] - F(7.5), F(25.0)), (far[0], far[1], far[2], F(1.0)), (far[0], far[1], far[2], None)]
    queries = [tuple(None if a is None else float(np.float32(a)) for a in q) for q in queries]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for x, y, z, r in queries:
        cmd += ["--nearest", "%r,%r,%r" % (x, y, z) + ("" if r is None else ",%r" % r)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"nearest"')]
    assert len(lines) == len(queries)
    points = np.array([[x, y, z, np.inf if r is None else r] for x, y, z, r in queries], np.float32)
    got = pt.queryNearest(state, points)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    assert got["prim"][0] != 0xFFFFFFFF and got["prim"][2] == 0xFFFFFFFF and got["prim"][3] != 0xFFFFFFFF      # nothing within 1 of the far point
    for i, line in enumerate(lines):
        assert np.array_equal(np.array(line["nearest"], np.float32), points[i, :3])
        if got["prim"][i] == 0xFFFFFFFF:
            assert line == {"nearest": line["nearest"], "found": False}
            continue
        assert line["found"] is True and line["triangle"] == int(got["prim"][i])
        assert np.float32(line["distance"]) == got["distance"][i]
        assert line["material"] == names[int(got["material"][i])]
        assert np.array_equal(np.array(line["point"], np.float32), got["point"][i])
        assert np.float32(line["u"]) == got["u"][i] and np.float32(line["v"]) == got["v"][i]
    for arg in ("1,2", "1,2,nan", "1,2,3,-1", "1,2,3,nan"):
        bad = subprocess.run([exe, "--obj", BOX, "--nearest", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--nearest" in bad.stderr, arg
