"""Translating-triangle casts on the GPU: pt_query_triangle_cast against tests/tricast_ref.py's brute force (the whole record, bits) and
pt_query_triangle_cast_any against the records, on every cast set and size and both node formats; the counting twin, the output's
bounds, the scene's memory and the render state, scene edits, the refusals, the cross-checks against pt_query_triangles* and
pt_query_triangle_distance, the wrappers with arrays and tensors and castContacts."""
import ctypes as C
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import nearest_ref as nr
import tricast_ref as tc
from test_tricast_host import CONTACT_BOUND

F = np.float32
pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
GUARD = 64                                         # bytes of 0xCD kept behind every output


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


class _DeviceCasts:
    """casts in a device buffer, with buffers for the records, the bytes and the visit counts and a guard behind each; the C ABI
    called as a C caller would"""
    def __init__(self, state, casts):
        self.state, self.n = state, casts.shape[0]
        self.casts = np.ascontiguousarray(casts, np.float32)
        assert self.casts.shape == (self.n, 16)
        self.bufs = pt.pathtracer._device_buffers(state, 4, max(self.n * 64, 64) + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.casts.ctypes.data, self.casts.nbytes) == 0

    def _read(self, ptr, nbytes):
        raw = np.zeros(nbytes + GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, ptr, raw.nbytes) == 0
        assert (raw[nbytes:] == 0xCD).all(), "written past the end of the output"
        return raw[:nbytes]

    def _arm(self, ptr, nbytes):
        assert _L().pt_device_memset(self.state.context, ptr, 0xCD, nbytes + GUARD) == 0

    def cast(self):
        self._arm(self.bufs[1], self.n * 32)
        assert _L().pt_query_triangle_cast(self.state.context, self.bufs[0], self.n, self.bufs[1]) == 0, _err(self.state)
        return self._read(self.bufs[1], self.n * 32).view(np.uint32).reshape(self.n, 8)

    def blocked(self, offset=0):
        self._arm(self.bufs[2], self.n + offset)
        assert _L().pt_query_triangle_cast_any(self.state.context, self.bufs[0], self.n, self.bufs[2] + offset) == 0, _err(self.state)
        raw = self._read(self.bufs[2], self.n + offset)
        assert (raw[:offset] == 0xCD).all()
        return raw[offset:]

    def visits(self):
        self._arm(self.bufs[1], self.n * 32)
        self._arm(self.bufs[3], self.n * 8)
        assert _L().pt_debug_triangle_cast_visits(self.state.context, self.bufs[0], self.n, self.bufs[1], self.bufs[3]) == 0, _err(self.state)
        return (self._read(self.bufs[1], self.n * 32).view(np.uint32).reshape(self.n, 8), self._read(self.bufs[3], self.n * 8).view(np.uint32).reshape(self.n, 2))

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _query(state, casts):
    """(records, blocked bytes) of the two calls"""
    d = _DeviceCasts(state, casts)
    try:
        return d.cast().copy(), d.blocked().copy()
    finally:
        d.free()


def _reference(obj, casts):
    return tc.cast_records(casts, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices())


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
    """The Cornell box under the default variant (fp16 centre / half-extent nodes) and under an fp32-node variant, each set up once.
    name -> (state, obj)"""
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
                made[name] = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
        return made[name]

    yield get
    for s in extra:
        pt.CleanAllTheThings(s)


@pytest.fixture(scope="module")
def references(scenes):
    """set -> (casts, records) of the box by the brute force on the whole set: computed once, shared, never written"""
    cache = {}

    def get(name):
        if name not in cache:
            state, obj = scenes("box")
            s = tc.cast_set(name, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices())
            ref = _reference(obj, s)
            s.setflags(write=False); ref.setflags(write=False)
            cache[name] = (s, ref)
        return cache[name]

    return get


def test_unchanged_hash_and_abi_version():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH
    assert _L().pt_abi_version() == 4


@pytest.mark.parametrize("name", tc.CAST_SETS)
@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_records_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    s, ref = references(name)
    hit = ref[:, 1] != 0xFFFFFFFF
    # the set still does what it is there for, by the reference's own answers: a set that lost its hits must not pass vacuously
    assert hit.mean() >= 0.2 and np.unique(ref[hit, 1]).size >= 8, (name, hit.mean())
    if name in ("short", "outside", "zero_d", "bad"):
        assert (~hit).mean() >= 0.2, name
    before = pt.getBvhInfo(state).device_bytes
    for n in SIZES:
        rec, blocked = _query(state, s[:n])
        assert np.array_equal(rec, ref[:n]), (scene, name, n) + _diff(rec, ref[:n])
        assert np.array_equal(blocked, tc.blocked_of(ref[:n])), (scene, name, n, np.flatnonzero(blocked != tc.blocked_of(ref[:n]))[:8])
    assert pt.getBvhInfo(state).device_bytes == before
    if name == "bad":
        assert np.array_equal(ref[~tc.castable(s)], tc.miss_records(int((~tc.castable(s)).sum())))


def test_blocked_may_have_any_alignment(scenes, references):
    state, obj = scenes("box")
    s, ref = references("outside")
    d = _DeviceCasts(state, s[:257])
    try:
        for offset in (1, 2, 3, 7):
            assert np.array_equal(d.blocked(offset), tc.blocked_of(ref[:257])), offset
    finally:
        d.free()


def test_counting_twin(scenes, references):
    """pt_debug_triangle_cast_visits: the same records, no cast tests more triangles than the scene has, the boxes prune, and a cast
    whose swept box misses the scene box visits the root at most and tests nothing"""
    for scene in ("box", "fp32"):
        state, obj = scenes(scene)
        n_tris = len(obj.getIndexBuffer()) // 3
        for name in ("aimed", "grazing"):
            s, ref = references(name)
            d = _DeviceCasts(state, s[:257])
            try:
                rec, vis = d.visits()
            finally:
                d.free()
            assert np.array_equal(rec, ref[:257]), (scene, name) + _diff(rec, ref[:257])
            assert (vis[:, 1] <= n_tris).all() and (vis[:, 0] < n_tris).all() and (vis[:, 0] >= 1).all()
            assert vis[:, 1].mean() < n_tris / 4, (scene, name, vis[:, 1].mean())
        lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
        c = 0.5 * (lo + hi)
        shape = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 5.0], [0.0, 10.0, -5.0]])
        # beside the box, running along it; towards it, but too short to reach; away from it
        away = tc.pack(np.array([[hi[0] + 100.0, c[1], c[2]], [hi[0] + 100.0, c[1], c[2]], [c[0], hi[1] + 50.0, c[2]], [c[0], c[1], lo[2] - 500.0]])[:, None, :] + shape[None],
                       np.array([[0.01, 1.0, 0.37], [-1.0, 0.2, 0.1], [0.3, 1.0, -0.2], [0.1, 0.1, -1.0]]), np.array([10.0, 25.0, np.inf, np.inf]))
        d = _DeviceCasts(state, away)
        try:
            rec, vis = d.visits()
        finally:
            d.free()
        assert np.array_equal(rec, tc.miss_records(4)) and np.array_equal(rec, _reference(obj, away))
        assert (vis[:, 0] <= 1).all() and (vis[:, 1] == 0).all(), vis
        d = _DeviceCasts(state, away)
        try:
            assert _L().pt_debug_triangle_cast_visits(state.context, d.bufs[0], 4, d.bufs[1], None) != 0 and "null argument" in _err(state)
            assert _L().pt_debug_triangle_cast_visits(state.context, d.bufs[0], 4, d.bufs[1], d.bufs[3] + 4) != 0 and "visit counts must be 8-byte aligned" in _err(state)
            assert _L().pt_debug_triangle_cast_visits(state.context, d.bufs[0], 4, d.bufs[1] + 8, d.bufs[3]) != 0 and "16-byte aligned" in _err(state)
        finally:
            d.free()


def test_two_calls_give_the_same_bits(scenes, references):
    state, obj = scenes("box")
    s, ref = references("aimed")
    d = _DeviceCasts(state, s[:257])
    try:
        a, b = d.cast().copy(), d.cast().copy()            # cast() checks the 0xCD guard behind record n
        x, y = d.blocked().copy(), d.blocked().copy()
    finally:
        d.free()
    assert np.array_equal(a, b) and np.array_equal(a, ref[:257]) and np.array_equal(x, y)


def test_queries_leave_the_scene_memory_and_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    s = tc.cast_set("aimed", obj.getVerticesFloat(), obj.getIndexBuffer())
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for st, o in ((state, ob), (twin, None)):
            st.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, st, 1)
        acc, fb, stats = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        rec, blocked = _query(state, s)
        got = pt.queryTriangleCast(state, s)
        assert np.array_equal(got["prim"], rec[:, 1]) and np.array_equal(pt.queryTriangleCast(state, s, any_hit=True), blocked.view(np.bool_))
        assert pt.getBvhInfo(state).device_bytes == before              # a default scene holds the fp16 nodes only, and stays so
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == stats
        for st, o in ((state, ob), (twin, None)):
            st.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, st, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_after_scene_edits_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    casts = np.concatenate([tc.cast_set(name, verts0, idx, obj.getMaterialIndices())[:300] for name in ("aimed", "links", "grazing")])
    _query(state, casts)                                     # the queries have run on the scene before it changes
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
        (rec, blk), (rec2, blk2) = _query(state, casts), _query(fresh[-1], casts)
        ref = _reference(moved, casts)
        assert np.array_equal(rec, rec2), _diff(rec, rec2)
        assert np.array_equal(rec, ref), _diff(rec, ref)
        assert np.array_equal(blk, blk2) and np.array_equal(blk, tc.blocked_of(ref))
        assert (ref != _reference(obj, casts)).any()          # the move shows in the answers
        # 2. new material assignments on top: the ids rotate by one
        n_mats = obj.getNumMaterials()
        ids = ((np.asarray(obj.getMaterialIndices(), np.uint32) + 1) % n_mats).astype(np.uint32)
        pt.updateMaterials(state, material_ids=ids)
        moved._materialIndices = ids
        fresh.append(_fresh_state(state, moved))
        rec3, rec4 = _query(state, casts)[0], _query(fresh[-1], casts)[0]
        assert np.array_equal(rec3, rec4) and np.array_equal(rec3, _reference(moved, casts))
        found = rec[:, 1] != 0xFFFFFFFF
        assert np.array_equal(rec3[:, :7], rec[:, :7]) and (rec3[:, 7] != rec[:, 7])[found].all() and found.mean() >= 0.25
    finally:
        for s in fresh:
            pt.CleanAllTheThings(s)


def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    s, ref = references("aimed")
    L = _L()
    d = _DeviceCasts(state, s[:256])
    try:
        expected = d.cast().copy()
        p, o, b = d.bufs[0], d.bufs[1], d.bufs[2]
        refused = {
            "null casts": L.pt_query_triangle_cast(state.context, None, 256, o),
            "null hits": L.pt_query_triangle_cast(state.context, p, 256, None),
            "too many": L.pt_query_triangle_cast(state.context, p, 0x80000000, o),
            "the hits are the casts": L.pt_query_triangle_cast(state.context, p, 256, p),
            "the hits overlap the casts' end": L.pt_query_triangle_cast(state.context, p, 256, p + 255 * 64),
            "the casts lie inside the hits": L.pt_query_triangle_cast(state.context, o + 1024, 64, o),
            "casts not aligned": L.pt_query_triangle_cast(state.context, p + 4, 16, o),
            "hits not aligned": L.pt_query_triangle_cast(state.context, p, 16, o + 8),
            "null context": L.pt_query_triangle_cast(None, p, 256, o),
            "any: null casts": L.pt_query_triangle_cast_any(state.context, None, 256, b),
            "any: null blocked": L.pt_query_triangle_cast_any(state.context, p, 256, None),
            "any: too many": L.pt_query_triangle_cast_any(state.context, p, 0x80000000, b),
            "any: blocked inside the casts": L.pt_query_triangle_cast_any(state.context, p, 256, p + 100),
            "any: casts not aligned": L.pt_query_triangle_cast_any(state.context, p + 4, 16, b),
            "any: null context": L.pt_query_triangle_cast_any(None, p, 256, b),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_triangle_cast(state.context, None, 256, o) != 0 and _err(state).startswith("pt_query_triangle_cast: ")
        assert L.pt_query_triangle_cast(state.context, p, 0x80000000, o) != 0 and "too many casts" in _err(state)
        assert L.pt_query_triangle_cast(state.context, p, 256, p) != 0 and "overlaps" in _err(state)
        assert L.pt_query_triangle_cast(state.context, p + 4, 16, o) != 0 and "aligned" in _err(state)
        assert L.pt_query_triangle_cast_any(state.context, p, 256, None) != 0 and _err(state).startswith("pt_query_triangle_cast_any: ")
        # the order: a null argument is named before the count, the count before the alignment, the alignment before the overlap
        assert L.pt_query_triangle_cast(state.context, None, 0x80000000, o) != 0 and "null argument" in _err(state)
        assert L.pt_query_triangle_cast(state.context, p + 4, 0x80000000, o) != 0 and "too many casts" in _err(state)
        assert L.pt_query_triangle_cast(state.context, p + 4, 16, p + 4) != 0 and "aligned" in _err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_triangle_cast(bare, p, 256, o) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_triangle_cast_any(bare, p, 256, b) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_triangle_cast(bare, None, 0, None) == 0          # no casts: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_triangle_cast(state.context, None, 0, None) == 0 and L.pt_query_triangle_cast_any(state.context, None, 0, None) == 0
        assert np.array_equal(d.cast(), expected)                              # the next valid call
        assert np.array_equal(expected, ref[:256])
    finally:
        d.free()


def test_zero_motion_is_the_intersection_query(scenes, references):
    """With d = 0 only the start overlap can answer: blocked is pt_query_triangles_any's byte and prim the first index of
    pt_query_triangles' list, on every query"""
    state, obj = scenes("box")
    s = np.concatenate([references("zero_d")[0], references("overlap")[0]]).copy()
    s[:, 12:15] = 0
    rec, blocked = _query(state, s)
    tris = tc.triangles_of(s)
    assert np.array_equal(blocked.view(np.bool_), np.asarray(pt.queryTrianglesAny(state, tris)).astype(np.bool_))
    got = pt.queryTriangles(state, tris, max_prims=1, counts=True)
    assert np.array_equal(rec[:, 1], np.asarray(got["prim"], np.uint32).reshape(-1))
    hit = blocked.view(np.bool_)
    assert 0.3 <= hit.mean() <= 0.95
    col = tc.columns(rec)
    assert (col["t"][hit] == 0).all() and (col["feature"][hit] == 15).all() and not col["point"][hit].any()


def test_moved_by_t_the_triangle_touches_the_scene(scenes, references):
    """Moving the query by the returned t and asking pt_query_triangle_distance gives a distance within the host test's bound, the
    rounding of the moved vertices to fp32 (half an ulp of a coordinate below 1024 per component) included: measured 1.05e-4."""
    state, obj = scenes("box")
    for name in ("aimed", "links"):
        s, ref = references(name)
        t = tc.columns(ref)["t"]
        hit = t >= 0
        tri = tc.moved(s[hit], t[hit]).astype(np.float32)
        assert np.abs(tri).max() < 1024
        got = pt.queryTriangleDistance(state, tri)
        worst = float(got["distance"].max())
        print("%s: the scene lies within %.3e of the triangle at its time of impact" % (name, worst))
        assert (got["distance"] >= 0).all() and worst <= CONTACT_BOUND, (name, worst)


def test_querytrianglecast_numpy_path_and_contacts(scenes, references):
    state, obj = scenes("box")
    s, ref = references("aimed")
    got = pt.queryTriangleCast(state, s)
    assert got["t"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32 and got["feature"].dtype == np.float32
    packed = np.concatenate([got["t"].view(np.uint32)[:, None], got["prim"][:, None], got["feature"].view(np.uint32)[:, None], got["query_triangle"][:, None],
                             got["point"].view(np.uint32), got["material"][:, None]], axis=1)
    assert np.array_equal(packed, ref)
    # triangles and directions with one tmax
    same = s.copy(); same[:, 3] = F(0.75)
    want = _reference(obj, same)
    for tris in (tc.triangles_of(s), tc.triangles_of(s).reshape(-1, 3, 4)[:, :, :3], tc.triangles_of(s).reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9).tolist()):
        got2 = pt.queryTriangleCast(state, tris, s[:, 12:15], tmax=0.75)
        assert np.array_equal(got2["prim"], want[:, 1]) and np.array_equal(got2["t"].view(np.uint32), want[:, 0])
    assert np.array_equal(pt.queryTriangleCast(state, same, any_hit=True), tc.blocked_of(want).view(np.bool_))
    one = s.copy(); one[:, 12:15] = s[0, 12:15]
    assert np.array_equal(pt.queryTriangleCast(state, tc.triangles_of(s), s[0, 12:15])["prim"], _reference(obj, one)[:, 1])
    # castContacts: unit normals that face against d and are perpendicular to the features that met
    normal, start = pt.castContacts(got, s, obj.getVerticesFloat(), obj.getIndexBuffer())
    hit = got["t"] >= 0
    assert hit.all() and np.array_equal(start, got["feature"] == 15) and 0.02 <= start.mean() <= 0.5
    moving = hit & ~start
    nn = normal[moving].astype(np.float64)
    assert np.abs(np.sqrt((nn * nn).sum(axis=1)) - 1.0).max() <= 1e-6
    assert ((nn * s[moving, 12:15]).sum(axis=1) <= 0).all()
    v0, e1, e2 = nr.records_of_scene(obj.getVerticesFloat(), obj.getIndexBuffer())
    face = moving & (got["feature"] <= 2)
    n_scene = np.cross(e1[got["prim"][face]].astype(np.float64), e2[got["prim"][face]])
    n_scene /= np.sqrt((n_scene * n_scene).sum(axis=1, keepdims=True))
    assert face.sum() >= 100 and np.abs(np.abs((normal[face] * n_scene).sum(axis=1)) - 1.0).max() <= 1e-6
    assert not normal[start].any()
    miss = pt.queryTriangleCast(state, references("outside")[0][:8])
    assert np.isnan(pt.castContacts(miss, references("outside")[0][:8], obj.getVerticesFloat(), obj.getIndexBuffer())[0][miss["t"] < 0]).all()
    with pytest.raises(pt.PathTracerError, match="expected"):
        pt.queryTriangleCast(state, np.zeros((4, 8), np.float32))
    with pytest.raises(pt.PathTracerError, match="tmax"):
        pt.queryTriangleCast(state, np.zeros((4, 9), np.float32), np.zeros(3), tmax=-1.0)
    assert pt.queryTriangleCast(state, np.zeros((0, 16), np.float32))["t"].shape == (0,)


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    s, ref = references("links")
    L = _L()
    seen = {}
    real, real_any = L.pt_query_triangle_cast, L.pt_query_triangle_cast_any
    monkeypatch.setattr(L, "pt_query_triangle_cast", lambda ctx, p, n, out: seen.update(call=(p, n, out)) or real(ctx, p, n, out))
    monkeypatch.setattr(L, "pt_query_triangle_cast_any", lambda ctx, p, n, out: seen.update(any=(p, n, out)) or real_any(ctx, p, n, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(s.copy()).to(dev)
    got = pt.queryTriangleCast(state, x)
    assert seen["call"][0] == x.data_ptr() and seen["call"][1] == s.shape[0]
    assert all(v.device == dev for v in got.values())
    assert seen["call"][2] == got["t"].data_ptr()                   # the columns are views of the tensor the library wrote
    assert got["t"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32
    assert got["point"].shape == (s.shape[0], 3)
    cols = {"t": ref[:, 0], "prim": ref[:, 1], "feature": ref[:, 2], "query_triangle": ref[:, 3], "material": ref[:, 7]}
    for k, want in cols.items():
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), k
    assert np.array_equal(got["point"].cpu().numpy().view(np.uint32), ref[:, 4:7])
    blocked = pt.queryTriangleCast(state, x, any_hit=True)
    assert seen["any"][0] == x.data_ptr() and seen["any"][2] == blocked.data_ptr() and blocked.dtype == torch.bool and blocked.device == dev
    assert np.array_equal(blocked.cpu().numpy(), tc.blocked_of(ref).view(np.bool_))
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.queryTriangleCast(state, y)
    assert seen["call"][0] == y.data_ptr() and torch.equal(again["prim"], got["prim"]) and torch.equal(again["t"], got["t"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :7].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.queryTriangleCast(state, bad)
    assert pt.queryTriangleCast(state, x[:0])["t"].shape == (0,)
