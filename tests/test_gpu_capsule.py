"""Swept-capsule casts on the GPU: pt_query_capsule_cast against tests/capsule_ref.py's brute force (the whole record, bits) and
pt_query_capsule_cast_any against the records, on every cast set and size, both Cornell fixtures and both node formats, the counting
twin in both modes, the output's bounds, the point set against pt_query_sweep, the scene's memory and the render state, vertex updates,
the refusals, torch tensors, capsuleContacts and acgpt_main --capsule-cast."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import capsule_ref as cr
import nearest_ref as nr
import sweep_ref as sw
from test_capsule_host import AXIS_MARGIN, SPHERE_CONTACT_MEASURED

F = np.float32
pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
GUARD = 64                                         # bytes of 0xCD kept behind every output


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


def _camera(state):
    p = state.params
    return p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple()


class _DeviceCasts:
    """casts in a device buffer, with buffers for the records, the bytes and the visit counts and a guard behind each; the C ABI
    called as a C caller would"""
    def __init__(self, state, casts):
        self.state, self.n = state, casts.shape[0]
        self.casts = np.ascontiguousarray(casts, np.float32)
        assert self.casts.shape == (self.n, 12)
        self.bufs = pt.pathtracer._device_buffers(state, 4, max(self.n * 48, 48) + GUARD)
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
        assert _L().pt_query_capsule_cast(self.state.context, self.bufs[0], self.n, self.bufs[1]) == 0, _err(self.state)
        return self._read(self.bufs[1], self.n * 32).view(np.uint32).reshape(self.n, 8)

    def blocked(self, offset=0):
        self._arm(self.bufs[2], self.n + offset)
        assert _L().pt_query_capsule_cast_any(self.state.context, self.bufs[0], self.n, self.bufs[2] + offset) == 0, _err(self.state)
        raw = self._read(self.bufs[2], self.n + offset)
        assert (raw[:offset] == 0xCD).all()
        return raw[offset:]

    def visits(self, mode):
        self._arm(self.bufs[1], self.n * 32)
        self._arm(self.bufs[3], self.n * 8)
        assert _L().pt_debug_capsule_cast_visits(self.state.context, self.bufs[0], self.n, self.bufs[1], self.bufs[3], mode) == 0, _err(self.state)
        return (self._read(self.bufs[1], self.n * 32).view(np.uint32).reshape(self.n, 8).copy(), self._read(self.bufs[3], self.n * 8).view(np.uint32).reshape(self.n, 2).copy())

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
    return cr.capsule_records(casts, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices())


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
    """The two Cornell fixtures under the default variant (fp16 centre / half-extent nodes) and the first under an fp32-node variant,
    each set up once.  name -> (state, obj)"""
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
                made[name] = gpu_state_factory(BOX if name == "box" else DIFFUSE, width=97, height=61, max_depth=4, spp=8)
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
            c = cr.cast_set(name, obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state), obj.getMaterialIndices())
            ref = _reference(obj, c)
            c.setflags(write=False); ref.setflags(write=False)
            cache[name] = (c, ref)
        return cache[name]

    return get


def _reference_on(scenes, references, scene, name):
    """The box's reference on another fixture: the second Cornell fixture has the box's triangles under other materials, so only the
    last word of a record differs; the brute force runs once"""
    c, ref = references(name)
    if scene != "diffuse":
        return c, ref
    box, other = scenes("box")[1], scenes("diffuse")[1]
    assert np.array_equal(box.getVerticesFloat(), other.getVerticesFloat()) and np.array_equal(box.getIndexBuffer(), other.getIndexBuffer())
    out = ref.copy()
    hit = ref[:, 1] != 0xFFFFFFFF
    out[hit, 7] = np.asarray(other.getMaterialIndices(), np.uint32)[ref[hit, 1]] & cr.SHADE_MAT_MASK
    return c, out


def test_unchanged_hash_and_abi_version():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH
    assert _L().pt_abi_version() == 4


@pytest.mark.parametrize("name", cr.CAST_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_records_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    c, ref = _reference_on(scenes, references, scene, name)
    hit = ref[:, 1] != 0xFFFFFFFF
    # the set still does what it is there for, by the reference's own answers: a set that lost its hits must not pass vacuously
    assert hit.mean() >= 0.25 and np.unique(ref[hit, 1]).size >= 8, (name, hit.mean())
    if name in ("short", "outside", "zero_d", "bad"):
        assert (~hit).mean() >= 0.2, name
    before = pt.getBvhInfo(state).device_bytes
    for n in SIZES:
        rec, blocked = _query(state, c[:n])
        assert np.array_equal(rec, ref[:n]), (scene, name, n) + _diff(rec, ref[:n])
        assert np.array_equal(blocked, cr.blocked_of(ref[:n])), (scene, name, n, np.flatnonzero(blocked != cr.blocked_of(ref[:n]))[:8])
    assert pt.getBvhInfo(state).device_bytes == before
    if name == "bad":
        assert np.array_equal(ref[~cr.castable(c)], cr.miss_records(int((~cr.castable(c)).sum())))


def test_blocked_may_have_any_alignment(scenes, references):
    state, obj = scenes("box")
    c, ref = references("outside")
    d = _DeviceCasts(state, c[:257])
    try:
        for offset in (1, 2, 3, 7):
            assert np.array_equal(d.blocked(offset), cr.blocked_of(ref[:257])), offset
    finally:
        d.free()


def test_counting_twin_in_both_modes(scenes, references):
    """pt_debug_capsule_cast_visits: the same records with and without the plane axis, the plane axis never adds a node, no cast tests
    more triangles than the scene has, the boxes prune, and a cast whose swept capsule misses the scene box visits the root at most and
    tests nothing"""
    for scene in ("box", "fp32"):
        state, obj = scenes(scene)
        n_tris = len(obj.getIndexBuffer()) // 3
        for name in ("links", "upright", "grazing"):
            c, ref = references(name)
            d = _DeviceCasts(state, c[:257])
            try:
                rec0, vis0 = d.visits(0)
                rec1, vis1 = d.visits(1)
            finally:
                d.free()
            assert np.array_equal(rec0, ref[:257]), (scene, name) + _diff(rec0, ref[:257])
            assert np.array_equal(rec1, ref[:257]), (scene, name) + _diff(rec1, ref[:257])
            assert (vis0[:, 0] <= vis1[:, 0]).all() and (vis0[:, 1] <= vis1[:, 1]).all(), (scene, name)
            assert (vis1[:, 1] <= n_tris).all() and (vis1[:, 0] < n_tris).all() and (vis0[:, 0] >= 1).all()
            assert vis0[:, 1].mean() < n_tris / 4, (scene, name, vis0[:, 1].mean())
            if name == "links":
                assert vis0[:, 0].sum() < vis1[:, 0].sum(), (scene, vis0[:, 0].sum(), vis1[:, 0].sum())          # on long diagonal capsules the plane prunes
        lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
        ce = 0.5 * (lo + hi)
        r = F(20.0)
        # beside the box by more than the radius, running along it; towards it, but too short to reach; away from it; a long diagonal
        # capsule whose box holds the scene's and whose swept plane passes beside it
        away = np.array([[hi[0] + 3 * r + 50, ce[1], ce[2], r, hi[0] + 3 * r + 50, ce[1] + 40, ce[2], 10.0, 0.01, 1.0, 0.37, 0.0],
                         [hi[0] + 3 * r + 50, ce[1], ce[2], r, hi[0] + 3 * r + 90, ce[1], ce[2] + 30, 25.0, -1.0, 0.2, 0.1, 0.0],
                         [ce[0], hi[1] + 2 * r + 1, ce[2], r, ce[0] + 10, hi[1] + 2 * r + 31, ce[2], np.inf, 0.3, 1.0, -0.2, 0.0],
                         [lo[0] - 1500, ce[1], lo[2] - 100, r, lo[0] - 100, ce[1], lo[2] - 1500, np.inf, 0.0, 1.0, 0.0, 0.0]], np.float32)
        d = _DeviceCasts(state, away)
        try:
            rec, vis = d.visits(0)
            rec1, vis1 = d.visits(1)
        finally:
            d.free()
        assert np.array_equal(rec, cr.miss_records(4)) and np.array_equal(rec, _reference(obj, away)) and np.array_equal(rec1, rec)
        assert (vis[:, 0] <= 1).all() and (vis[:, 1] == 0).all(), vis
        L = _L()
        d = _DeviceCasts(state, away)
        try:
            assert L.pt_debug_capsule_cast_visits(state.context, d.bufs[0], 4, d.bufs[1], None, 0) != 0 and "null argument" in _err(state)
            assert L.pt_debug_capsule_cast_visits(state.context, d.bufs[0], 4, d.bufs[1], d.bufs[3], 2) != 0 and "mode" in _err(state)
        finally:
            d.free()


def test_two_calls_give_the_same_bits(scenes, references):
    state, obj = scenes("box")
    c, ref = references("aimed")
    d = _DeviceCasts(state, c[:257])
    try:
        a, b = d.cast().copy(), d.cast().copy()          # cast() checks the 0xCD guard behind record n
        x, y = d.blocked().copy(), d.blocked().copy()
    finally:
        d.free()
    assert np.array_equal(a, b) and np.array_equal(a, ref[:257]) and np.array_equal(x, y)


def test_the_point_set_equals_pt_query_sweep(scenes, references):
    """p1 = p0 on the device: t and prim are pt_query_sweep's, bit for bit, wherever neither call starts in contact"""
    state, obj = scenes("box")
    c, ref = references("point")
    sweeps = np.ascontiguousarray(np.concatenate([c[:, 0:3], c[:, 8:11], c[:, 3:4], c[:, 7:8]], axis=1))
    got = pt.querySweep(state, sweeps)
    rec = _query(state, c)[0]
    out = (got["t"] == 0) | (rec[:, 0].view(np.float32) == 0)
    assert out.mean() < 0.25 and (got["prim"][~out] != 0xFFFFFFFF).mean() >= 0.25
    assert np.array_equal(got["t"][~out].view(np.uint32), rec[~out, 0]) and np.array_equal(got["prim"][~out], rec[~out, 1])
    assert np.array_equal(got["t"] == 0, rec[:, 0].view(np.float32) == 0)


def test_queries_leave_the_scene_memory_and_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    c = cr.cast_set("links", obj.getVerticesFloat(), obj.getIndexBuffer())
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for st, o in ((state, ob), (twin, None)):
            st.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, st, 1)
        acc, fb, stats = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        rec, blocked = _query(state, c)
        got = pt.queryCapsuleCast(state, c)
        assert np.array_equal(got["prim"], rec[:, 1]) and np.array_equal(pt.queryCapsuleCast(state, c, any_hit=True), blocked.view(np.bool_))
        assert pt.getBvhInfo(state).device_bytes == before              # a default scene holds the fp16 nodes only, and stays so
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == stats
        assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH
        for st, o in ((state, ob), (twin, None)):
            st.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, st, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_after_update_vertices_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    casts = np.concatenate([cr.cast_set(name, verts0, idx)[:300] for name in ("aimed", "grazing", "upright", "links")])
    _query(state, casts)                                    # the queries have run on the scene before it changes
    fresh = []
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
        fresh.append(_fresh_state(state, moved))
        (rec, blk), (rec2, blk2) = _query(state, casts), _query(fresh[-1], casts)
        ref = _reference(moved, casts)
        assert np.array_equal(rec, rec2), _diff(rec, rec2)
        assert np.array_equal(rec, ref), _diff(rec, ref)
        assert np.array_equal(blk, blk2) and np.array_equal(blk, cr.blocked_of(ref))
        assert (ref != _reference(obj, casts)).any()         # the move shows in the answers
    finally:
        for s in fresh:
            pt.CleanAllTheThings(s)


def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    c, ref = references("aimed")
    L = _L()
    d = _DeviceCasts(state, c[:256])
    try:
        expected = d.cast().copy()
        p, o, b = d.bufs[0], d.bufs[1], d.bufs[2]
        refused = {
            "null casts": L.pt_query_capsule_cast(state.context, None, 256, o),
            "null hits": L.pt_query_capsule_cast(state.context, p, 256, None),
            "too many": L.pt_query_capsule_cast(state.context, p, 0x80000000, o),
            "the hits are the casts": L.pt_query_capsule_cast(state.context, p, 256, p),
            "the hits overlap the casts' end": L.pt_query_capsule_cast(state.context, p, 256, p + 255 * 48),
            "the casts lie inside the hits": L.pt_query_capsule_cast(state.context, o + 1024, 64, o),
            "casts not aligned": L.pt_query_capsule_cast(state.context, p + 4, 16, o),
            "hits not aligned": L.pt_query_capsule_cast(state.context, p, 16, o + 8),
            "null context": L.pt_query_capsule_cast(None, p, 256, o),
            "any: null casts": L.pt_query_capsule_cast_any(state.context, None, 256, b),
            "any: null blocked": L.pt_query_capsule_cast_any(state.context, p, 256, None),
            "any: too many": L.pt_query_capsule_cast_any(state.context, p, 0x80000000, b),
            "any: blocked inside the casts": L.pt_query_capsule_cast_any(state.context, p, 256, p + 100),
            "any: casts not aligned": L.pt_query_capsule_cast_any(state.context, p + 4, 16, b),
            "any: null context": L.pt_query_capsule_cast_any(None, p, 256, b),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_capsule_cast(state.context, None, 256, o) != 0 and _err(state).startswith("pt_query_capsule_cast: ")
        assert L.pt_query_capsule_cast(state.context, p, 0x80000000, o) != 0 and "too many casts" in _err(state)
        assert L.pt_query_capsule_cast(state.context, p, 256, p) != 0 and "overlaps" in _err(state)
        assert L.pt_query_capsule_cast(state.context, p + 4, 16, o) != 0 and "aligned" in _err(state)
        assert L.pt_query_capsule_cast_any(state.context, p, 256, None) != 0 and _err(state).startswith("pt_query_capsule_cast_any: ")
        # pt_query_sweep's order: a null pointer before the count, the count before the alignment, the alignment before the overlap
        assert L.pt_query_capsule_cast(state.context, None, 0x80000000, o) != 0 and "null argument" in _err(state)
        assert L.pt_query_capsule_cast(state.context, p + 4, 0x80000000, o) != 0 and "too many casts" in _err(state)
        assert L.pt_query_capsule_cast(state.context, p + 4, 16, p + 4) != 0 and "aligned" in _err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_capsule_cast(bare, p, 256, o) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_capsule_cast_any(bare, p, 256, b) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_capsule_cast(bare, None, 0, None) == 0                  # no casts: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_capsule_cast(state.context, None, 0, None) == 0 and L.pt_query_capsule_cast_any(state.context, None, 0, None) == 0
        assert np.array_equal(d.cast(), expected)                             # the next valid call
        assert np.array_equal(expected, ref[:256])
    finally:
        d.free()


def test_querycapsulecast_numpy_path_and_contacts(scenes, references):
    state, obj = scenes("box")
    c, ref = references("aimed")
    got = pt.queryCapsuleCast(state, c)
    assert got["t"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32
    packed = np.concatenate([got["t"].view(np.uint32)[:, None], got["prim"][:, None], got["s"].view(np.uint32)[:, None], got["feature"].view(np.uint32)[:, None],
                             got["point"].view(np.uint32), got["material"][:, None]], axis=1)
    assert np.array_equal(packed, ref)
    # p0, p1 and directions with one radius and one tmax
    same = c.copy(); same[:, 3] = F(7.5); same[:, 7] = F(3.0); same[:, 11] = 0.0
    got2 = pt.queryCapsuleCast(state, c[:, 0:3].tolist(), c[:, 4:7], c[:, 8:11], radius=7.5, tmax=3.0)
    want = _reference(obj, same)
    assert np.array_equal(got2["prim"], want[:, 1]) and np.array_equal(got2["t"].view(np.uint32), want[:, 0])
    assert np.array_equal(pt.queryCapsuleCast(state, same, any_hit=True), cr.blocked_of(want).view(np.bool_))
    # capsuleContacts: unit normals, and axis points at the radius from the contact point within the bound of the host test
    q0, q1, on_axis, normal, start = pt.capsuleContacts(got, c)
    hit = got["t"] >= 0
    assert hit.all() and np.array_equal(start, got["t"] == 0) and 0.05 <= start.mean() <= 0.5
    moving = hit & ~start
    assert np.abs(np.sqrt((normal[moving].astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 1e-6
    dist = np.sqrt(((on_axis[moving].astype(np.float64) - got["point"][moving]) ** 2).sum(axis=1))
    # the axis point and the contact point are fp32 values of ~550: each component within an ulp or two, 1e-4
    assert np.abs(dist - c[moving, 3]).max() <= SPHERE_CONTACT_MEASURED * AXIS_MARGIN + 4e-4, np.abs(dist - c[moving, 3]).max()
    assert np.isfinite(q0).all() and np.isfinite(q1).all()


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    c, ref = references("upright")
    L = _L()
    seen = {}
    real, real_any = L.pt_query_capsule_cast, L.pt_query_capsule_cast_any
    monkeypatch.setattr(L, "pt_query_capsule_cast", lambda ctx, p, n, out: seen.update(call=(p, n, out)) or real(ctx, p, n, out))
    monkeypatch.setattr(L, "pt_query_capsule_cast_any", lambda ctx, p, n, out: seen.update(any=(p, n, out)) or real_any(ctx, p, n, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(c.copy()).to(dev)
    got = pt.queryCapsuleCast(state, x)
    assert seen["call"][0] == x.data_ptr() and seen["call"][1] == c.shape[0]
    assert all(v.device == dev for v in got.values())
    assert seen["call"][2] == got["t"].data_ptr()                   # the columns are views of the tensor the library wrote
    assert got["t"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32
    assert got["point"].shape == (c.shape[0], 3)
    cols = {"t": ref[:, 0], "prim": ref[:, 1], "s": ref[:, 2], "feature": ref[:, 3], "material": ref[:, 7]}
    for k, want in cols.items():
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), k
    assert np.array_equal(got["point"].cpu().numpy().view(np.uint32), ref[:, 4:7])
    blocked = pt.queryCapsuleCast(state, x, any_hit=True)
    assert seen["any"][0] == x.data_ptr() and seen["any"][2] == blocked.data_ptr() and blocked.dtype == torch.bool and blocked.device == dev
    assert np.array_equal(blocked.cpu().numpy(), cr.blocked_of(ref).view(np.bool_))
    q0, q1, on_axis, normal, start = pt.capsuleContacts(got, x)
    assert q0.device == dev and normal.shape == (c.shape[0], 3) and torch.equal(start, got["t"] == 0)
    n0, n1, na, nn, ns = pt.capsuleContacts({k: v.cpu().numpy() for k, v in got.items()}, c)
    hit = (got["t"] > 0).cpu().numpy()
    assert np.abs(normal.cpu().numpy()[hit] - nn[hit]).max() <= 1e-5 and np.abs(on_axis.cpu().numpy()[hit] - na[hit]).max() <= 1e-3
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.queryCapsuleCast(state, y)
    assert seen["call"][0] == y.data_ptr() and torch.equal(again["prim"], got["prim"]) and torch.equal(again["t"], got["t"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :8].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.queryCapsuleCast(state, bad)
    assert pt.queryCapsuleCast(state, x[:0])["t"].shape == (0,)


def test_cli_capsule_cast_prints_what_querycapsulecast_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (F(0.5) * (lo + hi)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    # an upright capsule under the ceiling in front of the blocks straight down, without and with a tmax that ends in mid-air; a tilted
    # one from in front of the open side into the room; one beside the box, moving away from it
    up0, up1 = (c[0], hi[1] - F(140.0), lo[2] + F(60.0)), (c[0], hi[1] - F(100.0), lo[2] + F(60.0))
    queries = [up0 + up1 + (0.0, -1.0, 0.0, 10.0, None), (c[0], c[1], lo[2] - F(300.0), c[0] + F(30.0), c[1] + F(40.0), lo[2] - F(320.0), 0.25, 0.125, 2.0, 25.0, None),
               up0 + up1 + (0.0, -1.0, 0.0, 10.0, 5.0), (hi[0] + F(500.0), c[1], c[2], hi[0] + F(520.0), c[1] + F(50.0), c[2], 1.0, 0.0, 0.0, 10.0, None)]
    queries = [tuple(None if a is None else float(np.float32(a)) for a in q) for q in queries]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for q in queries:
        cmd += ["--capsule-cast", ",".join("%r" % a for a in q if a is not None)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"capsule_cast"')]
    assert len(lines) == len(queries)
    casts = np.array([q[0:3] + (q[9],) + q[3:6] + (np.inf if q[10] is None else q[10],) + q[6:9] + (0.0,) for q in queries], np.float32)
    got = pt.queryCapsuleCast(state, casts)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    assert got["prim"][0] != 0xFFFFFFFF and got["prim"][1] != 0xFFFFFFFF and got["prim"][2] == 0xFFFFFFFF and got["prim"][3] == 0xFFFFFFFF
    for i, line in enumerate(lines):
        assert np.array_equal(np.array(line["capsule_cast"], np.float32), np.array(queries[i][:10], np.float32))
        assert line["tmax"] == queries[i][10]
        if got["prim"][i] == 0xFFFFFFFF:
            assert line == {"capsule_cast": line["capsule_cast"], "tmax": line["tmax"], "hit": False}
            continue
        assert line["hit"] is True and line["triangle"] == int(got["prim"][i])
        assert np.float32(line["t"]) == got["t"][i]
        assert line["material"] == names[int(got["material"][i])]
        assert np.array_equal(np.array(line["point"], np.float32), got["point"][i])
        assert np.float32(line["s"]) == got["s"][i] and line["feature"] == int(got["feature"][i])
    for arg in ("1,2,3,4,5,6,7,8,9", "1,2,3,0,1,nan,1,0,0,1", "1,2,3,0,1,0,1,0,0,-1", "1,2,3,0,1,0,1,0,0,1,-2", "1,2,3,0,1,0,1,0,0,inf"):
        bad = subprocess.run([exe, "--obj", BOX, "--capsule-cast", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--capsule-cast" in bad.stderr, (arg, bad.returncode, bad.stderr)
