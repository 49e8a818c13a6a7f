"""Swept oriented-box casts on the GPU: pt_query_box_cast against tests/boxcast_ref.py's brute force (the whole record, bits) and
pt_query_box_cast_any against the records, on every cast set and size, both Cornell fixtures and both node formats, the counting twin
in both modes, the output's bounds, d = 0 against the oriented and the axis-aligned overlap queries, the scene's memory and the render
state, vertex updates, the refusals, torch tensors, boxCastContacts, poseBoxCasts and acgpt_main --box-cast."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import boxcast_ref as br
import nearest_ref as nr
import oriented_ref as ot

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


class _DeviceCasts:
    """casts in a device buffer, with buffers for the records, the bytes and the visit counts and a guard behind each; the C ABI
    called as a C caller would"""
    def __init__(self, state, casts):
        self.state, self.n = state, casts.shape[0]
        self.casts = np.ascontiguousarray(casts, np.float32)
        assert self.casts.shape == (self.n, 20)
        self.bufs = pt.pathtracer._device_buffers(state, 4, max(self.n * 80, 80) + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.casts.ctypes.data, self.casts.nbytes) == 0

    def _read(self, ptr, nbytes):
        raw = np.zeros(nbytes + GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, ptr, raw.nbytes) == 0
        assert (raw[nbytes:] == 0xCD).all(), "written past the end of the output"
        return raw[:nbytes]

    def _arm(self, ptr, nbytes):
        assert _L().pt_device_memset(self.state.context, ptr, 0xCD, nbytes + GUARD) == 0

    def cast(self):
        self._arm(self.bufs[1], self.n * 48)
        assert _L().pt_query_box_cast(self.state.context, self.bufs[0], self.n, self.bufs[1]) == 0, _err(self.state)
        return self._read(self.bufs[1], self.n * 48).view(np.uint32).reshape(self.n, 12)

    def blocked(self, offset=1):
        """the bytes, written at an odd address unless told otherwise"""
        self._arm(self.bufs[2], self.n + offset)
        assert _L().pt_query_box_cast_any(self.state.context, self.bufs[0], self.n, self.bufs[2] + offset) == 0, _err(self.state)
        raw = self._read(self.bufs[2], self.n + offset)
        assert (raw[:offset] == 0xCD).all()
        return raw[offset:]

    def visits(self, mode):
        self._arm(self.bufs[1], self.n * 48)
        self._arm(self.bufs[3], self.n * 8)
        assert _L().pt_debug_box_cast_visits(self.state.context, self.bufs[0], self.n, self.bufs[1], self.bufs[3], mode) == 0, _err(self.state)
        return (self._read(self.bufs[1], self.n * 48).view(np.uint32).reshape(self.n, 12).copy(), self._read(self.bufs[3], self.n * 8).view(np.uint32).reshape(self.n, 2).copy())

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
    return br.box_records(casts, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices())


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
            c = br.cast_set(name, obj.getVerticesFloat(), obj.getIndexBuffer(), None, obj.getMaterialIndices())
            ref = _reference(obj, c)
            c.setflags(write=False); ref.setflags(write=False)
            cache[name] = (c, ref)
        return cache[name]

    return get


def _reference_on(scenes, references, scene, name):
    """The box's reference on another fixture: the second Cornell fixture has the box's triangles under other materials, so only the
    material word of a record differs; the brute force runs once"""
    c, ref = references(name)
    if scene != "diffuse":
        return c, ref
    box, other = scenes("box")[1], scenes("diffuse")[1]
    assert np.array_equal(box.getVerticesFloat(), other.getVerticesFloat()) and np.array_equal(box.getIndexBuffer(), other.getIndexBuffer())
    out = ref.copy()
    hit = ref[:, 1] != 0xFFFFFFFF
    out[hit, 3] = np.asarray(other.getMaterialIndices(), np.uint32)[ref[hit, 1]] & br.SHADE_MAT_MASK
    return c, out


def test_unchanged_hash_and_abi_version():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH
    assert _L().pt_abi_version() == 4


@pytest.mark.parametrize("name", br.CAST_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_records_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    c, ref = _reference_on(scenes, references, scene, name)
    hit = ref[:, 1] != 0xFFFFFFFF
    # the set still does what it is there for, by the reference's own answers: a set that lost its hits must not pass vacuously
    assert hit.mean() >= 0.25 and np.unique(ref[hit, 1]).size >= 8, (name, hit.mean())
    if name in ("short", "outside", "zero_d", "bad", "tolerance"):
        assert (~hit).mean() >= 0.2, name
    before = pt.getBvhInfo(state).device_bytes
    for n in SIZES:
        rec, blocked = _query(state, c[:n])                  # the bytes land at an odd address
        assert np.array_equal(rec, ref[:n]), (scene, name, n) + _diff(rec, ref[:n])
        assert np.array_equal(blocked, br.blocked_of(ref[:n])), (scene, name, n, np.flatnonzero(blocked != br.blocked_of(ref[:n]))[:8])
    assert pt.getBvhInfo(state).device_bytes == before
    if name == "bad":
        assert np.array_equal(ref[~br.castable(c)], br.miss_records(int((~br.castable(c)).sum())))


def test_blocked_may_have_any_alignment(scenes, references):
    state, obj = scenes("box")
    c, ref = references("outside")
    d = _DeviceCasts(state, c[:257])
    try:
        for offset in (0, 1, 2, 3, 7):
            assert np.array_equal(d.blocked(offset), br.blocked_of(ref[:257])), offset
    finally:
        d.free()


def test_zero_d_is_the_oriented_overlap_query(scenes, references):
    """d = 0: the byte is pt_query_overlap_oriented_any's on the first sixteen floats, byte for byte, and t == 0 wherever it is set"""
    state, obj = scenes("box")
    c, ref = references("zero_d")
    rec, blocked = _query(state, c)
    want = pt.queryOverlapOrientedAny(state, np.ascontiguousarray(c[:, :16]))
    assert np.array_equal(blocked.view(np.bool_), np.asarray(want, np.bool_))
    assert np.array_equal(rec[:, 0].view(np.float32) == 0, np.asarray(want, np.bool_)) and 0.2 <= np.mean(want) <= 0.8


def test_identity_with_zero_d_is_the_box_overlap_query(scenes, references):
    """the exact identity and d = 0: the byte is pt_query_overlap_any's on {c, h}"""
    state, obj = scenes("box")
    c = references("identity")[0].copy()
    c[:, 16:19] = 0.0
    aabbs = np.zeros((c.shape[0], 8), np.float32)
    aabbs[:, 0:3], aabbs[:, 3:6] = c[:, [3, 7, 11]], c[:, 12:15]
    want = np.asarray(pt.queryOverlapAny(state, aabbs), np.bool_)
    assert np.array_equal(_query(state, c)[1].view(np.bool_), want) and 0.1 <= want.mean() <= 0.9


def test_counting_twin_in_both_modes(scenes, references):
    """pt_debug_box_cast_visits: the same records with the six extra axes and on the slab alone, the extra axes never add a node, no
    cast tests more triangles than the scene has, the boxes prune, and a cast whose swept box misses the scene box visits the root at
    most and tests nothing"""
    for scene in ("box", "fp32"):
        state, obj = scenes(scene)
        n_tris = len(obj.getIndexBuffer()) // 3
        for name in ("links", "cells", "grazing"):
            c, ref = references(name)
            d = _DeviceCasts(state, c[:257])
            try:
                rec0, vis0 = d.visits(0)
                rec1, vis1 = d.visits(1)
                product = d.cast().copy()
            finally:
                d.free()
            assert np.array_equal(rec0, ref[:257]), (scene, name) + _diff(rec0, ref[:257])
            assert np.array_equal(rec1, ref[:257]), (scene, name) + _diff(rec1, ref[:257])
            assert np.array_equal(product, ref[:257])
            assert (vis0[:, 0] <= vis1[:, 0]).all() and (vis0[:, 1] <= vis1[:, 1]).all(), (scene, name)
            assert (vis1[:, 1] <= n_tris).all() and (vis1[:, 0] < n_tris).all() and (vis0[:, 0] >= 1).all()
            assert vis0[:, 1].mean() < n_tris / 4, (scene, name, vis0[:, 1].mean())
            if name == "links":
                assert vis0[:, 0].sum() < vis1[:, 0].sum(), (scene, vis0[:, 0].sum(), vis1[:, 0].sum())          # on long thin boxes the extra axes prune
        lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
        ce = 0.5 * (lo + hi)
        # beside the box, running along it; towards it, but too short to reach; away from it; a long diagonal box whose world box holds
        # the scene's and which passes beside it
        away = np.concatenate([
            br.pack(ot.as_oboxes([(hi[0] + 120, ce[1], ce[2])], [(20, 30, 40)], ot.rotations(np.random.default_rng(1), 1)), [(0.01, 1.0, 0.37)], np.inf),
            br.pack(ot.as_oboxes([(hi[0] + 200, ce[1], ce[2])], [(20, 30, 40)], ot.rotations(np.random.default_rng(2), 1)), [(-1.0, 0.2, 0.1)], 25.0),
            br.pack(ot.as_oboxes([(ce[0], hi[1] + 100, ce[2])], [(20, 30, 40)], ot.rotations(np.random.default_rng(3), 1)), [(0.3, 1.0, -0.2)], np.inf),
            br.pack(ot.as_oboxes([(lo[0] - 800, ce[1], lo[2] - 800)], [(1000, 5, 5)], ot.turns_about(np.array([1]), np.array([np.pi / 4]))), [(0.0, 1.0, 0.0)], np.inf)])
        d = _DeviceCasts(state, away)
        try:
            rec, vis = d.visits(0)
            rec1, vis1 = d.visits(1)
        finally:
            d.free()
        assert np.array_equal(rec, br.miss_records(4)) and np.array_equal(rec, _reference(obj, away)) and np.array_equal(rec1, rec)
        assert (vis[:, 0] <= 1).all() and (vis[:, 1] == 0).all(), vis
        L = _L()
        d = _DeviceCasts(state, away)
        try:
            assert L.pt_debug_box_cast_visits(state.context, d.bufs[0], 4, d.bufs[1], None, 0) != 0 and "null argument" in _err(state)
            assert L.pt_debug_box_cast_visits(state.context, d.bufs[0], 4, d.bufs[1], d.bufs[3], 2) != 0 and "mode" in _err(state)
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


def test_queries_leave_the_scene_memory_and_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    c = br.cast_set("links", obj.getVerticesFloat(), obj.getIndexBuffer())
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for st, o in ((state, ob), (twin, None)):
            st.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, st, 1)
        acc, fb, stats = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        rec, blocked = _query(state, c)
        got = pt.queryBoxCast(state, c)
        assert np.array_equal(got["prim"], rec[:, 1]) and np.array_equal(pt.queryBoxCast(state, c, any_hit=True), blocked.view(np.bool_))
        assert pt.getBvhInfo(state).device_bytes == before              # a default scene holds the fp16 nodes only, and stays so
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == stats
        assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH and _L().pt_abi_version() == 4
        for st, o in ((state, ob), (twin, None)):
            st.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, st, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_after_update_vertices_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    casts = np.concatenate([br.cast_set(name, verts0, idx)[:300] for name in ("aimed", "grazing", "cells", "links")])
    _query(state, casts)                                    # the queries have run on the scene before it changes
    fresh = []
    try:
        # a refit: the blocks' and the other inner pieces' vertices (everything strictly inside the room) move
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
        assert np.array_equal(blk, blk2) and np.array_equal(blk, br.blocked_of(ref))
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
            "null casts": L.pt_query_box_cast(state.context, None, 256, o),
            "null hits": L.pt_query_box_cast(state.context, p, 256, None),
            "too many": L.pt_query_box_cast(state.context, p, 0x80000000, o),
            "the hits are the casts": L.pt_query_box_cast(state.context, p, 256, p),
            "the hits overlap the casts' end": L.pt_query_box_cast(state.context, p, 256, p + 255 * 80),
            "the casts lie inside the hits": L.pt_query_box_cast(state.context, o + 1024, 64, o),
            "casts not aligned": L.pt_query_box_cast(state.context, p + 4, 16, o),
            "hits not aligned": L.pt_query_box_cast(state.context, p, 16, o + 8),
            "null context": L.pt_query_box_cast(None, p, 256, o),
            "any: null casts": L.pt_query_box_cast_any(state.context, None, 256, b),
            "any: null blocked": L.pt_query_box_cast_any(state.context, p, 256, None),
            "any: too many": L.pt_query_box_cast_any(state.context, p, 0x80000000, b),
            "any: blocked inside the casts": L.pt_query_box_cast_any(state.context, p, 256, p + 100),
            "any: casts not aligned": L.pt_query_box_cast_any(state.context, p + 4, 16, b),
            "any: null context": L.pt_query_box_cast_any(None, p, 256, b),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_box_cast(state.context, None, 256, o) != 0 and _err(state).startswith("pt_query_box_cast: ")
        assert L.pt_query_box_cast(state.context, p, 0x80000000, o) != 0 and "too many casts" in _err(state)
        assert L.pt_query_box_cast(state.context, p, 256, p) != 0 and "overlaps" in _err(state)
        assert L.pt_query_box_cast(state.context, p + 4, 16, o) != 0 and "aligned" in _err(state)
        assert L.pt_query_box_cast_any(state.context, p, 256, None) != 0 and _err(state).startswith("pt_query_box_cast_any: ")
        # pt_query_capsule_cast's order: a null pointer before the count, the count before the alignment, the alignment before the overlap
        assert L.pt_query_box_cast(state.context, None, 0x80000000, o) != 0 and "null argument" in _err(state)
        assert L.pt_query_box_cast(state.context, p + 4, 0x80000000, o) != 0 and "too many casts" in _err(state)
        assert L.pt_query_box_cast(state.context, p + 4, 16, p + 4) != 0 and "aligned" in _err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_box_cast(bare, p, 256, o) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_box_cast_any(bare, p, 256, b) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_box_cast(bare, None, 0, None) == 0                  # no casts: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_box_cast(state.context, None, 0, None) == 0 and L.pt_query_box_cast_any(state.context, None, 0, None) == 0
        assert np.array_equal(d.cast(), expected)                             # the next valid call
        assert np.array_equal(expected, ref[:256])
    finally:
        d.free()


def test_queryboxcast_numpy_path_and_contacts(scenes, references):
    state, obj = scenes("box")
    c, ref = references("aimed")
    got = pt.queryBoxCast(state, c)
    assert got["t"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32
    col = br.columns(ref)
    for k in ("t", "feature", "normal", "point"):
        assert np.array_equal(got[k].view(np.uint32), col[k].view(np.uint32)), k
    assert np.array_equal(got["prim"], col["prim"]) and np.array_equal(got["material"], col["material"])
    # oriented boxes and directions with one tmax; one direction for all
    same = c.copy(); same[:, 19] = F(3.0)
    got2 = pt.queryBoxCast(state, c[:, :16], c[:, 16:19].tolist(), tmax=3.0)
    want = _reference(obj, same)
    assert np.array_equal(got2["prim"], want[:, 1]) and np.array_equal(got2["t"].view(np.uint32), want[:, 0])
    assert np.array_equal(pt.queryBoxCast(state, same, any_hit=True), br.blocked_of(want).view(np.bool_))
    down = c.copy(); down[:, 16:19] = (0.0, -1.0, 0.0); down[:, 19] = np.inf
    assert np.array_equal(pt.queryBoxCast(state, c[:, :16], (0, -1, 0))["t"].view(np.uint32), _reference(obj, down)[:, 0])
    # boxCastContacts: the centre at impact, unit normals against the motion, the point on the box within the host test's bar
    centre, normal, point, start, slide = pt.boxCastContacts(got, c)
    hit = got["t"] >= 0
    assert hit.all() and np.array_equal(start, got["t"] == 0) and 0.05 <= start.mean() <= 0.5
    moving = hit & ~start
    assert np.abs(np.sqrt((normal[moving].astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 1e-6
    assert ((slide[moving].astype(np.float64) * normal[moving]).sum(axis=1) >= -1e-3).all() and np.isfinite(centre).all()
    from test_boxcast_host import FRAME_MARGIN, SPHERE_CONTACT_MEASURED
    assert br.obb_distance_f64(c[moving], got["t"][moving], point[moving]).max() <= SPHERE_CONTACT_MEASURED * FRAME_MARGIN


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    c, ref = references("cells")
    L = _L()
    seen = {}
    real, real_any = L.pt_query_box_cast, L.pt_query_box_cast_any
    monkeypatch.setattr(L, "pt_query_box_cast", lambda ctx, p, n, out: seen.update(call=(p, n, out)) or real(ctx, p, n, out))
    monkeypatch.setattr(L, "pt_query_box_cast_any", lambda ctx, p, n, out: seen.update(any=(p, n, out)) or real_any(ctx, p, n, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(c.copy()).to(dev)
    got = pt.queryBoxCast(state, x)
    assert seen["call"][0] == x.data_ptr() and seen["call"][1] == c.shape[0]
    assert all(v.device == dev for v in got.values())
    assert seen["call"][2] == got["t"].data_ptr()                   # the columns are views of the tensor the library wrote
    assert got["t"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32
    assert got["point"].shape == (c.shape[0], 3) and got["normal"].shape == (c.shape[0], 3)
    cols = {"t": ref[:, 0], "prim": ref[:, 1], "feature": ref[:, 2], "material": ref[:, 3]}
    for k, want in cols.items():
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), k
    assert np.array_equal(got["normal"].cpu().numpy().view(np.uint32), ref[:, 4:7]) and np.array_equal(got["point"].cpu().numpy().view(np.uint32), ref[:, 8:11])
    blocked = pt.queryBoxCast(state, x, any_hit=True)
    assert seen["any"][0] == x.data_ptr() and seen["any"][2] == blocked.data_ptr() and blocked.dtype == torch.bool and blocked.device == dev
    assert np.array_equal(blocked.cpu().numpy(), br.blocked_of(ref).view(np.bool_))
    centre, normal, point, start, slide = pt.boxCastContacts(got, x)
    assert centre.device == dev and normal.shape == (c.shape[0], 3) and torch.equal(start, got["t"] == 0)
    n_c, n_n, n_p, n_s, n_sl = pt.boxCastContacts({k: v.cpu().numpy() for k, v in got.items()}, c)
    hit = (got["t"] > 0).cpu().numpy()
    assert np.abs(centre.cpu().numpy()[hit] - n_c[hit]).max() <= 1e-3 and np.abs(slide.cpu().numpy()[hit] - n_sl[hit]).max() <= 1e-3
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.queryBoxCast(state, y)
    assert seen["call"][0] == y.data_ptr() and torch.equal(again["prim"], got["prim"]) and torch.equal(again["t"], got["t"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :16].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.queryBoxCast(state, bad)
    assert pt.queryBoxCast(state, x[:0])["t"].shape == (0,)


def test_pose_box_casts_assemble_the_records(scenes):
    """poseBoxCasts: pt_pose_boxes' records (oriented_ref.pose_boxes) with the motions behind them, and the casts they answer"""
    state, obj = scenes("box")
    rng = np.random.default_rng(4101)
    P = 300
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    poses = np.zeros((P, 3, 4), np.float32)
    poses[:, :, :3] = ot.rotations(rng, P)
    poses[:, :, 3] = lo + (0.2 + 0.6 * rng.random((P, 3))) * (hi - lo)
    poses = poses.reshape(P, 12)
    blo, bhi = (-20.0, -5.0, -8.0), (30.0, 9.0, 4.0)
    motions = np.concatenate([rng.normal(size=(P, 3)) * 50.0, rng.uniform(0.5, 3.0, (P, 1))], axis=1).astype(np.float32)
    casts = pt.poseBoxCasts(state, poses, (blo, bhi), motions)
    want = np.concatenate([ot.pose_boxes(poses, pt.pathtracer._local_box("test", blo, bhi)), motions], axis=1)
    assert casts.dtype == np.float32 and casts.shape == (P, 20) and np.array_equal(casts.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(pt.poseBoxCasts(state, poses, (blo, bhi), motions[0, :3])[:, 16:], np.broadcast_to(np.append(motions[0, :3], np.inf).astype(np.float32), (P, 4)))
    got = pt.queryBoxCast(state, casts)
    ref = _reference(obj, want)
    assert np.array_equal(got["t"].view(np.uint32), ref[:, 0]) and np.array_equal(got["prim"], ref[:, 1]) and 0.2 <= (got["t"] >= 0).mean()
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        tc_ = pt.poseBoxCasts(state, torch.from_numpy(poses).to(dev), (blo, bhi), torch.from_numpy(motions).to(dev))
        assert tc_.device == dev and tc_.is_contiguous() and np.array_equal(tc_.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(pt.queryBoxCast(state, tc_)["t"].cpu().numpy().view(np.uint32), ref[:, 0])


def test_cli_box_cast_prints_what_queryboxcast_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (F(0.5) * (lo + hi)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    # cx,cy,cz,hx,hy,hz,qw,qx,qy,qz,dx,dy,dz[,tmax]: an upright box under the ceiling in front of the blocks straight down, without and
    # with a tmax that ends in mid-air; a turned one from in front of the open side into the room; one beside the room, moving away
    up = (c[0], hi[1] - F(120.0), lo[2] + F(60.0), 10.0, 20.0, 5.0, 1.0, 0.0, 0.0, 0.0)
    queries = [up + (0.0, -1.0, 0.0, None), (c[0], c[1], lo[2] - F(300.0), 30.0, 10.0, 20.0, 0.5, 0.5, 0.5, 0.5, 0.25, 0.125, 2.0, None),
               up + (0.0, -1.0, 0.0, 5.0), (hi[0] + F(500.0), c[1], c[2], 10.0, 10.0, 10.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, None)]
    queries = [tuple(None if a is None else float(np.float32(a)) for a in q) for q in queries]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for q in queries:
        cmd += ["--box-cast", ",".join("%r" % a for a in q if a is not None)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"box_cast"')]
    assert len(lines) == len(queries)

    def rotation(q):          # the unit quaternion's matrix, in float32 operation for operation as the app forms it
        w, x, y, z = (F(a) for a in q)
        two = F(2.0)
        return np.array([[F(1.0) - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                         [two * (x * y + z * w), F(1.0) - two * (x * x + z * z), two * (y * z - x * w)],
                         [two * (x * z - y * w), two * (y * z + x * w), F(1.0) - two * (x * x + y * y)]], np.float32)
    casts = np.concatenate([br.pack(ot.as_oboxes([q[0:3]], [q[3:6]], rotation(q[6:10])), [q[10:13]], np.inf if q[13] is None else q[13]) for q in queries])
    got = pt.queryBoxCast(state, casts)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    assert got["prim"][0] != 0xFFFFFFFF and got["prim"][1] != 0xFFFFFFFF and got["prim"][2] == 0xFFFFFFFF and got["prim"][3] == 0xFFFFFFFF
    for i, line in enumerate(lines):
        assert np.array_equal(np.array(line["box_cast"], np.float32), np.array(queries[i][:13], np.float32))
        assert line["tmax"] == queries[i][13]
        if got["prim"][i] == 0xFFFFFFFF:
            assert line == {"box_cast": line["box_cast"], "tmax": line["tmax"], "hit": False}
            continue
        assert line["hit"] is True and line["triangle"] == int(got["prim"][i])
        assert np.float32(line["t"]) == got["t"][i] and line["feature"] == int(got["feature"][i])
        assert line["material"] == names[int(got["material"][i])]
        assert np.array_equal(np.array(line["point"], np.float32), got["point"][i]) and np.array_equal(np.array(line["normal"], np.float32), got["normal"][i])
    for arg in ("1,2,3,4,5,6,7,8,9", "1,2,3,1,1,nan,1,0,0,0,1,0,0", "1,2,3,1,1,-1,1,0,0,0,1,0,0", "1,2,3,1,1,1,0,0,0,0,1,0,0", "1,2,3,1,1,1,1,0,0,0,1,0,0,-2", "1,2,3,1,1,1,1,0,0,0,inf,0,0"):
        bad = subprocess.run([exe, "--obj", BOX, "--box-cast", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--box-cast" in bad.stderr, (arg, bad.returncode, bad.stderr)
