"""Swept-sphere casts on the GPU: pt_query_sweep against tests/sweep_ref.py's brute force (the whole record, bits) and
pt_query_sweep_any against the records, on every sweep set and size, both node formats, the scenes of tests/query_scenes.py that break
walks, the counting twin, the output's bounds, the scene's memory and the render state, scene edits, the refusals, torch tensors,
sweepContacts and acgpt_main --sweep."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import nearest_ref as nr
import sweep_ref as sw
from test_sweep_host import CONTACT_BOUND

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


def _camera(state):
    p = state.params
    return p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple()


class _DeviceSweeps:
    """sweeps in a device buffer, with buffers for the records, the bytes and the visit counts and a guard behind each; the C ABI
    called as a C caller would"""
    def __init__(self, state, sweeps):
        self.state, self.n = state, sweeps.shape[0]
        self.sweeps = np.ascontiguousarray(sweeps, np.float32)
        assert self.sweeps.shape == (self.n, 8)
        self.bufs = pt.pathtracer._device_buffers(state, 4, max(self.n * 32, 32) + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.sweeps.ctypes.data, self.sweeps.nbytes) == 0

    def _read(self, ptr, nbytes):
        raw = np.zeros(nbytes + GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, ptr, raw.nbytes) == 0
        assert (raw[nbytes:] == 0xCD).all(), "written past the end of the output"
        return raw[:nbytes]

    def _arm(self, ptr, nbytes):
        assert _L().pt_device_memset(self.state.context, ptr, 0xCD, nbytes + GUARD) == 0

    def sweep(self):
        self._arm(self.bufs[1], self.n * 32)
        assert _L().pt_query_sweep(self.state.context, self.bufs[0], self.n, self.bufs[1]) == 0, _err(self.state)
        return self._read(self.bufs[1], self.n * 32).view(np.uint32).reshape(self.n, 8)

    def blocked(self, offset=0):
        self._arm(self.bufs[2], self.n + offset)
        assert _L().pt_query_sweep_any(self.state.context, self.bufs[0], self.n, self.bufs[2] + offset) == 0, _err(self.state)
        raw = self._read(self.bufs[2], self.n + offset)
        assert (raw[:offset] == 0xCD).all()
        return raw[offset:]

    def visits(self):
        self._arm(self.bufs[1], self.n * 32)
        self._arm(self.bufs[3], self.n * 8)
        assert _L().pt_debug_sweep_visits(self.state.context, self.bufs[0], self.n, self.bufs[1], self.bufs[3]) == 0, _err(self.state)
        return (self._read(self.bufs[1], self.n * 32).view(np.uint32).reshape(self.n, 8), self._read(self.bufs[3], self.n * 8).view(np.uint32).reshape(self.n, 2))

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _query(state, sweeps):
    """(records, blocked bytes) of the two calls"""
    d = _DeviceSweeps(state, sweeps)
    try:
        return d.sweep().copy(), d.blocked().copy()
    finally:
        d.free()


def _reference(obj, sweeps):
    return sw.sweep_records(sweeps, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices())


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
    """set -> (sweeps, records) of the box by the brute force on the whole set: computed once, shared, never written"""
    cache = {}

    def get(name):
        if name not in cache:
            state, obj = scenes("box")
            s = sw.sweep_set(name, obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state), obj.getMaterialIndices())
            ref = _reference(obj, s)
            s.setflags(write=False); ref.setflags(write=False)
            cache[name] = (s, ref)
        return cache[name]

    return get


def test_unchanged_hash_and_abi_version():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH
    assert _L().pt_abi_version() == 4


@pytest.mark.parametrize("name", sw.SWEEP_SETS)
@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_records_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    s, ref = references(name)
    hit = ref[:, 1] != 0xFFFFFFFF
    # the set still does what it is there for, by the reference's own answers: a set that lost its hits must not pass vacuously
    assert hit.mean() >= 0.25 and np.unique(ref[hit, 1]).size >= 8, (name, hit.mean())
    if name in ("short", "outside", "zero_d", "bad"):
        assert (~hit).mean() >= 0.2, name
    before = pt.getBvhInfo(state).device_bytes
    for n in SIZES:
        rec, blocked = _query(state, s[:n])
        assert np.array_equal(rec, ref[:n]), (scene, name, n) + _diff(rec, ref[:n])
        assert np.array_equal(blocked, sw.blocked_of(ref[:n])), (scene, name, n, np.flatnonzero(blocked != sw.blocked_of(ref[:n]))[:8])
    assert pt.getBvhInfo(state).device_bytes == before
    if name == "bad":
        assert np.array_equal(ref[~sw.castable(s)], sw.miss_records(int((~sw.castable(s)).sum())))


def test_blocked_may_have_any_alignment(scenes, references):
    state, obj = scenes("box")
    s, ref = references("outside")
    d = _DeviceSweeps(state, s[:257])
    try:
        for offset in (1, 2, 3, 7):
            assert np.array_equal(d.blocked(offset), sw.blocked_of(ref[:257])), offset
    finally:
        d.free()


def test_counting_twin(scenes, references):
    """pt_debug_sweep_visits: the same records, no sweep tests more triangles than the scene has, the boxes prune, and a sweep whose
    inflated line misses the scene box visits the root at most and tests nothing"""
    n_tris = None
    for scene in ("box", "fp32"):
        state, obj = scenes(scene)
        n_tris = len(obj.getIndexBuffer()) // 3
        for name in ("camera", "grazing"):
            s, ref = references(name)
            d = _DeviceSweeps(state, s[:257])
            try:
                rec, vis = d.visits()
            finally:
                d.free()
            assert np.array_equal(rec, ref[:257]), (scene, name) + _diff(rec, ref[:257])
            assert (vis[:, 1] <= n_tris).all() and (vis[:, 0] < n_tris).all() and (vis[:, 0] >= 1).all()
            assert vis[:, 1].mean() < n_tris / 4, (scene, name, vis[:, 1].mean())
        lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
        c = 0.5 * (lo + hi)
        r = F(20.0)
        # beside the box by more than the radius, running along it; towards it, but too short to reach; away from it
        away = np.array([[hi[0] + 3 * r + 50, c[1], c[2], 0.01, 1.0, 0.37, r, 10.0],
                         [hi[0] + 3 * r + 50, c[1], c[2], -1.0, 0.2, 0.1, r, 25.0],
                         [c[0], hi[1] + 2 * r + 1, c[2], 0.3, 1.0, -0.2, r, np.inf],
                         [c[0], c[1], lo[2] - 500.0, 0.1, 0.1, -1.0, 0.0, np.inf]], np.float32)
        d = _DeviceSweeps(state, away)
        try:
            rec, vis = d.visits()
        finally:
            d.free()
        assert np.array_equal(rec, sw.miss_records(4)) and np.array_equal(rec, _reference(obj, away))
        assert (vis[:, 0] <= 1).all() and (vis[:, 1] == 0).all(), vis
        L = _L()
        d = _DeviceSweeps(state, away)
        try:
            assert L.pt_debug_sweep_visits(state.context, d.bufs[0], 4, d.bufs[1], None) != 0 and "null argument" in _err(state)
        finally:
            d.free()


def test_two_calls_give_the_same_bits(scenes, references):
    state, obj = scenes("box")
    s, ref = references("aimed")
    d = _DeviceSweeps(state, s[:257])
    try:
        a, b = d.sweep().copy(), d.sweep().copy()          # sweep() checks the 0xCD guard behind record n
        x, y = d.blocked().copy(), d.blocked().copy()
    finally:
        d.free()
    assert np.array_equal(a, b) and np.array_equal(a, ref[:257]) and np.array_equal(x, y)


def test_queries_leave_the_scene_memory_and_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    s = sw.sweep_set("aimed", obj.getVerticesFloat(), obj.getIndexBuffer())
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for st, o in ((state, ob), (twin, None)):
            st.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, st, 1)
        acc, fb, stats = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        rec, blocked = _query(state, s)
        got = pt.querySweep(state, s)
        assert np.array_equal(got["prim"], rec[:, 1]) and np.array_equal(pt.querySweep(state, s, any_hit=True), blocked.view(np.bool_))
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
    sweeps = np.concatenate([sw.sweep_set(name, verts0, idx, _camera(state), obj.getMaterialIndices())[:400] for name in ("camera", "aimed", "grazing")])
    _query(state, sweeps)                                    # the queries have run on the scene before it changes
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
        (rec, blk), (rec2, blk2) = _query(state, sweeps), _query(fresh[-1], sweeps)
        ref = _reference(moved, sweeps)
        assert np.array_equal(rec, rec2), _diff(rec, rec2)
        assert np.array_equal(rec, ref), _diff(rec, ref)
        assert np.array_equal(blk, blk2) and np.array_equal(blk, sw.blocked_of(ref))
        assert (ref != _reference(obj, sweeps)).any()         # the move shows in the answers
        # 2. new material assignments on top: the ids rotate by one
        n_mats = obj.getNumMaterials()
        ids = ((np.asarray(obj.getMaterialIndices(), np.uint32) + 1) % n_mats).astype(np.uint32)
        pt.updateMaterials(state, material_ids=ids)
        moved._materialIndices = ids
        fresh.append(_fresh_state(state, moved))
        rec3, rec4 = _query(state, sweeps)[0], _query(fresh[-1], sweeps)[0]
        assert np.array_equal(rec3, rec4) and np.array_equal(rec3, _reference(moved, sweeps))
        found = rec[:, 1] != 0xFFFFFFFF
        assert np.array_equal(rec3[:, :7], rec[:, :7]) and (rec3[:, 7] != rec[:, 7])[found].all() and found.mean() >= 0.25
    finally:
        for s in fresh:
            pt.CleanAllTheThings(s)


def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    s, ref = references("aimed")
    L = _L()
    d = _DeviceSweeps(state, s[:256])
    try:
        expected = d.sweep().copy()
        p, o, b = d.bufs[0], d.bufs[1], d.bufs[2]
        refused = {
            "null sweeps": L.pt_query_sweep(state.context, None, 256, o),
            "null hits": L.pt_query_sweep(state.context, p, 256, None),
            "too many": L.pt_query_sweep(state.context, p, 0x80000000, o),
            "the hits are the sweeps": L.pt_query_sweep(state.context, p, 256, p),
            "the hits overlap the sweeps' end": L.pt_query_sweep(state.context, p, 256, p + 255 * 32),
            "the sweeps lie inside the hits": L.pt_query_sweep(state.context, o + 1024, 64, o),
            "sweeps not aligned": L.pt_query_sweep(state.context, p + 4, 16, o),
            "hits not aligned": L.pt_query_sweep(state.context, p, 16, o + 8),
            "null context": L.pt_query_sweep(None, p, 256, o),
            "any: null sweeps": L.pt_query_sweep_any(state.context, None, 256, b),
            "any: null blocked": L.pt_query_sweep_any(state.context, p, 256, None),
            "any: too many": L.pt_query_sweep_any(state.context, p, 0x80000000, b),
            "any: blocked inside the sweeps": L.pt_query_sweep_any(state.context, p, 256, p + 100),
            "any: sweeps not aligned": L.pt_query_sweep_any(state.context, p + 4, 16, b),
            "any: null context": L.pt_query_sweep_any(None, p, 256, b),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_sweep(state.context, None, 256, o) != 0 and _err(state).startswith("pt_query_sweep: ")
        assert L.pt_query_sweep(state.context, p, 0x80000000, o) != 0 and "too many sweeps" in _err(state)
        assert L.pt_query_sweep(state.context, p, 256, p) != 0 and "overlaps" in _err(state)
        assert L.pt_query_sweep(state.context, p + 4, 16, o) != 0 and "aligned" in _err(state)
        assert L.pt_query_sweep_any(state.context, p, 256, None) != 0 and _err(state).startswith("pt_query_sweep_any: ")
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_sweep(bare, p, 256, o) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_sweep_any(bare, p, 256, b) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_sweep(bare, None, 0, None) == 0                  # no sweeps: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_sweep(state.context, None, 0, None) == 0 and L.pt_query_sweep_any(state.context, None, 0, None) == 0
        assert np.array_equal(d.sweep(), expected)                             # the next valid call
        assert np.array_equal(expected, ref[:256])
    finally:
        d.free()


def test_querysweep_numpy_path_and_contacts(scenes, references):
    state, obj = scenes("box")
    s, ref = references("aimed")
    got = pt.querySweep(state, s)
    assert got["t"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32
    packed = np.concatenate([got["t"].view(np.uint32)[:, None], got["prim"][:, None], got["u"].view(np.uint32)[:, None], got["v"].view(np.uint32)[:, None],
                             got["point"].view(np.uint32), got["material"][:, None]], axis=1)
    assert np.array_equal(packed, ref)
    # origins and directions with one radius and one tmax
    same = s.copy(); same[:, 6] = F(7.5); same[:, 7] = F(3.0)
    got2 = pt.querySweep(state, s[:, 0:3].tolist(), s[:, 3:6], radius=7.5, tmax=3.0)
    want = _reference(obj, same)
    assert np.array_equal(got2["prim"], want[:, 1]) and np.array_equal(got2["t"].view(np.uint32), want[:, 0])
    assert np.array_equal(pt.querySweep(state, same, any_hit=True), sw.blocked_of(want).view(np.bool_))
    # sweepContacts: unit normals, and centres at distance r from the contact point within the bound of the host test
    centre, normal, start = pt.sweepContacts(got, s)
    hit = got["t"] >= 0
    assert hit.all() and np.array_equal(start, got["t"] == 0) and 0.05 <= start.mean() <= 0.5
    moving = hit & ~start
    assert np.abs(np.sqrt((normal[moving].astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 1e-6
    dist = np.sqrt(((centre[moving].astype(np.float64) - got["point"][moving]) ** 2).sum(axis=1))
    # the centre and the contact point are fp32 values of ~550: each component within half an ulp, 3e-5
    assert np.abs(dist - s[moving, 6]).max() <= CONTACT_BOUND + 2e-4, np.abs(dist - s[moving, 6]).max()
    assert (dist[...] >= 0).all() and np.isfinite(centre).all()


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    s, ref = references("camera")
    L = _L()
    seen = {}
    real, real_any = L.pt_query_sweep, L.pt_query_sweep_any
    monkeypatch.setattr(L, "pt_query_sweep", lambda ctx, p, n, out: seen.update(call=(p, n, out)) or real(ctx, p, n, out))
    monkeypatch.setattr(L, "pt_query_sweep_any", lambda ctx, p, n, out: seen.update(any=(p, n, out)) or real_any(ctx, p, n, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(s.copy()).to(dev)
    got = pt.querySweep(state, x)
    assert seen["call"][0] == x.data_ptr() and seen["call"][1] == s.shape[0]
    assert all(v.device == dev for v in got.values())
    assert seen["call"][2] == got["t"].data_ptr()                   # the columns are views of the tensor the library wrote
    assert got["t"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32
    assert got["point"].shape == (s.shape[0], 3)
    cols = {"t": ref[:, 0], "prim": ref[:, 1], "u": ref[:, 2], "v": ref[:, 3], "material": ref[:, 7]}
    for k, want in cols.items():
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), k
    assert np.array_equal(got["point"].cpu().numpy().view(np.uint32), ref[:, 4:7])
    blocked = pt.querySweep(state, x, any_hit=True)
    assert seen["any"][0] == x.data_ptr() and seen["any"][2] == blocked.data_ptr() and blocked.dtype == torch.bool and blocked.device == dev
    assert np.array_equal(blocked.cpu().numpy(), sw.blocked_of(ref).view(np.bool_))
    centre, normal, start = pt.sweepContacts(got, x)
    assert centre.device == dev and normal.shape == (s.shape[0], 3) and torch.equal(start, got["t"] == 0)
    hit = (got["t"] > 0).cpu().numpy()
    assert np.abs(np.sqrt((normal.cpu().numpy()[hit & (s[:, 6] > 0)].astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 1e-6
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.querySweep(state, y)
    assert seen["call"][0] == y.data_ptr() and torch.equal(again["prim"], got["prim"]) and torch.equal(again["t"], got["t"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :7].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.querySweep(state, bad)
    assert pt.querySweep(state, x[:0])["t"].shape == (0,)


def test_cli_sweep_prints_what_querysweep_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (F(0.5) * (lo + hi)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    # from under the ceiling in front of the blocks straight down, without and with a tmax that ends in mid-air; from in front of the open
    # side into the room; from beside the box, away from it
    up = (c[0], hi[1] - F(100.0), lo[2] + F(60.0))
    queries = [up + (0.0, -1.0, 0.0, 10.0, None), (c[0], c[1], lo[2] - F(300.0), 0.25, 0.125, 2.0, 25.0, None),
               up + (0.0, -1.0, 0.0, 10.0, 5.0), (hi[0] + F(500.0), c[1], c[2], 1.0, 0.0, 0.0, 10.0, None)]
    queries = [tuple(None if a is None else float(np.float32(a)) for a in q) for q in queries]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for q in queries:
        cmd += ["--sweep", ",".join("%r" % a for a in q if a is not None)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"sweep"')]
    assert len(lines) == len(queries)
    sweeps = np.array([q[:7] + (np.inf if q[7] is None else q[7],) for q in queries], np.float32)
    got = pt.querySweep(state, sweeps)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    assert got["prim"][0] != 0xFFFFFFFF and got["prim"][1] != 0xFFFFFFFF and got["prim"][2] == 0xFFFFFFFF and got["prim"][3] == 0xFFFFFFFF
    for i, line in enumerate(lines):
        assert np.array_equal(np.array(line["sweep"], np.float32), sweeps[i, :7])
        assert line["tmax"] == queries[i][7]
        if got["prim"][i] == 0xFFFFFFFF:
            assert line == {"sweep": line["sweep"], "tmax": line["tmax"], "hit": False}
            continue
        assert line["hit"] is True and line["triangle"] == int(got["prim"][i])
        assert np.float32(line["t"]) == got["t"][i]
        assert line["material"] == names[int(got["material"][i])]
        assert np.array_equal(np.array(line["point"], np.float32), got["point"][i])
        assert np.float32(line["u"]) == got["u"][i] and np.float32(line["v"]) == got["v"][i]
    for arg in ("1,2,3,4,5,6", "1,2,3,0,1,nan,1", "1,2,3,0,1,0,-1", "1,2,3,0,1,0,1,-2", "1,2,3,0,1,0,inf"):
        bad = subprocess.run([exe, "--obj", BOX, "--sweep", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--sweep" in bad.stderr, (arg, bad.returncode, bad.stderr)
