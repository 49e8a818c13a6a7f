"""Device-resident ray queries on the GPU: pt_query_closest / pt_query_any against the host queries (bits) and against
tests/query_ref.py (the whole record, bits), the rays that are a miss before any traversal, the features, the scene's memory, scene
edits, the render state, the refusals, torch tensors and acgpt_main --pick."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import denoise_ref as dr
import query_ref as qr

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
    n = rays.shape[0]
    t = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32)
    assert _L().pt_trace_closest(state.context, rays.ctypes.data, n, t.ctypes.data, prim.ctypes.data) == 0, _err(state)
    return t, prim


def _host_any(state, rays):
    hit = np.zeros(rays.shape[0], np.uint8)
    assert _L().pt_trace_any(state.context, rays.ctypes.data, rays.shape[0], hit.ctypes.data) == 0, _err(state)
    return hit


class _DeviceRays:
    """rays in a device buffer, with room for the records and the bytes beside them; the C ABI called as a C caller would"""
    def __init__(self, state, rays):
        self.state, self.n = state, rays.shape[0]
        self.rays = np.ascontiguousarray(rays, np.float32)
        self.bufs = pt.pathtracer._device_buffers(state, 3, max(self.rays.nbytes, 32))
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.rays.ctypes.data, self.rays.nbytes) == 0

    def closest(self):
        L, s = _L(), self.state
        assert L.pt_device_memset(s.context, self.bufs[1], 0xCD, self.n * 32) == 0
        assert L.pt_query_closest(s.context, self.bufs[0], self.n, self.bufs[1]) == 0, _err(s)
        rec = np.zeros((self.n, 8), np.uint32)
        assert L.pt_copy_to_host(s.context, rec.ctypes.data, self.bufs[1], rec.nbytes) == 0
        return rec

    def any(self):
        L, s = _L(), self.state
        assert L.pt_device_memset(s.context, self.bufs[2], 0xCD, self.n) == 0
        assert L.pt_query_any(s.context, self.bufs[0], self.n, self.bufs[2]) == 0, _err(s)
        occ = np.zeros(self.n, np.uint8)
        assert L.pt_copy_to_host(s.context, occ.ctypes.data, self.bufs[2], occ.nbytes) == 0
        return occ

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _query(state, rays):
    d = _DeviceRays(state, rays)
    try:
        return d.closest(), d.any()
    finally:
        d.free()


def _reference(obj, rays, t, prim):
    return qr.hit_records(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices())


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
    box under an fp32-node variant (the scene of test_features_on_an_fp32_node_scene).  name -> (state, obj)"""
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
def host_answers(scenes):
    """(scene, set) -> (rays, t, prim, occluded) of the host queries on the whole set: computed once, shared, never written"""
    cache = {}

    def get(scene, name):
        if (scene, name) not in cache:
            state, obj = scenes(scene)
            rays = qr.ray_set(name, obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))
            t, prim = _host_closest(state, rays)
            occ = _host_any(state, rays)
            for a in (rays, t, prim, occ):
                a.setflags(write=False)
            cache[(scene, name)] = (rays, t, prim, occ)
        return cache[(scene, name)]

    return get


def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


def test_scene_memory_is_what_it_was(gpu_state_factory):
    """Before any host query has brought the fp32 nodes: a default scene holds the fp16 nodes only, and the calls leave it so."""
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    before = pt.getBvhInfo(state).device_bytes
    rays = qr.ray_set("inside", obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))
    rec, occ = _query(state, rays)
    assert pt.getBvhInfo(state).device_bytes == before
    t, prim = _host_closest(state, rays)                           # now the fp32 nodes come
    assert pt.getBvhInfo(state).device_bytes > before
    assert np.array_equal(rec[:, 0], t.view(np.uint32)) and np.array_equal(rec[:, 1], prim)
    assert np.array_equal(occ, _host_any(state, rays))
    assert (prim != 0xFFFFFFFF).mean() >= 0.25


@pytest.mark.parametrize("name", qr.RAY_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_closest_and_any_equal_the_host_queries(scenes, host_answers, scene, name):
    state, obj = scenes(scene)
    rays, t, prim, occ = host_answers(scene, name)
    hit = prim != 0xFFFFFFFF
    # the set still does what it is there for, by the host queries' own answers: a set that lost its hits must not pass vacuously
    if name == "outside":
        assert not hit.any()
    else:
        assert hit.mean() >= 0.25 and (~hit).mean() >= 0.10, (name, hit.mean())
    assert np.array_equal(occ.astype(bool), hit)
    before = pt.getBvhInfo(state).device_bytes
    ref = _reference(obj, rays, t, prim)
    for n in SIZES:
        rec, got = _query(state, rays[:n])
        assert np.array_equal(rec[:, 0], t[:n].view(np.uint32)), (n, "t")
        assert np.array_equal(rec[:, 1], prim[:n]), (n, "prim")
        bad = (rec != ref[:n]).any(axis=1)
        assert not bad.any(), (n, np.flatnonzero(bad)[:4], rec[bad][:2], ref[:n][bad][:2])
        assert np.isin(got, (0, 1)).all(), n
        assert np.array_equal(got, occ[:n]), n
    assert pt.getBvhInfo(state).device_bytes == before


def test_bad_rays_between_good_ones(scenes, host_answers):
    state, obj = scenes("box")
    rays, t, prim, occ = host_answers("box", "inside")
    good = rays[(prim != 0xFFFFFFFF) & np.isfinite(rays[:, 7])][:64]
    bad, why = qr.bad_rays(good[0])
    assert bad.shape[0] < 32 and good.shape[0] == 64
    mixed = good.copy()
    where = 2 * np.arange(bad.shape[0]) + 1                 # every other lane of the first wave
    mixed[where] = bad
    still_good = np.ones(64, bool); still_good[where] = False
    alone_rec, alone_occ = _query(state, good)
    assert (alone_rec[:, 1] != 0xFFFFFFFF).all() and alone_occ.all()
    rec, got = _query(state, mixed)
    wrong = (rec[where] != qr.miss_records(where.size)).any(axis=1)
    assert not wrong.any(), [why[i] for i in np.flatnonzero(wrong)]
    assert not got[where].any(), [why[i] for i in np.flatnonzero(got[where])]
    assert np.array_equal(rec[still_good], alone_rec[still_good]) and np.array_equal(got[still_good], alone_occ[still_good])
    # rays that look odd and are rays: no far end, a short direction, a zero direction (the triangle test turns it away, not a rule)
    odd = np.repeat(good[:1], 3, axis=0)
    odd[0, 7] = np.inf
    odd[1, 3:6] *= np.float32(1e-3)          # t is in units of the direction's length
    odd[1, 7] = np.inf
    odd[2, 3:6] = 0.0
    assert qr.traceable(odd).all()
    ht, hp = _host_closest(state, odd)
    rec, got = _query(state, odd)
    assert np.array_equal(rec, _reference(obj, odd, ht, hp)) and np.array_equal(got, _host_any(state, odd))
    assert hp[0] == alone_rec[0, 1] and hp[2] == 0xFFFFFFFF


def test_camera_rays_equal_the_features(scenes):
    state, obj = scenes("box")
    w, h = int(state.params.width), int(state.params.height)
    assert (w, h) == (97, 61)                                # odd sizes: a partial last wave
    alb, nd = pt.renderFeatures(state)
    rec, _ = _query(state, dr.pixel_rays(w, h, *_camera(state)))
    nd, alb = nd.reshape(-1, 4).view(np.uint32), alb.reshape(-1, 4).view(np.uint32)
    assert np.array_equal(rec[:, 0], nd[:, 3]) and np.array_equal(rec[:, 1], alb[:, 3])
    assert np.array_equal(rec[:, 4:7], nd[:, 0:3])
    assert 0.5 < (rec[:, 1] != 0xFFFFFFFF).mean() < 1.0


def test_queryrays_numpy_path(scenes, host_answers):
    state, obj = scenes("diffuse")
    rays, t, prim, occ = host_answers("diffuse", "occlusion")
    ref = _reference(obj, rays, t, prim)
    got = pt.queryRays(state, rays)
    assert got["t"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32
    assert got["uv"].shape == (rays.shape[0], 2) and got["normal"].shape == (rays.shape[0], 3)
    packed = np.concatenate([got["t"].view(np.uint32)[:, None], got["prim"][:, None], got["uv"].view(np.uint32), got["normal"].view(np.uint32),
                             got["material"][:, None]], axis=1)
    assert np.array_equal(packed, ref)
    any_hit = pt.queryRays(state, rays.tolist(), any_hit=True)          # anything np.asarray takes
    assert any_hit.dtype == np.bool_ and np.array_equal(any_hit, occ.astype(bool))


def test_after_scene_edits_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    rays = np.concatenate([qr.ray_set(name, obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state)) for name in ("camera", "inside")])
    _query(state, rays)                                      # the queries have run on the scene before it changes
    fresh = []
    try:
        # 1. a refit: the tall block's and the short block's vertices (everything strictly inside the room) move
        verts = np.array(obj.getVerticesFloat(), np.float32).reshape(-1, 4).copy()
        lo, hi = qr.scene_box(verts, obj.getIndexBuffer())
        inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)
        assert 8 <= inner.sum() < verts.shape[0]
        verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
        info = pt.updateVertices(state, verts, "refit")
        assert not info["rebuilt"]
        moved = pt.TinyObjWrapper(BOX)
        moved._vertices = verts.reshape(-1).copy()
        fresh.append(_fresh_state(state, moved))
        rec, occ = _query(state, rays)
        rec2, occ2 = _query(fresh[-1], rays)
        assert np.array_equal(rec, rec2) and np.array_equal(occ, occ2)
        t, prim = _host_closest(fresh[-1], rays)
        assert np.array_equal(rec, _reference(moved, rays, t, prim))
        assert (prim != 0xFFFFFFFF).mean() >= 0.25
        # 2. new material assignments on top: the ids rotate by one
        n_mats = obj.getNumMaterials()
        ids = ((np.asarray(obj.getMaterialIndices(), np.uint32) + 1) % n_mats).astype(np.uint32)
        pt.updateMaterials(state, material_ids=ids)
        moved._materialIndices = ids
        fresh.append(_fresh_state(state, moved))
        rec3, occ3 = _query(state, rays)
        rec4, occ4 = _query(fresh[-1], rays)
        assert np.array_equal(rec3, rec4) and np.array_equal(occ3, occ4)
        assert np.array_equal(rec3, _reference(moved, rays, t, prim))
        assert np.array_equal(rec3[:, :7], rec[:, :7]) and (rec3[:, 7] != rec[:, 7])[prim != 0xFFFFFFFF].all()
    finally:
        for s in fresh:
            pt.CleanAllTheThings(s)


def test_queries_leave_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    rays = qr.ray_set("inside", obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        _query(state, rays)
        pt.queryRays(state, rays, any_hit=True)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_refusals_leave_the_context_usable(scenes, host_answers):
    state, obj = scenes("box")
    rays, t, prim, occ = host_answers("box", "camera")
    L = _L()
    d = _DeviceRays(state, rays[:256])
    try:
        expected = d.closest()
        r, h, o = d.bufs
        refused = {
            "null rays": L.pt_query_closest(state.context, None, 256, h),
            "null hits": L.pt_query_closest(state.context, r, 256, None),
            "any: null rays": L.pt_query_any(state.context, None, 256, o),
            "any: null output": L.pt_query_any(state.context, r, 256, None),
            "too many": L.pt_query_closest(state.context, r, 0x80000000, h),
            "any: too many": L.pt_query_any(state.context, r, 0x80000000, o),
            "hits are the rays": L.pt_query_closest(state.context, r, 256, r),
            "hits overlap the rays' end": L.pt_query_closest(state.context, r, 256, r + 255 * 32),
            "any: output inside the rays": L.pt_query_any(state.context, r, 256, r + 100),
            "rays not aligned": L.pt_query_closest(state.context, r + 4, 16, h),
            "hits not aligned": L.pt_query_closest(state.context, r, 16, h + 8),
            "null context": L.pt_query_closest(None, r, 256, h),
            "any: null context": L.pt_query_any(None, r, 256, o),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_closest(state.context, None, 256, h) != 0 and _err(state).startswith("pt_query_closest: ")
        assert L.pt_query_any(state.context, r, 256, None) != 0 and _err(state).startswith("pt_query_any: ")
        assert L.pt_query_closest(state.context, r, 0x80000000, h) != 0 and "too many rays" in _err(state)
        assert L.pt_query_closest(state.context, r, 256, r) != 0 and "overlaps" in _err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_closest(bare, r, 256, h) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_any(bare, r, 256, o) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_closest(bare, None, 0, None) == 0             # no rays: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_closest(state.context, None, 0, None) == 0 and L.pt_query_any(state.context, None, 0, None) == 0
        assert np.array_equal(d.closest(), expected)                        # the next valid call
        assert np.array_equal(d.any(), occ[:256])
        assert np.array_equal(expected, _reference(obj, rays[:256], t[:256], prim[:256]))
    finally:
        d.free()


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, host_answers, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    rays, t, prim, occ = host_answers("box", "inside")
    ref = pt.queryRays(state, rays)
    L = _L()
    seen = {}
    real_closest, real_any = L.pt_query_closest, L.pt_query_any
    monkeypatch.setattr(L, "pt_query_closest", lambda ctx, r, n, out: seen.update(closest=(r, n, out)) or real_closest(ctx, r, n, out))
    monkeypatch.setattr(L, "pt_query_any", lambda ctx, r, n, out: seen.update(any=(r, n, out)) or real_any(ctx, r, n, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(rays.copy()).to(dev)
    got = pt.queryRays(state, x)
    assert seen["closest"][0] == x.data_ptr() and seen["closest"][1] == rays.shape[0]
    assert all(v.device == dev for v in got.values())
    assert seen["closest"][2] == got["t"].data_ptr()                       # the columns are views of the tensor the library wrote
    assert got["t"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32
    assert got["uv"].shape == (rays.shape[0], 2) and got["normal"].shape == (rays.shape[0], 3)
    for k in ("t", "uv", "normal"):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), ref[k].view(np.uint32)), k
    for k in ("prim", "material"):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), ref[k]), k
    occluded = pt.queryRays(state, x, any_hit=True)
    assert seen["any"][0] == x.data_ptr()
    assert occluded.dtype == torch.bool and occluded.device == dev and np.array_equal(occluded.cpu().numpy(), occ.astype(bool))
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.queryRays(state, y)
    assert seen["closest"][0] == y.data_ptr() and torch.equal(again["prim"], got["prim"]) and torch.equal(again["t"], got["t"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :6].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.queryRays(state, bad)
    assert pt.queryRays(state, x[:0])["t"].shape == (0,)


def test_cli_pick_prints_what_queryrays_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    w, h = 128, 96
    picks = [(w // 2, h // 2), (0, 0), (w - 1, h - 1), (40, 30)]
    cmd = [exe, "--obj", BOX, "--width", str(w), "--height", str(h), "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for x, y in picks:
        cmd += ["--pick", "%d,%d" % (x, y)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"pick"')]
    assert [tuple(l["pick"]) for l in lines] == picks
    state, obj = gpu_state_factory(BOX, width=w, height=h, max_depth=4, spp=1)
    rays = dr.pixel_rays(w, h, *_camera(state))[[y * w + x for x, y in picks]]
    got = pt.queryRays(state, rays)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    assert got["prim"][0] != 0xFFFFFFFF and got["prim"][1] == 0xFFFFFFFF         # the centre hits, the corner misses
    for i, line in enumerate(lines):
        if got["prim"][i] == 0xFFFFFFFF:
            assert line == {"pick": list(picks[i]), "hit": False}
            continue
        assert line["hit"] is True and line["prim"] == int(got["prim"][i])
        assert np.float32(line["t"]) == got["t"][i]
        assert line["material"] == names[int(got["material"][i])]
        assert np.array_equal(np.array(line["normal"], np.float32), got["normal"][i])
        assert np.array_equal(np.array(line["position"], np.float32), rays[i, 0:3] + got["t"][i] * rays[i, 3:6])
    bad = subprocess.run([exe, "--obj", BOX, "--width", str(w), "--height", str(h), "--pick", "%d,0" % w], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "outside" in bad.stderr
