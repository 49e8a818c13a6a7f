"""Ambient occlusion on the GPU: pt_ao_points / pt_ao_image against the host any-hit query on the rays of tests/ao_ref.py (counts as
integers, ao as bits), points that are no surface inside a wave, accumulation, determinism, what a call leaves alone, scene edits,
the refusals, the Python wrappers, torch tensors and acgpt_main --ao."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import ao_ref as ar
import query_ref as qr

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
SAMPLES = (1, 2, 16, 256)
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build


def _L():
    return _native.hip()


def _ao_entry(name):
    """The entry point, looked up the way a caller binds it: every test of this file fails here on a library without the stage"""
    return getattr(_L(), name)


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


def _camera(state):
    p = state.params
    return p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple()


def _host_any(state, rays):
    hit = np.zeros(rays.shape[0], np.uint8)
    assert _L().pt_trace_any(state.context, rays.ctypes.data, rays.shape[0], hit.ctypes.data) == 0, _err(state)
    return hit


def _params(disk, p, seed=None, accumulate=0, total=None):
    K = disk.shape[0]
    return _native.AoParams(K, p["radius"], p["bias"], p["seed"] if seed is None else seed, accumulate, K if total is None else total, (C.c_uint32 * 2)(0, 0))


class _Device:
    """input records in a device buffer with room for visible and ao beside them; the C ABI called as a C caller would"""
    def __init__(self, state, records):
        self.state = state
        self.rec = np.ascontiguousarray(records, np.float32)
        self.bufs = pt.pathtracer._device_buffers(state, 3, max(self.rec.nbytes, 32))
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.rec.ctypes.data, self.rec.nbytes) == 0

    def read(self, n):
        vis, ao = np.zeros(n, np.uint32), np.zeros(n, np.float32)
        assert _L().pt_copy_to_host(self.state.context, vis.ctypes.data, self.bufs[1], vis.nbytes) == 0
        assert _L().pt_copy_to_host(self.state.context, ao.ctypes.data, self.bufs[2], ao.nbytes) == 0
        return vis, ao.view(np.uint32)

    def points(self, n, disk, ap, fill=True, want_ao=True):
        L, s = _L(), self.state
        if fill:
            assert L.pt_device_memset(s.context, self.bufs[1], 0xCD, n * 4) == 0 and L.pt_device_memset(s.context, self.bufs[2], 0xCD, n * 4) == 0
        assert _ao_entry("pt_ao_points")(s.context, self.bufs[0], n, disk.ctypes.data, C.byref(ap), self.bufs[1], self.bufs[2] if want_ao else None) == 0, _err(s)
        return self.read(n)

    def image(self, disk, ap, fill=True):
        L, s = _L(), self.state
        n = int(s.params.width) * int(s.params.height)
        if fill:
            assert L.pt_device_memset(s.context, self.bufs[1], 0xCD, n * 4) == 0 and L.pt_device_memset(s.context, self.bufs[2], 0xCD, n * 4) == 0
        assert _ao_entry("pt_ao_image")(s.context, C.byref(s.params), self.bufs[0], disk.ctypes.data, C.byref(ap), self.bufs[1], self.bufs[2]) == 0, _err(s)
        return self.read(n)

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _records(P, N):
    rec = np.zeros((P.shape[0], 8), np.float32)
    rec[:, 0:3] = P
    rec[:, 4:7] = N
    rec[:, 3] = np.float32(np.nan)          # the unused words are unused
    rec[:, 7] = np.float32(np.inf)
    return rec


def _expected(state, P, N, disk, p, total=None, first=0):
    """(visible, ao bits, occluded share) by the host any-hit query on the reference's rays"""
    K = disk.shape[0]
    r = ar.rays(P, N, disk, p, first=first)
    send = r.copy()
    send[~qr.traceable(r)] = (0, 0, 0, 0, 0, 1, 0, 1)      # the host query gets rays only; counts() knows which ones were none
    occ = _host_any(state, send)
    vis = ar.counts(occ, r, K)
    return vis, ar.ao_value(vis, K if total is None else total).view(np.uint32), float(occ.mean())


def _fresh_state(like, obj, tuning=None):
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
    """The three scenes of tests/test_gpu_query.py, each set up once: name -> (state, obj, points, normals, parameters)"""
    made, extra = {}, []

    def get(name):
        if name not in made:
            if name == "fp32":
                base, obj = get("box")[:2]
                state = _fresh_state(base, obj, tuning=1)           # variant 1: fp32 nodes
                extra.append(state)
            else:
                state, obj = gpu_state_factory({"box": BOX, "diffuse": BOX_DIFFUSE}[name], width=97, height=61, max_depth=4, spp=8)
            P, N = ar.occlusion_points(obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))
            for a in (P, N):
                a.setflags(write=False)
            made[name] = (state, obj, P, N, ar.gpu_test_parameters(obj.getVerticesFloat(), obj.getIndexBuffer()))
        return made[name]

    yield get
    for s in extra:
        pt.CleanAllTheThings(s)


def test_kernel_source_hash_is_the_parents():
    _ao_entry("pt_ao_points")
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@pytest.mark.parametrize("K", SAMPLES)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_points_equal_the_host_query_on_the_reference_rays(scenes, scene, K):
    state, obj, P, N, p = scenes(scene)
    disk = pt.aoSamples(K)
    before = pt.getBvhInfo(state).device_bytes if scene != "fp32" else None
    d = _Device(state, _records(P, N))
    try:
        got = {n: d.points(n, disk, _params(disk, p)) for n in SIZES}
        assert before is None or pt.getBvhInfo(state).device_bytes == before      # before the host query below brings the fp32 nodes
        vis, ao, share = _expected(state, P, N, disk, p)
        # the set still does what it is there for, by the host query's own answers
        assert share >= 0.10 and 1.0 - share >= 0.10, share
        for n in SIZES:
            assert np.array_equal(got[n][0], vis[:n]), (n, np.flatnonzero(got[n][0] != vis[:n])[:4])
            assert np.array_equal(got[n][1], ao[:n]), n
        only_visible, untouched = d.points(257, disk, _params(disk, p), want_ao=False)
        assert np.array_equal(only_visible, vis[:257]) and (untouched == 0xCDCDCDCD).all()
    finally:
        d.free()


def test_no_surface_points_between_good_ones(scenes):
    state, obj, P, N, p = scenes("box")
    K = 16
    disk = pt.aoSamples(K)
    P, N = P[:64].copy(), N[:64].copy()
    alone, _, _ = _expected(state, P, N, disk, p)
    assert (alone < K).sum() >= 16                           # points with something above them
    bad = []
    for k in range(3):
        for val in (np.nan, np.inf, -np.inf):
            bad += [("P", k, val), ("N", k, val)]
    bad.append(("N", None, 0.0))
    where = 2 * np.arange(len(bad)) + 1                      # every other lane of the first wave
    assert where.max() < 64
    for i, (what, k, val) in zip(where, bad):
        if k is None:
            N[i] = 0.0
        else:
            (P if what == "P" else N)[i, k] = val
    good = np.ones(64, bool); good[where] = False
    d = _Device(state, _records(P, N))
    try:
        vis, ao = d.points(64, disk, _params(disk, p))
    finally:
        d.free()
    assert (vis[where] == K).all(), [bad[j] for j in np.flatnonzero(vis[where] != K)]
    assert (ao[where] == np.float32(1.0).view(np.uint32)).all()
    assert np.array_equal(vis[good], alone[good])
    want, want_ao, _ = _expected(state, P, N, disk, p)
    assert np.array_equal(vis, want) and np.array_equal(ao, want_ao)


@pytest.mark.parametrize("size", [(1, 1), (9, 7), (97, 61), (128, 128)])
@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_image_equals_the_same_construction_from_the_features(scenes, scene, size):
    base, obj, _, _, p = scenes(scene)
    w, h = size
    state = base
    old = (int(base.params.width), int(base.params.height))
    state.params.width, state.params.height = w, h           # the camera stays: the calls read width, height and the camera only
    K = 16
    disk = pt.aoSamples(K)
    try:
        nd = pt.renderFeatures(state)[1]
        miss = nd[..., 3].reshape(-1) < 0
        if (w, h) != (1, 1):
            assert miss.any() and (~miss).any()               # miss pixels included
        d = _Device(state, nd)
        try:
            vis, ao = d.image(disk, _params(disk, p, seed=9))
        finally:
            d.free()
        P, N = ar.image_points(nd, _camera(state), w, h)
        want, want_ao, share = _expected(state, P, N, disk, dict(p, seed=9))
        assert np.array_equal(vis, want), np.flatnonzero(vis != want)[:4]
        assert np.array_equal(ao, want_ao)
        assert (vis[miss] == K).all()
        if w * h >= 63:
            assert share >= 0.10 and (want[~miss] < K).any() and (want[~miss] > 0).any()
        got = pt.ambientOcclusion(state, samples=K, radius=p["radius"], bias=p["bias"], seed=9)
        assert got.shape == (h, w) and np.array_equal(got.reshape(-1).view(np.uint32), want_ao)
        assert np.array_equal(pt.ambientOcclusion(state, disk=disk, radius=p["radius"], bias=p["bias"], seed=9, normal_depth=nd), got)
    finally:
        state.params.width, state.params.height = old


def test_accumulate_and_determinism(scenes):
    state, obj, P, N, p = scenes("diffuse")
    K, n = 16, 1000
    disk = pt.aoSamples(K)
    d = _Device(state, _records(P, N))
    try:
        singles = [d.points(n, disk, _params(disk, p, seed=s))[0] for s in (0, 1, 2)]
        assert not np.array_equal(singles[0], singles[1])                     # another seed: other rays
        again = d.points(n, disk, _params(disk, p, seed=1))
        twice = d.points(n, disk, _params(disk, p, seed=1))
        assert np.array_equal(again[0], singles[1]) and np.array_equal(again[0], twice[0]) and np.array_equal(again[1], twice[1])
        for j, s in enumerate((0, 1, 2)):
            vis, ao = d.points(n, disk, _params(disk, p, seed=s, accumulate=1 if j else 0, total=K * (j + 1)), fill=(j == 0))
            assert np.array_equal(vis, sum(singles[:j + 1]))
            assert np.array_equal(ao, ar.ao_value(vis, K * (j + 1)).view(np.uint32))
        want, _, _ = _expected(state, P, N, disk, dict(p, seed=2))
        assert np.array_equal(singles[2], want)
    finally:
        d.free()
    # the class that does this for a view
    prog = pt.AmbientOcclusion(samples=K, radius=p["radius"], bias=p["bias"])
    try:
        imgs = [prog.update(state) for _ in range(3)]
        one = [pt.ambientOcclusion(state, samples=K, radius=p["radius"], bias=p["bias"], seed=s) for s in (0, 1, 2)]
        total = sum((o * np.float32(K)).astype(np.uint32) for o in one)
        assert prog.total == 3 * K and np.array_equal(prog.visible(), total)
        assert np.array_equal(imgs[0], one[0]) and np.array_equal(imgs[2], ar.ao_value(total, 3 * K))
    finally:
        prog.close()


def test_calls_leave_the_render_state_and_the_scene_memory_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    before = pt.getBvhInfo(state).device_bytes
    P, N = ar.occlusion_points(obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        img = pt.ambientOcclusion(state)
        baked = pt.bakeAO(state, P, N, samples=16)
        assert 0.0 < img.mean() < 1.0 and 0.0 < baked.mean() < 1.0
        assert pt.getBvhInfo(state).device_bytes == before
        assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_after_a_vertex_update_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    p = ar.gpu_test_parameters(obj.getVerticesFloat(), obj.getIndexBuffer())
    kw = dict(samples=16, radius=p["radius"], bias=p["bias"])
    first = pt.ambientOcclusion(state, **kw)
    verts = np.array(obj.getVerticesFloat(), np.float32).reshape(-1, 4).copy()
    lo, hi = qr.scene_box(verts, obj.getIndexBuffer())
    inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)      # the two blocks
    assert 8 <= inner.sum() < verts.shape[0]
    verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
    assert not pt.updateVertices(state, verts, "refit")["rebuilt"]
    moved = pt.TinyObjWrapper(BOX)
    moved._vertices = verts.reshape(-1).copy()
    fresh = _fresh_state(state, moved)
    try:
        a, b = pt.ambientOcclusion(state, **kw), pt.ambientOcclusion(fresh, **kw)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not np.array_equal(a, first)
        va, vb = pt.bakeVertexAO(state, **kw), pt.bakeVertexAO(fresh, **kw)
        assert va.shape == (verts.shape[0],) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
        assert 0.0 < va.mean() < 1.0
        nrm = pt.vertexNormals(verts[:, :3], obj.getIndexBuffer())
        want, want_ao, _ = _expected(fresh, verts[:, :3], nrm, pt.aoSamples(16), p)
        assert np.array_equal(va.view(np.uint32), want_ao)
    finally:
        pt.CleanAllTheThings(fresh)


def test_refusals_leave_the_context_usable(scenes):
    state, obj, P, N, p = scenes("box")
    L = _L()
    K, n = 16, 256
    disk = pt.aoSamples(K)
    ok = _params(disk, p)
    d = _Device(state, _records(P[:n], N[:n]))
    nd_state = state
    nd = pt.renderFeatures(nd_state)[1]
    dn = _Device(state, nd)
    try:
        expected = d.points(n, disk, ok)
        r, v, a = d.bufs
        dp = disk.ctypes.data

        def bad(**kw):
            q = _native.AoParams(K, p["radius"], p["bias"], 0, 0, K, (C.c_uint32 * 2)(0, 0))
            for k, val in kw.items():
                if k == "reserved":
                    q.reserved[val] = 1
                else:
                    setattr(q, k, val)
            return C.byref(q)

        outside = np.array(disk); outside[5] = (0.8, 0.7)
        nan_disk = np.array(disk); nan_disk[K - 1, 1] = np.nan
        pts, img = L.pt_ao_points, L.pt_ao_image
        prm = C.byref(state.params)
        refused = {
            "null context": pts(None, r, n, dp, C.byref(ok), v, a),
            "null points": pts(state.context, None, n, dp, C.byref(ok), v, a),
            "null disk": pts(state.context, r, n, None, C.byref(ok), v, a),
            "null params": pts(state.context, r, n, dp, None, v, a),
            "null visible": pts(state.context, r, n, dp, C.byref(ok), None, a),
            "points not aligned": pts(state.context, r + 8, 16, dp, C.byref(ok), v, a),
            "visible not aligned": pts(state.context, r, 16, dp, C.byref(ok), v + 2, a),
            "ao not aligned": pts(state.context, r, 16, dp, C.byref(ok), v, a + 1),
            "too many": pts(state.context, r, 0x80000000, dp, C.byref(ok), v, a),
            "K = 0": pts(state.context, r, n, dp, bad(samples=0, total_samples=0), v, a),
            "K = 257": pts(state.context, r, n, dp, bad(samples=257, total_samples=257), v, a),
            "radius 0": pts(state.context, r, n, dp, bad(radius=0.0), v, a),
            "radius < 0": pts(state.context, r, n, dp, bad(radius=-1.0), v, a),
            "radius inf": pts(state.context, r, n, dp, bad(radius=np.inf), v, a),
            "radius nan": pts(state.context, r, n, dp, bad(radius=np.nan), v, a),
            "bias < 0": pts(state.context, r, n, dp, bad(bias=-1e-3), v, a),
            "bias inf": pts(state.context, r, n, dp, bad(bias=np.inf), v, a),
            "bias nan": pts(state.context, r, n, dp, bad(bias=np.nan), v, a),
            "total < samples": pts(state.context, r, n, dp, bad(total_samples=K - 1), v, a),
            "reserved[0]": pts(state.context, r, n, dp, bad(reserved=0), v, a),
            "reserved[1]": pts(state.context, r, n, dp, bad(reserved=1), v, a),
            "disk point outside": pts(state.context, r, n, outside.ctypes.data, C.byref(ok), v, a),
            "disk point nan": pts(state.context, r, n, nan_disk.ctypes.data, C.byref(ok), v, a),
            "visible is the points": pts(state.context, r, n, dp, C.byref(ok), r, a),
            "visible inside the points' end": pts(state.context, r, n, dp, C.byref(ok), r + n * 32 - 4, a),
            "ao inside the points": pts(state.context, r, n, dp, C.byref(ok), v, r + 64),
            "ao is visible": pts(state.context, r, n, dp, C.byref(ok), v, v),
            "ao overlaps visible's end": pts(state.context, r, n, dp, C.byref(ok), v, v + n * 4 - 4),
            "image: null context": img(None, prm, dn.bufs[0], dp, C.byref(ok), v, a),
            "image: null params": img(state.context, None, dn.bufs[0], dp, C.byref(ok), v, a),
            "image: null features": img(state.context, prm, None, dp, C.byref(ok), v, a),
            "image: null disk": img(state.context, prm, dn.bufs[0], None, C.byref(ok), v, a),
            "image: null visible": img(state.context, prm, dn.bufs[0], dp, C.byref(ok), None, a),
            "image: features not aligned": img(state.context, prm, dn.bufs[0] + 4, dp, C.byref(ok), v, a),
            "image: visible in the features": img(state.context, prm, dn.bufs[0], dp, C.byref(ok), dn.bufs[0] + 16, a),
            "image: K = 0": img(state.context, prm, dn.bufs[0], dp, bad(samples=0), v, a),
        }
        assert all(rc != 0 for rc in refused.values()), {k: rc for k, rc in refused.items() if rc == 0}
        assert pts(state.context, r, n, None, C.byref(ok), v, a) != 0 and _err(state).startswith("pt_ao_points: ")
        assert img(state.context, prm, dn.bufs[0], dp, C.byref(ok), None, a) != 0 and _err(state).startswith("pt_ao_image: ")
        assert pts(state.context, r, n, outside.ctypes.data, C.byref(ok), v, a) != 0 and "disk point 5" in _err(state)
        assert pts(state.context, r, n, dp, C.byref(ok), v, v) != 0 and "overlaps" in _err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert pts(bare, r, n, dp, C.byref(ok), v, a) != 0 and b"no scene" in L.pt_last_error(bare)
            assert img(bare, prm, dn.bufs[0], dp, C.byref(ok), v, a) != 0 and b"no scene" in L.pt_last_error(bare)
            assert pts(bare, None, 0, None, None, None, None) == 0          # no points: nothing to do, nothing to refuse
        finally:
            L.pt_destroy(bare)
        assert pts(state.context, None, 0, None, None, None, None) == 0
        empty = pt.PathTraceParams()
        C.memmove(C.byref(empty), C.byref(state.params), C.sizeof(empty))
        empty.width = 0
        assert img(state.context, C.byref(empty), None, None, None, None, None) == 0
        got = d.points(n, disk, ok)                                          # the next valid call
        assert np.array_equal(got[0], expected[0]) and np.array_equal(got[1], expected[1])
        want, want_ao, _ = _expected(state, P[:n], N[:n], disk, p)
        assert np.array_equal(expected[0], want) and np.array_equal(expected[1], want_ao)
    finally:
        d.free()
        dn.free()


def test_bakeao_numpy_and_torch_paths(scenes, monkeypatch):
    state, obj, P, N, p = scenes("box")
    K = 16
    kw = dict(samples=K, radius=p["radius"], bias=p["bias"])
    want, want_ao, _ = _expected(state, P, N, pt.aoSamples(K), p)
    got = pt.bakeAO(state, P, N, **kw)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want_ao)
    assert np.array_equal(pt.bakeAO(state, _records(P, N).tolist(), **kw), got)          # records, and anything np.asarray takes
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    L = _L()
    seen = {}
    real = L.pt_ao_points
    monkeypatch.setattr(L, "pt_ao_points", lambda ctx, pts, n, *rest: seen.update(call=(pts, n)) or real(ctx, pts, n, *rest))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(_records(P, N)).to(dev)
    out = pt.bakeAO(state, x, **kw)
    assert seen["call"] == (x.data_ptr(), P.shape[0])                        # the tensor's own memory went in
    assert out.device == dev and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy().view(np.uint32), want_ao)
    y = (x * 1.0).contiguous()                                               # a result of torch's own kernels, still in flight
    assert torch.equal(pt.bakeAO(state, y, **kw), out) and seen["call"][0] == y.data_ptr()
    split = pt.bakeAO(state, torch.from_numpy(P.copy()).to(dev), torch.from_numpy(N.copy()).to(dev), **kw)
    assert torch.equal(split, out)
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :6].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.bakeAO(state, bad, **kw)
    assert pt.bakeAO(state, x[:0], **kw).shape == (0,)


def test_cli_ao_writes_the_python_paths_image(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    w, h = 128, 96
    common = [exe, "--obj", BOX, "--width", str(w), "--height", str(h), "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    r = subprocess.run(common + ["--ao", "16", "--ao-out", str(tmp_path / "ao.pfm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r3 = subprocess.run(common + ["--ao", "8,120.5,0.25", "--ao-frames", "3", "--ao-out", str(tmp_path / "ao3.pfm")], capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stdout + r3.stderr
    state, obj = gpu_state_factory(BOX, width=w, height=h, max_depth=4, spp=1)
    want = pt.ambientOcclusion(state, samples=16)                            # the defaults on both sides: pattern, radius, bias
    got = pt.readPFM(str(tmp_path / "ao.pfm"))[::-1]                         # row 0 = bottom, as the buffer holds it
    assert got.shape == (h, w, 3) and all(np.array_equal(got[..., k].view(np.uint32), want.view(np.uint32)) for k in range(3))
    assert 0.0 < want.mean() < 1.0
    prog = pt.AmbientOcclusion(samples=8, radius=120.5, bias=0.25)
    try:
        for _ in range(3):
            want3 = prog.update(state)
    finally:
        prog.close()
    assert np.array_equal(pt.readPFM(str(tmp_path / "ao3.pfm"))[::-1][..., 0].view(np.uint32), want3.view(np.uint32))
    for args in (["--ao", "0", "--ao-out", "x.pfm"], ["--ao", "16"], ["--ao-out", "x.pfm"], ["--ao", "16,-1", "--ao-out", "x.pfm"]):
        bad = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--ao" in bad.stderr, args
