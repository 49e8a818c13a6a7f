"""pt_ao_points / pt_ao_image without a GPU: the NumPy statement of the rays (tests/ao_ref.py) by hand and by its properties, the
default sample pattern, the points that are no surface, what the statement says about the Cornell fixtures under the CPU oracle's
brute force (and that the GPU tests' parameters give occluded and open rays alike), and the argument checks of the Python wrappers
that need no device."""
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import ao_ref as ar
import query_ref as qr

F = np.float32
IDENT = np.array([[1.0, 0.0]], np.float32)          # one sample on the disk's x axis


def test_tea4_is_the_renderers(oracle):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
    a[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
    b[:4] = (0, 0xFFFFFFFF, 0xFFFFFFFF, 1)
    got = ar.tea4(a, b)
    assert got.dtype == np.uint32
    assert [int(x) for x in got] == [oracle.tea4(int(x), int(y)) for x, y in zip(a, b)]


def test_rays_by_hand():
    """N = +z: T = (1, 0, 0), S = (0, 1, 0); N = -z: T = (1, 0, 0), S = (0, -1, 0); one sample at the disk's centre goes along N, one
    on its rim along the rotated T; the origin is P + bias N, the interval (0, radius)."""
    params = {"radius": 3.0, "bias": 0.5, "seed": 0}
    P = np.array([[1.0, 2.0, 3.0]] * 2, np.float32)
    N = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], np.float32)
    T, S = ar.frame(N)
    assert np.array_equal(T, [[1, 0, 0], [1, 0, 0]]) and np.array_equal(S, [[0, 1, 0], [0, -1, 0]])
    r = ar.rays(P, N, np.array([[0.0, 0.0]], np.float32), params)
    assert r.shape == (2, 8) and r.dtype == np.float32
    assert np.array_equal(r[:, 0:3], [[1, 2, 3.5], [1, 2, 2.5]])
    assert np.array_equal(r[:, 3:6], N) and np.array_equal(r[:, 6], [0, 0]) and np.array_equal(r[:, 7], [3, 3])
    # a rim sample: d = c T + s S with (c, s) the point's own rotation of (1, 0); z = sqrt(max(0, 1 - c^2 - s^2)) is a rounding's worth
    c, s, _ = ar.rotation(ar.tea4(np.array([0, 1], np.uint32), np.uint32(0)))
    r = ar.rays(P, N, IDENT, params)
    assert np.array_equal(r[0, 3:5], [c[0], s[0]]) and np.array_equal(r[1, 3:5], [c[1], -s[1]]) and (np.abs(r[:, 5]) <= 1e-3).all()
    assert (c[0], s[0]) != (c[1], s[1])
    # a tilted normal, by the formulas in float64: N = (2, -1, 2) / 3
    n = np.array([[2.0, -1.0, 2.0]], np.float32) / F(3.0)
    T, S = ar.frame(n)
    n64 = n[0].astype(np.float64)
    a = -1.0 / (1.0 + n64[2]); b = n64[0] * n64[1] * a
    assert np.allclose(T[0], [1.0 + n64[0] * n64[0] * a, b, -n64[0]], atol=1e-6) and np.allclose(S[0], [b, 1.0 + n64[1] * n64[1] * a, -n64[1]], atol=1e-6)
    for u, v in ((T[0], S[0]), (T[0], n[0]), (S[0], n[0])):
        assert abs(float(np.dot(u.astype(np.float64), v.astype(np.float64)))) <= 1e-6
    r = ar.rays(np.zeros((1, 3), np.float32), n, np.array([[0.6, 0.0]], np.float32), dict(params, bias=0.0))
    c, s, _ = ar.rotation(ar.tea4(np.array([0], np.uint32), np.uint32(0)))
    want = 0.6 * float(c[0]) * T[0].astype(np.float64) + 0.6 * float(s[0]) * S[0].astype(np.float64) + 0.8 * n64
    assert np.allclose(r[0, 3:6], want, atol=1e-6) and np.array_equal(r[0, 0:3], [0, 0, 0])
    # the index of the first point goes into the hash: point 5 alone equals point 5 of six
    six = ar.rays(np.zeros((6, 3), np.float32), np.repeat(n, 6, axis=0), pt.aoSamples(4), params)
    assert np.array_equal(ar.rays(np.zeros((1, 3), np.float32), n, pt.aoSamples(4), params, first=5), six[20:24])


def test_directions_stay_on_the_hemisphere_and_unit():
    rng = np.random.default_rng(11)
    N = rng.normal(size=(4000, 3))
    N = (N / np.sqrt((N * N).sum(axis=1, keepdims=True))).astype(np.float32)
    N[:6] = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [0.6, 0, -0.8], [1e-4, 0, -1]], np.float32)
    N[5] /= np.sqrt((N[5].astype(np.float64) ** 2).sum())
    P = rng.uniform(-5, 5, (4000, 3)).astype(np.float32)
    for K in (1, 16):
        r = ar.rays(P, N, pt.aoSamples(K), {"radius": 1.0, "bias": 0.0, "seed": 3})
        d = r[:, 3:6].astype(np.float64)
        n = np.repeat(N, K, axis=0).astype(np.float64)
        assert ((d * n).sum(axis=1) >= -1e-6).all()
        assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 1e-5
        assert qr.traceable(r).all()


def test_rotation_is_a_rotation_and_reaches_every_quadrant():
    h = ar.tea4(np.arange(100000, dtype=np.uint32), np.uint32(7))
    c, s, q = ar.rotation(h)
    assert c.dtype == np.float32 and s.dtype == np.float32
    assert np.abs(c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1.0).max() <= 4e-7
    for sc, ss in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        assert ((np.sign(c) == sc) & (np.sign(s) == ss)).mean() >= 0.2
    assert all((q == k).mean() >= 0.2 for k in range(4))
    # the quarter turns are exact: the same a under q = 0 .. 3
    same = np.array([0x00001234, 0x00011234, 0x00021234, 0x00031234], np.uint32)
    c, s, q = ar.rotation(same)
    assert np.array_equal(q, [0, 1, 2, 3])
    assert np.array_equal(c, [c[0], -s[0], -c[0], s[0]]) and np.array_equal(s, [s[0], c[0], -s[0], -c[0]])
    # the ends of the parameter: a = 0 is no turn, a -> 1 comes up to a quarter turn from below
    c, s, _ = ar.rotation(np.array([0x00000000, 0x0000FFFF], np.uint32))
    assert (c[0], s[0]) == (1.0, 0.0) and 0.0 < c[1] < 2e-5 and s[1] <= 1.0


def test_default_pattern():
    for K in (1, 2, 16, 256):
        d = pt.aoSamples(K)
        assert d.shape == (K, 2) and d.dtype == np.float32
        assert (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= F(1.0)).all()
        assert np.array_equal(pt.pathtracer._ao_disk(d, K, "test"), d)
    d = pt.aoSamples(256).astype(np.float64)
    z = np.sqrt(np.maximum(0.0, 1.0 - (d * d).sum(axis=1)))
    assert abs(z.mean() - 2.0 / 3.0) <= 0.02 * (2.0 / 3.0)            # cosine-distributed over the hemisphere: E[z] = 2/3
    assert np.abs(d.mean(axis=0)).max() <= 0.02                        # ... and centred
    r2 = (pt.aoSamples(16).astype(np.float64) ** 2).sum(axis=1)
    assert np.allclose(r2, (np.arange(16) + 0.5) / 16, atol=1e-6)
    for bad in (0, 257, -1):
        with pytest.raises(pt.PathTracerError, match="1..256"):
            pt.aoSamples(bad)


def test_points_that_are_no_surface():
    good_p, good_n = [1.0, 2.0, 3.0], [0.0, 1.0, 0.0]
    table = [(good_p, good_n, True), (good_p, [0.0, 0.0, 0.0], False), (good_p, [0.0, -0.0, 0.0], False), (good_p, [0.0, 0.0, 1e-30], True),
             (good_p, [0.0, 2.0, 0.0], True)]
    for k in range(3):
        for val in (np.nan, np.inf, -np.inf):
            p = list(good_p); p[k] = val
            n = list(good_n); n[k] = val
            table += [(p, good_n, False), (good_p, n, False)]
    P = np.array([t[0] for t in table], np.float32); N = np.array([t[1] for t in table], np.float32)
    want = np.array([t[2] for t in table])
    assert np.array_equal(ar.surface(P, N), want)
    K = 4
    r = ar.rays(P, N, pt.aoSamples(K), {"radius": 1.0, "bias": 0.1, "seed": 0})
    assert np.array_equal(qr.traceable(r).reshape(-1, K).all(axis=1), want)
    assert np.array_equal(qr.traceable(r).reshape(-1, K).any(axis=1), want)
    # whatever the query would say about them, they count K: fully open
    vis = ar.counts(np.ones(r.shape[0], np.uint8), r, K)
    assert np.array_equal(vis, np.where(want, 0, K))
    assert np.array_equal(ar.ao_value(vis, K), np.where(want, 0.0, 1.0).astype(np.float32))
    # the image form: a miss pixel (w = -1) and a NaN depth are no surface, a hit is P = eye + t dir
    nd = np.zeros((1, 3, 4), np.float32)
    nd[0, 0] = (0, 0, 1, 2.0); nd[0, 1] = (0, 0, 0, -1.0); nd[0, 2] = (0, 0, 1, np.nan)
    cam = ((1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))
    Pi, Ni = ar.image_points(nd, cam, 3, 1)
    assert np.array_equal(ar.surface(Pi, Ni), [True, False, False])
    import denoise_ref as dr
    ray = dr.pixel_rays(3, 1, *cam)[0]
    assert np.array_equal(Pi[0], ray[0:3] + F(2.0) * ray[3:6])
    assert np.array_equal(ar.ao_value(np.array([3, 48], np.uint32), 48), np.array([3, 48], np.float32) / F(48))


@pytest.mark.parametrize("scene", ["cornell_box.obj", "cornell_box_diffuse.obj"])
def test_cornell_box_on_the_oracle(oracle, scene):
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    cam = pt.initCamera()
    cam.setAspectRatio(np.float32(97) / np.float32(61))
    camera = (cam.eye(),) + tuple(cam.UVWFrame())
    params = ar.gpu_test_parameters(verts, idx)
    sc = oracle.scene(verts, idx, obj.getMaterialIndices(), obj.getMaterials())
    try:
        # the GPU tests' points and parameters: occluded and open rays alike, at every K they use
        P, N = ar.occlusion_points(verts, idx, camera)
        assert P.shape == (qr.SET_SIZE, 3) and ar.surface(P, N).all()
        assert np.abs((N.astype(np.float64) ** 2).sum(axis=1) - 1.0).max() <= 4 * np.finfo(np.float32).eps
        for K in (1, 2, 16, 256):
            n = qr.SET_SIZE if K <= 16 else 100
            r = ar.rays(P[:n], N[:n], pt.aoSamples(K), params)
            occ = sc.trace_any(r)
            print("%s K = %d: occluded share %.3f" % (scene, K, occ.mean()))
            assert occ.mean() >= 0.10 and (1 - occ).mean() >= 0.10, (K, occ.mean())
        # the floor (y = 0, normal +y).  The box is open to the front (z = 0) and the two blocks stand around the floor's centre, so:
        # the back corners, where two walls meet the floor, are darker than the floor's centre, and the front corners, with one wall
        # each, are darker than the middle of the front edge, which has none
        lo, hi = qr.scene_box(verts, idx)
        eps = F(0.02) * (hi - lo)
        cx, cz = F(0.5) * (lo[0] + hi[0]), F(0.5) * (lo[2] + hi[2])
        spots = np.array([[lo[0] + eps[0], 0, hi[2] - eps[2]], [hi[0] - eps[0], 0, hi[2] - eps[2]], [cx, 0, cz],
                          [lo[0] + eps[0], 0, lo[2] + eps[2]], [hi[0] - eps[0], 0, lo[2] + eps[2]], [cx, 0, lo[2] + eps[2]]], np.float32)
        K = 64
        r = ar.rays(spots, np.repeat(np.array([[0, 1, 0]], np.float32), 6, axis=0), pt.aoSamples(K), params)
        ao = ar.ao_value(ar.counts(sc.trace_any(r), r, K), K)
        print("%s floor: back corners %s centre %.3f, front corners %s front edge %.3f" % (scene, ao[0:2], ao[2], ao[3:5], ao[5]))
        assert (ao[0:2] < ao[2]).all() and (ao[3:5] < ao[5]).all()
        assert (ao[0:2] < ao[3:5]).all()
    finally:
        sc.close()


def test_vertex_normals():
    # a unit square in the plane z = 0 from two triangles of different area plus a fin: area weights, an unused vertex gets 0
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 5], [0, 0, 3]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3], [0, 5, 1]], np.uint32)
    n = pt.vertexNormals(verts, idx)
    assert n.dtype == np.float32 and n.shape == (6, 3)
    assert np.array_equal(n[2], [0, 0, 1]) and np.array_equal(n[3], [0, 0, 1]) and np.array_equal(n[4], [0, 0, 0])
    # vertex 0: two triangles of cross (0, 0, 1) each and the fin's cross((0, 0, 3), (1, 0, 0)) = (0, 3, 0)
    assert np.allclose(n[0], np.array([0, 3, 2]) / np.sqrt(13.0), atol=1e-7)
    assert np.array_equal(n[5], [0, 1, 0])
    assert np.array_equal(pt.vertexNormals(np.concatenate([verts, np.ones((6, 1), np.float32)], axis=1), idx.reshape(-1)), n)


def test_build_lists_and_abi():
    assert "ao.hip" in _build.HIP_SOURCES and "ao.h" in _build.HIP_HEADERS
    for name in ("ao.hip", "ao.h", "capi_query.hip", "traverse_hc.h"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert "pt_ao_points" in _native.ABI_SYMBOLS and "pt_ao_image" in _native.ABI_SYMBOLS
    import ctypes as C
    assert C.sizeof(_native.AoParams) == 32 and _native.AoParams.total_samples.offset == 20 and _native.AoParams.reserved.offset == 24
    assert _native.ABI_VERSION == 4


def test_wrapper_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    P = np.zeros((4, 3), np.float32)
    for args in ((np.zeros((4, 2), np.float32), P), (P, np.zeros((5, 3), np.float32)), (np.zeros(3, np.float32), np.zeros(3, np.float32)),
                 (np.zeros((4, 7), np.float32), None), (np.zeros((4, 3), np.float32), None)):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.bakeAO(state, *args)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.bakeAO(state, np.zeros((2, 3), np.complex64), np.zeros((2, 3), np.float32))
    assert pt.bakeAO(state, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).shape == (0,)
    assert pt.bakeAO(state, np.zeros((0, 8), np.float32)).dtype == np.float32
    for fn in (lambda **kw: pt.bakeAO(state, P, P, **kw), lambda **kw: pt.ambientOcclusion(state, **kw), lambda **kw: pt.AmbientOcclusion(**kw)):
        for disk, what in ((np.zeros((3, 3), np.float32), "a .K, 2. array"), (np.zeros((0, 2), np.float32), "1..256 points"), (np.zeros((257, 2), np.float32), "1..256 points"),
                           (np.array([[0.8, 0.7]], np.float32), "point 0 is outside"), (np.array([[0, 0], [np.nan, 0]], np.float32), "point 1 is outside"),
                           (np.array([[0, 0], [0, np.inf]], np.float32), "point 1 is outside")):
            with pytest.raises(pt.PathTracerError, match=what):
                fn(disk=disk)
        with pytest.raises(pt.PathTracerError, match="1..256"):
            fn(samples=0)
    for radius, bias, what in ((0.0, 0.0, "radius"), (-1.0, 0.0, "radius"), (np.inf, 0.0, "radius"), (np.nan, 0.0, "radius"), (1.0, -1e-3, "bias"), (1.0, np.nan, "bias"),
                               (1.0, np.inf, "bias")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.bakeAO(state, P, P, radius=radius, bias=bias)
        with pytest.raises(pt.PathTracerError, match=what):
            pt.ambientOcclusion(state, radius=radius, bias=bias)
    with pytest.raises(pt.PathTracerError, match="no scene"):
        pt.bakeVertexAO(state)
    with pytest.raises(pt.PathTracerError, match="update"):
        pt.AmbientOcclusion().visible()


def test_bakeao_refuses_unusable_tensors():
    torch = pytest.importorskip("torch")
    state = pt.PathTracerState()
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.bakeAO(state, torch.zeros((4, 8), dtype=torch.float32), radius=1.0, bias=0.0)          # host memory
    with pytest.raises(pt.PathTracerError, match="both"):
        pt.bakeAO(state, np.zeros((4, 3), np.float32), torch.zeros((4, 3), dtype=torch.float32), radius=1.0, bias=0.0)
