"""pt_query_closest / pt_query_any without a GPU: the NumPy statement of the hit record (tests/query_ref.py) against a float64
Moeller-Trumbore, the rays that are a miss before any traversal, the ray sets' hit and miss shares on the CPU oracle, and the
argument checks of queryRays that need no device."""
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import query_ref as qr

F = np.float32

# The largest |fp32 - float64| of a barycentric over _aimed_rays() below, measured once on the CPU (the figure DESIGN.md section 22
# quotes), and the bound the test holds the fp32 statement to: four times that.
BARY_MEASURED = 6.81e-6
BARY_BOUND = 4.0 * BARY_MEASURED


def _aimed_rays(n=4096, seed=7):
    """Random triangles of edge ~1 around points up to 10 from the origin, each with a ray from a random origin 0.5 .. 8 away, aimed
    at a point inside it (barycentrics u, v > 0.02, u + v < 0.98), the direction of random length 0.25 .. 4."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-10.0, 10.0, (n, 3))
    v = [(centre + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32) for _ in range(3)]
    b = rng.uniform(0.02, 0.96, (n, 2))
    fold = b.sum(axis=1) > 0.98
    b[fold] = 0.98 - b[fold]
    b = np.maximum(b, 0.02)
    target = v[0] + b[:, 0:1] * (v[1] - v[0]) + b[:, 1:2] * (v[2] - v[0])
    away = rng.normal(size=(n, 3))
    away /= np.sqrt((away * away).sum(axis=1, keepdims=True))
    o = (target + away * rng.uniform(0.5, 8.0, (n, 1))).astype(np.float32)
    d = ((target - o) * rng.uniform(0.25, 4.0, (n, 1)) / np.sqrt(((target - o) ** 2).sum(axis=1, keepdims=True))).astype(np.float32)
    # leave out grazing rays: |cos| between the ray and the triangle's normal below 0.1 (the barycentrics' condition number grows as 1 / cos)
    nrm = np.cross(v[1].astype(np.float64) - v[0], v[2].astype(np.float64) - v[0])
    cos = np.abs((nrm * d).sum(axis=1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(d.astype(np.float64), axis=1))
    keep = (cos >= 0.1) & (np.linalg.norm(nrm, axis=1) >= 0.2)
    return o[keep], d[keep], v[0][keep], v[1][keep], v[2][keep]


def test_fp32_barycentrics_against_float64():
    o, d, v0, v1, v2 = _aimed_rays()
    assert o.shape[0] >= 2000
    u, v = qr.barycentrics(o, d, v0, v1 - v0, v2 - v0)
    assert u.dtype == np.float32 and v.dtype == np.float32
    u64, v64 = qr.barycentrics_f64(o, d, v0, v1, v2)
    assert (u64 > 0.0).all() and (v64 > 0.0).all() and (u64 + v64 < 1.0).all()       # the rays hit where they were aimed
    worst = max(np.abs(u - u64).max(), np.abs(v - v64).max())
    print("largest |fp32 - float64| barycentric deviation over %d rays: %.3e (bound %.3e)" % (o.shape[0], worst, BARY_BOUND))
    assert worst <= BARY_BOUND
    assert worst >= BARY_MEASURED / 4.0          # the figure quoted is this set's, not a stale one


def test_hit_record_layout_and_epilogue():
    """One triangle, hand-checked: barycentrics of v1 and v2, the normal towards the origin from either side, the material mask."""
    verts = np.array([[0, 0, 0, 1], [2, 0, 0, 1], [0, 2, 0, 1]], np.float32)
    idx = np.array([0, 1, 2], np.uint32)
    rays = np.array([[0.5, 0.25, 1.0, 0, 0, -1, 0, 10], [0.5, 0.25, -3.0, 0, 0, 2, 0, 10]], np.float32)
    rec = qr.hit_records(rays, np.array([1.0, 1.5], np.float32), np.array([0, 0], np.uint32), verts, idx, np.array([0x05000007], np.uint32))
    f = rec.view(np.float32)
    assert np.array_equal(f[:, 0], [1.0, 1.5]) and np.array_equal(rec[:, 1], [0, 0])
    assert np.array_equal(f[:, 2], [0.25, 0.25]) and np.array_equal(f[:, 3], [0.125, 0.125])
    assert np.array_equal(f[0, 4:7], [0, 0, 1]) and np.array_equal(f[1, 4:7], [0, 0, -1])
    assert np.array_equal(rec[:, 7], [7, 7])
    miss = qr.hit_records(rays, np.array([-1.0, -1.0], np.float32), np.array([0xFFFFFFFF] * 2, np.uint32), verts, idx, np.array([0], np.uint32))
    assert np.array_equal(miss, qr.miss_records(2))
    assert np.array_equal(qr.miss_records(1)[0], np.array([0xBF800000, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0xFFFFFFFF], np.uint32))
    assert pt.HIT_DTYPE.itemsize == 32 and [pt.HIT_DTYPE.fields[k][1] for k in pt.HIT_DTYPE.names] == [0, 4, 8, 16, 28]


def test_rays_that_miss_before_any_traversal():
    good = np.array([1.0, 2.0, 3.0, 0.0, 0.0, -1.0, 0.001, 50.0], np.float32)
    bad, why = qr.bad_rays(good)
    assert bad.shape[0] == 3 * 8 - 2 + 3
    ok = qr.traceable(bad)
    assert not ok.any(), [w for w, k in zip(why, ok) if k]
    allowed = np.array([good, good, good, good], np.float32)
    allowed[1, 7] = np.inf          # an unbounded ray
    allowed[2, 6] = -np.inf         # ... on both sides
    allowed[3, 3:6] = 0.0           # a zero direction goes through the traversal: the triangle test rejects det == 0
    assert qr.traceable(allowed).all()
    # whatever {t, prim} claims, a bad ray's record is the miss record
    verts = np.array([[0, 0, 0, 1], [9, 0, 0, 1], [0, 9, 0, 1]], np.float32)
    rec = qr.hit_records(bad, np.full(bad.shape[0], 3.0, np.float32), np.zeros(bad.shape[0], np.uint32), verts, np.array([0, 1, 2], np.uint32), np.zeros(1, np.uint32))
    assert np.array_equal(rec, qr.miss_records(bad.shape[0]))
    # ... and so is every record of a scene without triangles
    rec = qr.hit_records(allowed, np.full(4, 3.0, np.float32), np.zeros(4, np.uint32), verts, np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert np.array_equal(rec, qr.miss_records(4))


@pytest.mark.parametrize("scene", ["cornell_box.obj", "cornell_box_diffuse.obj"])
def test_ray_sets_hit_and_miss_on_the_oracle(oracle, scene):
    """The shares the GPU tests rely on, by the oracle's brute force: at least a quarter of every set hits and at least a tenth
    misses, except the set that leaves the scene, which misses throughout; and any-hit agrees with closest-hit."""
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
    cam = pt.initCamera()
    cam.setAspectRatio(np.float32(97) / np.float32(61))
    sc = oracle.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    try:
        for name in qr.RAY_SETS:
            rays = qr.ray_set(name, obj.getVerticesFloat(), obj.getIndexBuffer(), (cam.eye(),) + tuple(cam.UVWFrame()))
            assert rays.shape == (qr.SET_SIZE, 8) and rays.dtype == np.float32 and qr.traceable(rays).all()
            t, prim = sc.trace_closest(rays)
            hit = prim != 0xFFFFFFFF
            assert np.array_equal(sc.trace_any(rays).astype(bool), hit)
            if name == "outside":
                assert not hit.any()
            else:
                assert hit.mean() >= 0.25 and (~hit).mean() >= 0.10, (name, hit.mean())
            if name == "in_wall_planes":
                assert ((rays[:, 3:6] == 0.0).sum(axis=1) == 2).all()
            if not hit.any():
                continue
            # the record of every hit is a point of its triangle.  The slack, 1e-3, is no measured bound: it is some hundred times
            # the statement's error on well-conditioned rays (above), there for grazing rays; swapped vertices or barycentrics are off by O(1)
            rec = qr.hit_records(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()).view(np.float32)
            u, v = rec[hit, 2], rec[hit, 3]
            assert (u >= -1e-3).all() and (v >= -1e-3).all() and (u + v <= 1.0 + 1e-3).all()
            assert np.abs((rec[hit, 4:7].astype(np.float64) ** 2).sum(axis=1) - 1.0).max() <= 4 * np.finfo(np.float32).eps      # a unit normal: three roundings
    finally:
        sc.close()


def test_build_lists():
    assert "query.hip" in _build.HIP_SOURCES and "capi_query.hip" in _build.HIP_SOURCES
    assert "query.h" in _build.HIP_HEADERS and "traverse_hc.h" in _build.HIP_HEADERS
    for name in ("query.hip", "query.h", "traverse_hc.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert "pt_query_closest" in _native.ABI_SYMBOLS and "pt_query_any" in _native.ABI_SYMBOLS


def test_queryrays_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for bad in (np.zeros((4, 7), np.float32), np.zeros(8, np.float32), np.zeros((2, 8, 1), np.float32), [[1, 2, 3]]):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.queryRays(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.queryRays(state, np.zeros((2, 8), np.complex64))
    # no rays: an empty answer of the right shape, without a device
    empty = pt.queryRays(state, np.zeros((0, 8), np.float32))
    assert sorted(empty) == ["material", "normal", "prim", "t", "uv"]
    assert empty["t"].shape == (0,) and empty["uv"].shape == (0, 2) and empty["normal"].shape == (0, 3) and empty["prim"].dtype == np.uint32
    assert pt.queryRays(state, np.zeros((0, 8), np.float32), any_hit=True).dtype == np.bool_


def test_queryrays_refuses_unusable_tensors():
    torch = pytest.importorskip("torch")
    state = pt.PathTracerState()
    cpu = torch.zeros((4, 8), dtype=torch.float32)
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.queryRays(state, cpu)                                    # another device: host memory
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        with pytest.raises(pt.PathTracerError, match="float32"):
            pt.queryRays(state, torch.zeros((4, 8), dtype=torch.float64, device=dev))
        with pytest.raises(pt.PathTracerError, match="contiguous"):
            pt.queryRays(state, torch.zeros((8, 4), dtype=torch.float32, device=dev).t())
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.queryRays(state, torch.zeros((4, 6), dtype=torch.float32, device=dev))
