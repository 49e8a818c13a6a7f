"""pt_query_winding without a GPU: tests/winding_ref.py's brute force on closed forms (cube, tetrahedron), the moments of hand-built
trees by hand, the accept rule at its boundary, a zero-area node, the empty child, beta = +inf against the brute force, the icosphere
figures the contract quotes; the share of near-surface points the GPU tests leave out; the build lists, the ABI, the kernels'
registers; the wrappers' argument checks."""
import os
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import multihit_ref as mr
import nearest_ref as nr
import winding_ref as wr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_FILES = ("cornell_box.obj", "cornell_box_diffuse.obj")
NEAR_REL = 1e-3                 # points closer to the surface than this share of the scene's diagonal are left out of value comparisons
VALUE_SETS = ("inside", "shell")          # `features` sits on the surface (vertices, edges): decisions and finiteness only


def _v4(rows):
    v = np.zeros((len(rows), 4), np.float32)
    v[:, :3] = rows
    return v


CUBE_V = _v4([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
# outward winding, two triangles per face: -z, +z, -y, +y, -x, +x
CUBE_I = np.array([0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 3, 7, 6, 3, 6, 2, 0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5], np.uint32)
TET_V = _v4([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)])
TET_I = np.array([0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2], np.uint32)


def median_tree(verts, idx):
    """(children int32 [n - 1, 2], empty bool, records [n, 12]) of a median-split tree over the triangles' centroids, nodes numbered
    in preorder, leaf slots in triangle order; one triangle: the build's one node with an empty second child"""
    rec = wr.records_of_scene(verts, idx)
    v0, v1, v2 = wr.record_vertices(rec)
    cen = (v0.astype(np.float64) + v1 + v2) / 3.0
    n = len(rec)
    if n == 1:
        return np.array([[-1, -1]], np.int32), np.array([[False, True]]), rec
    children = np.zeros((n - 1, 2), np.int32)
    nxt = [0]

    def build(ids):
        if len(ids) == 1:
            return ~int(ids[0])
        me = nxt[0]; nxt[0] += 1
        ext = cen[ids].max(axis=0) - cen[ids].min(axis=0)
        order = ids[np.argsort(cen[ids, int(np.argmax(ext))], kind="stable")]
        half = len(order) // 2
        children[me, 0] = build(order[:half])
        children[me, 1] = build(order[half:])
        return me

    build(np.arange(n))
    return children, np.zeros((n - 1, 2), bool), rec


def test_closed_forms():
    centre = np.array([[0.5, 0.5, 0.5]], F)
    assert abs(wr.exact(centre, CUBE_V, CUBE_I)[0] - 1.0) < 1e-14
    for face in range(6):                                   # the two triangles of one face: a sixth of the sphere
        assert abs(wr.exact(centre, CUBE_V, CUBE_I[6 * face:6 * face + 6])[0] - 1.0 / 6.0) < 1e-14, face
    outside = np.array([[2.0, 0.3, 0.4], [0.5, 0.5, -3.0], [-1.0, -1.0, -1.0]], F)
    assert np.abs(wr.exact(outside, CUBE_V, CUBE_I)).max() < 1e-14
    origin = np.zeros((1, 3), F)
    assert abs(wr.exact(origin, TET_V, TET_I)[0] - 1.0) < 1e-14
    for face in range(4):
        assert abs(wr.exact(origin, TET_V, TET_I[3 * face:3 * face + 3])[0] - 0.25) < 1e-14, face
    flipped = TET_I.reshape(-1, 3)[:, ::-1].reshape(-1)
    assert abs(wr.exact(origin, TET_V, flipped)[0] + 1.0) < 1e-14
    assert abs(wr.exact(centre, CUBE_V, CUBE_I.reshape(-1, 3)[:, [0, 2, 1]].reshape(-1))[0] + 1.0) < 1e-14
    # float32, sequential: the same to fp32's precision; a bad point is a NaN and stops nobody else
    w32 = wr.exact(np.array([[0.5, 0.5, 0.5], [np.nan, 0, 0], [2.0, 0.3, 0.4], [0, np.inf, 0]], F), CUBE_V, CUBE_I, np.float32)
    assert w32.dtype == np.float32 and abs(w32[0] - 1) < 1e-6 and abs(w32[2]) < 1e-6 and np.isnan(w32[1]) and np.isnan(w32[3])
    # at a vertex, on an edge, in a face: finite
    on = np.array([[0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]], F)
    assert np.isfinite(wr.exact(on, CUBE_V, CUBE_I)).all() and np.isfinite(wr.exact(on, CUBE_V, CUBE_I, np.float32)).all()
    # no triangles
    assert not wr.exact(centre, CUBE_V, np.zeros(0, np.uint32)).any()


def test_moments_of_hand_built_trees():
    # two right triangles of the unit square in z = 0: areas 1/2, normals (0, 0, 1/2), centroids (1/3, 1/3), (2/3, 2/3)
    v = _v4([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)])
    rec = wr.records_of_scene(v, np.array([0, 1, 2, 1, 3, 2], np.uint32))
    m = wr.moments(np.array([[-1, -2]]), np.zeros((1, 2), bool), rec)
    third = F(F(1.0) / F(3.0))
    c0 = F(0.0) + third
    assert m.shape == (1, 8) and m.dtype == np.float32
    sx = F(F(0.5) * c0) + F(F(0.5) * F(F(1.0) + F(F(-1.0) / F(3.0))))
    assert m[0, 7] == 1.0 and np.array_equal(m[0, 4:7], [0, 0, 1]) and m[0, 0] == sx and m[0, 2] == 0
    assert abs(m[0, 0] - 0.5) < 1e-6 and abs(m[0, 1] - 0.5) < 1e-6
    far = np.maximum(m[0, 0:3] - F(0), F(1) - m[0, 0:3]); far[2] = 0
    assert m[0, 3] == F(F(far[0] * far[0]) + F(far[1] * far[1]))
    # three triangles: node 1 = {triangle 1, triangle 2} under node 0 = {triangle 0, node 1}; the third is twice the size, in z = 2
    v = _v4([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 2), (2, 0, 2), (0, 2, 2)])
    rec = wr.records_of_scene(v, np.array([0, 1, 2, 1, 3, 2, 4, 5, 6], np.uint32))
    ch = np.array([[-1, 1], [-2, -3]])
    m = wr.moments(ch, np.zeros((2, 2), bool), rec)
    assert m[1, 7] == 2.5 and np.array_equal(m[1, 4:7], [0, 0, 2.5]) and m[0, 7] == 3.0 and np.array_equal(m[0, 4:7], [0, 0, 3])
    # node 1: S = 0.5 * c1 + 2 * c2, p = S / 2.5; its box is [0, 2] x [0, 2] x [0, 2]
    tn, ta, ts, tlo, thi = wr.triangle_sums(rec)
    s1 = (ts[1] + ts[2]).astype(F)
    assert np.array_equal(m[1, 0:3], (s1 / F(2.5)).astype(F)) and abs(m[1, 2] - 1.6) < 1e-6
    s0 = (ts[0] + s1).astype(F)                              # child 0 first
    assert np.array_equal(m[0, 0:3], (s0 / F(3.0)).astype(F))
    d = np.maximum(m[1, 0:3], F(2) - m[1, 0:3])
    assert m[1, 3] == F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))
    # a sum of two commutes in IEEE arithmetic: swapping every node's children gives the same bits, which is why combining exactly two
    # stored values per node makes the moments independent of the schedule (and why no test can tell child 1 + child 0 from the rule)
    verts, idx = mr.icosphere(1, (0.3, -0.2, 0.7), 1.3)
    children, empty, rec = median_tree(verts, idx)
    a = wr.moments(children, empty, rec)
    b = wr.moments(children[:, ::-1], empty, rec)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... while another tree over the same triangles is another set of sums
    other = wr.moments(*median_tree(verts, idx.reshape(-1, 3)[::-1].reshape(-1))[:2], rec[::-1])
    assert a[0, 7] != 0 and abs(a[0, 7] - other[0, 7]) < 1e-4


def test_zero_area_and_the_empty_child():
    # every triangle collapsed: A = 0, p is the centre of the box, N = 0; the walk never divides by the area
    v = _v4([(0, 0, 0), (2, 0, 0), (4, 0, 0), (1, 1, 1), (1, 1, 1)])
    rec = wr.records_of_scene(v, np.array([0, 1, 2, 3, 3, 4], np.uint32))
    m = wr.moments(np.array([[-1, -2]]), np.zeros((1, 2), bool), rec)
    assert m[0, 7] == 0 and not m[0, 4:7].any() and np.array_equal(m[0, 0:3], [2, 0.5, 0.5]) and m[0, 3] == F(4 + 0.25 + 0.25)
    vis, w = wr.walk(np.array([[-1, -2]]), np.zeros((1, 2), bool), m, rec, np.array([[9, 9, 9], [2, 0.5, 0.5]], F), 2.0)
    assert np.isfinite(w).all() and not w.any() and vis.tolist() == [[1, 0], [0, 2]]
    # one triangle: the node references it twice, the second reference is empty — once, not twice
    v = _v4([(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    one = np.array([0, 1, 2], np.uint32)
    children, empty, rec = median_tree(v, one)
    m = wr.moments(children, empty, rec)
    tn, ta, ts, tlo, thi = wr.triangle_sums(rec)
    assert m[0, 7] == ta[0] == 0.5 and np.array_equal(m[0, 4:7], tn[0])
    q = np.array([[0.2, 0.2, 0.5], [0.2, 0.2, -0.5], [30, 40, 50]], F)
    vis, w = wr.walk(children, empty, m, rec, q, 2.0)
    assert vis.tolist() == [[0, 1], [0, 1], [1, 0]]
    assert np.allclose(w[:2], wr.exact(q[:2], v, one), rtol=0, atol=1e-15) and w[1] > 0.05 and w[0] == -w[1]      # the normal points at q[0]: seen from outside
    assert abs(w[2] - wr.exact(q[2:], v, one)[0]) < 1e-6
    twice = wr.walk(children, np.zeros((1, 2), bool), m, rec, q[:1], 2.0)
    assert twice[0].tolist() == [[0, 2]] and abs(twice[1][0] - 2 * w[0]) < 1e-15 and twice[1][0] != 0          # what the mark is there to prevent


def test_the_accept_rule_is_strict_and_fp32():
    # a square of side 6 around the origin: the centroids (1, -1) and (-1, 1) are exact, both areas 18
    v = _v4([(-3, -3, 0), (3, -3, 0), (3, 3, 0), (-3, 3, 0)])
    rec = wr.records_of_scene(v, np.array([0, 1, 2, 0, 2, 3], np.uint32))
    ch, em = np.array([[-1, -2]]), np.zeros((1, 2), bool)
    m = wr.moments(ch, em, rec)
    assert np.array_equal(m[0], [0, 0, 0, 18, 0, 0, 36, 36])         # p = the origin, r2 = 9 + 9
    # beta = 2: d2 > 72.  (0, 6, 6): d2 == 72 exactly, not taken; one step further it is (36 + 2 ulp, then 72 + 1 ulp)
    q = np.array([[0, 6, 6], [0, 6, np.nextafter(F(6), F(7))], [0, 6, np.nextafter(F(6), F(5))]], F)
    vis, w = wr.walk(ch, em, m, rec, q, 2.0)
    assert vis.tolist() == [[0, 2], [1, 0], [0, 2]]
    assert wr.accepts(m[0], q, F(4.0))[0].tolist() == [False, True, False]
    # beta = 1 is the smallest legal value; +inf takes nothing, not even where r2 is 0 (inf * 0 is a NaN, the compare is false)
    assert wr.walk(ch, em, m, rec, q, 1.0)[0].tolist() == [[1, 0]] * 3
    assert wr.walk(ch, em, m, rec, q, np.inf)[0].tolist() == [[0, 2]] * 3
    point = m.copy(); point[0, 3] = 0
    assert wr.walk(ch, em, point, rec, q, np.inf)[0].tolist() == [[0, 2]] * 3 and wr.walk(ch, em, point, rec, q, 1e18)[0].tolist() == [[1, 0]] * 3
    # bad points: no traversal, a NaN, and the good ones beside them are untouched
    mixed = np.array([[0, 6, 6], [np.nan, 0, 0], [0, 15, 15], [0, -np.inf, 0]], F)
    vis, w = wr.walk(ch, em, m, rec, mixed, 2.0)
    assert vis.tolist() == [[0, 2], [0, 0], [1, 0], [0, 0]] and np.isnan(w[[1, 3]]).all() and np.isfinite(w[[0, 2]]).all()


@pytest.fixture(scope="module")
def sphere():
    """the icosphere of the contract at subdivision 2, its shell points, and a median-split tree over it: closed and without its
    first 8 triangles"""
    centre, radius = (0.0, 0.0, 0.0), 1.0
    verts, idx = mr.icosphere(2, centre, radius)
    pts, inside = mr.shell_points(1000, centre, radius)
    return verts, idx.reshape(-1), pts, inside


def test_beta_inf_is_the_exact_sum_and_the_icosphere_figures(sphere):
    verts, idx, pts, inside = sphere
    assert len(idx) == 3 * 320
    closed = wr.exact(pts, verts, idx)
    assert np.abs(closed[inside] - 1).max() < 1e-13 and np.abs(closed[~inside]).max() < 1e-13
    holed_idx = idx[3 * 8:]
    holed = wr.exact(pts, verts, holed_idx)
    print("holed icosphere: smallest w inside %.4f, largest outside %.4f" % (holed[inside].min(), holed[~inside].max()))
    assert round(float(holed[inside].min()), 2) == 0.74 and round(float(holed[~inside].max()), 2) == 0.09
    assert ((holed > 0.5) == inside).all()
    # float32 against float64: the E32 the GPU test's bar is made of
    e32 = np.abs(wr.exact(pts, verts, idx, np.float32).astype(np.float64) - closed).max()
    print("E32 at 320 triangles: %.3g" % e32)
    assert 2.0 ** -23 < e32 < 4e-6                            # a sequential fp32 sum of 320 terms that add up to 4 pi
    for which in (idx, holed_idx):
        children, empty, rec = median_tree(verts, which)
        m = wr.moments(children, empty, rec)
        ref = wr.exact(pts, verts, which)
        vis, w = wr.walk(children, empty, m, rec, pts, np.inf)
        assert (vis[:, 0] == 0).all() and (vis[:, 1] == len(which) // 3).all()
        assert np.abs(w - ref).max() < 1e-13                     # another order of the same terms
        vis, w2 = wr.walk(children, empty, m, rec, pts, 2.0)
        err = np.abs(w2 - ref).max()
        print("first order at beta = 2: off by at most %.4f; mean dipoles %.1f, triangles %.1f" % (err, vis[:, 0].mean(), vis[:, 1].mean()))
        assert err <= 0.03 and ((w2 > 0.5) == inside).all()
        assert (vis[:, 1] < len(which) // 3).any() and (vis[:, 0] > 0).any()
        tighter = np.abs(wr.walk(children, empty, m, rec, pts, 8.0)[1] - ref).max()
        assert tighter < err


def test_near_surface_share_of_the_sets_the_gpu_test_compares_values_on(built, sphere):
    """Points closer to the surface than 1e-3 of the scene's diagonal are left out of the value comparison: under 5 % of each set"""
    cam = pt.initCamera()
    cam.setAspectRatio(np.float32(97) / np.float32(61))
    camera = (cam.eye(),) + tuple(cam.UVWFrame())
    for scene in SCENE_FILES:
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
        verts, idx, mats = obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()
        lo, hi = nr.scene_box(verts, idx)
        diag = float(np.linalg.norm(hi.astype(np.float64) - lo))
        for name in VALUE_SETS:
            pts = nr.point_set(name, verts, idx, camera)
            rec = nr.nearest_records(nr.with_radius(pts, np.inf), verts, idx, mats)
            share = float((rec.view(np.float32)[:, 0] < NEAR_REL * diag).mean())
            print("%s %s: %.3f of the points within %g of the surface" % (scene, name, share, NEAR_REL * diag))
            assert share < 0.05, (scene, name, share)
    verts, idx, pts, inside = sphere
    r = np.linalg.norm(pts.astype(np.float64), axis=1)
    assert (np.abs(r - 1.0) >= 0.02 - 1e-6).all()                # the shell points keep 2 % of the radius: 1e-3 of the diagonal is 0.35 %


# ---- the layers ---------------------------------------------------------------------------------------------------------------------
def test_build_lists_and_abi():
    assert "winding.hip" in _build.HIP_SOURCES and "winding.h" in _build.HIP_HEADERS
    for name in ("winding.hip", "winding.h", "capi_query.hip", "context.h"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    assert "pt_query_winding" in _native.ABI_SYMBOLS and "pt_get_winding_info" in _native.ABI_SYMBOLS
    assert "pt_debug_winding_visits" in _native.TEST_SYMBOLS and "pt_debug_read_winding" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4 and _native.WINDING_BETA_DEFAULT == wr.BETA_DEFAULT == 2.0
    import ctypes as C
    assert C.sizeof(_native.BvhInfo) == 88 and C.sizeof(_native.WindingInfo) == 16
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert "#define PT_WINDING_BETA_DEFAULT 2.0f" in hdr
    assert "int pt_query_winding(pt_ctx* ctx, const float* points, size_t n, float beta, float* out);" in hdr
    assert "int pt_get_winding_info(pt_ctx* ctx, pt_winding_info* out);" in hdr


def test_winding_kernels_use_no_scratch_memory_and_spill_nothing(built):
    """The walk and its counting twin, and the four kernels of the moment build: no private segment, no spilled vector or scalar
    register"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    table = kernel_meta.kernel_table(_native.hip_library_path())
    walks = [k for k in table if "k_query_winding<" in k["name"]]
    build = [k for k in table if "k_wd_" in k["name"]]
    assert len(walks) == 2 and len(build) == 4, ([k["name"] for k in walks], [k["name"] for k in build])
    for k in walks + build:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


def test_querywinding_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    ok = np.zeros((2, 3), np.float32)
    for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros((2, 4, 1), np.float32), [[1, 2]]):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.queryWinding(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.queryWinding(state, ok.astype(np.complex64))
    for bad in (0.5, -2.0, float("nan"), "wide", None):
        with pytest.raises(pt.PathTracerError, match="beta"):
            pt.queryWinding(state, ok, beta=bad)
    for n in (3, 4):
        got = pt.queryWinding(state, np.zeros((0, n), np.float32), beta=float("inf"))
        assert got.shape == (0,) and got.dtype == np.float32
    with pytest.raises(pt.PathTracerError, match="method"):
        pt.pointsInside(state, ok, method="votes")
    with pytest.raises(pt.PathTracerError, match="\\(n, 3\\) points"):
        pt.pointsInside(state, np.zeros((2, 4), np.float32), method="winding")
    with pytest.raises(pt.PathTracerError, match="threshold"):
        pt.pointsInside(state, ok, method="winding", threshold="half")
    with pytest.raises(pt.PathTracerError, match="beta"):
        pt.pointsInside(state, ok, method="winding", beta=0.0)
    inside, w = pt.pointsInside(state, np.zeros((0, 3), np.float32), method="winding", return_counts=True)
    assert inside.shape == (0,) and inside.dtype == bool and w.dtype == np.float32
    with pytest.raises(pt.PathTracerError, match="signed"):
        pt.bakeDistanceField(state, (2, 2, 2), bounds=((0, 0, 0), (1, 1, 1)), signed="parity")
