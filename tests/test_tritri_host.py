"""pt_query_triangles without a GPU: the NumPy statement of the triangle-triangle test (tests/tritri_ref.py) on hand-checked triangles,
the miss table, the list rule, the 17 axes against two independent float64 tests, fp32 against the same algorithm in float64, the
query sets' shares on the Cornell fixtures, the argument checks of queryTriangles, triangleRecords and meshCollisions that need no
device, and the registers of the built kernels."""
import os
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import nearest_ref as nr
import tritri_ref as tt

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fp32 against float64.  A pair (query, scene triangle) on which the two differ must be a contact: in float64 its smallest normalised
# gap — every condition as a signed distance, an axis' conditions divided by |L|, axes of length 0 left out — is close to 0 from
# either side.  The largest |gap| over every differing pair of FP64_SETS on the Cornell box, relative to the scene's largest
# |coordinate| S, measured once on the CPU (the figure DESIGN.md section 29 quotes), and the bound the test holds the fp32 statement
# to: four times that.
FP64_SETS = ("random", "self", "edge", "coplanar", "wall_touch")
GAP_MEASURED = 9.82e-9
GAP_BOUND = 4.0 * GAP_MEASURED

# A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0)
TRI = (np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32), np.array([0, 1, 2], np.uint32))


def _one(q, verts=TRI[0], idx=TRI[1]):
    q = np.array(q, np.float32)
    m = tt.intersect_matrix(tt.as_records(q[None]), verts, idx)
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    g = tt.conditions(q[0], q[1], q[2], v0[0], e1[0], e2[0])
    return bool(m[0, 0]), tuple(bool(g[k]) for k in tt.GROUPS)


def test_hand_checked_triangles_against_one_triangle():
    """Every value below is exact in fp32.  (intersects, (boxes, normals, edges, in_a, in_b)): which groups of conditions separate"""
    all_keep = (True,) * 5
    cases = [
        (((1, 1, -1), (2, 1, 1), (1, 2, 1)), True, all_keep),                                   # piercing the face
        (((1, 1, 0), (2, 1, 1), (1, 2, 1)), True, all_keep),                                    # a vertex resting in the face: touching counts
        (((1, 1, 0.0625), (2, 1, 1), (1, 2, 1)), False, (False, False, False, True, True)),     # a sixteenth above it: z ranges apart
        (((4, 0, 0), (5, 0, 1), (5, 1, 1)), True, all_keep),                                    # touching vertex B with a vertex
        (((4.0625, 0, 0), (5, 0, 1), (5, 1, 1)), False, (False,) * 5),                          # a sixteenth short of it
        (((2, 0, 0), (2, -1, 1), (3, -1, 1)), True, all_keep),                                  # a vertex on edge AB
        (((2, -0.0625, 0), (2, -1, 1), (3, -1, 1)), False, (False,) * 5),                       # a sixteenth short of it
        (((2, 2, 0), (4, 4, 1), (4, 4, -1)), True, all_keep),                                   # in the plane x = y, its tip on edge BC
        (((2.0625, 2.0625, 0), (4, 4, 1), (4, 4, -1)), False, (True, True, False, False, False)),   # the tip beyond BC, inside the bounding box
        (((1, 1, 0), (3, 1, 0), (1, 3, 0)), True, all_keep),                                    # coplanar, overlapping
        (((4, 0, 0), (6, 0, 0), (4, 2, 0)), True, all_keep),                                    # coplanar, touching at B
        # coplanar and apart beyond BC, inside the bounding box: the normals project everything to 0 and the nine edge products are
        # parallel to them; only the in-plane axes separate
        (((3, 3, 0), (5, 3, 0), (3, 5, 0)), False, (True, True, True, False, False)),
        # the case only the edge-edge axes reject: one vertex in the plane z = 0 at (1, 4), outside the triangle, the others above it
        (((-2, 1, 3), (1, 4, 0), (3, 4, 6)), False, (True, True, False, True, True)),
        # the case only a normal rejects: an edge in the plane z = 0 along y = 4 + (x + 3) / 2, beyond C, the third vertex above
        (((-3, 4, 0), (1, 6, 0), (-1, -1, 5)), False, (True, False, True, True, True)),
    ]
    for q, want, groups in cases:
        got, g = _one(q)
        assert got == want and g == groups, (q, got, g)
    # documented behaviour, not exactness: a segment in the triangle's plane that passes A at a distance (on the line x + 2 y = -1) is
    # kept, because the only line that separates the two in that plane is the segment's own, and cross(nA, edge) = 0 for nA = 0
    seg = ((-3, 1, 0), (1, -1, 0), (1, -1, 0))
    assert _one(seg) == (True, all_keep)
    p = np.array(seg, np.float64)
    assert (p[:, 0] + 2.0 * p[:, 1] == -1.0).all() and (TRI[0][:, 0] + 2.0 * TRI[0][:, 1] >= 0.0).all()      # and apart they are
    # the same segment with an area (a third vertex on the far side of its line) is rejected by its own in-plane axis
    assert _one(((-3, 1, 0), (1, -1, 0), (-3, -1, 0))) == (False, (True, True, True, False, True))
    # zero-area scene triangles are tested like any other and never miss: the collapsed edge A-B-A, pierced and passed
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [2, 0, 0, 1]], np.float32)
    assert _one(((3, -1, -1), (3, 1, -1), (3, 0, 2)), verts)[0] is True
    assert _one(((5, -1, -1), (5, 1, -1), (5, 0, 2)), verts)[0] is False


def test_the_miss_table():
    good = tt.as_records(np.array([[[1, 1, -1], [2, 1, 1], [1, 2, 1]]], np.float32))[0]
    assert tt.triangle_records(good[None], *TRI)[0].tolist() == [1]
    bad, why = tt.bad_triangles(good)
    assert bad.shape == (27, 12) and not tt.searchable(bad).any(), [w for w, s in zip(why, tt.searchable(bad)) if s]
    counts, prims, hit = tt.triangle_records(bad, *TRI, max_prims=4)
    assert not counts.any() and (prims == 0xFFFFFFFF).all() and not hit.any()
    # the reserved floats are not looked at; a point and a segment are triangles; the largest finite coordinates are coordinates
    odd = good[None].repeat(4, axis=0)
    odd[0, [3, 7, 11]] = (np.nan, np.inf, -7.0)
    odd[1] = tt.as_records(np.array([[[1, 1, 0]] * 3], np.float32))[0]
    odd[2] = tt.as_records(np.array([[[1, 1, -1], [1, 1, 1], [1, 1, 1]]], np.float32))[0]
    odd[3] = tt.as_records(np.array([[[-3e38, -3e38, -3e38], [3e38, 3e38, 3e38], [3e38, -3e38, 3e38]]], np.float32))[0]
    assert tt.searchable(odd).all()
    counts, prims, hit = tt.triangle_records(odd, *TRI, max_prims=2)
    assert counts[:3].tolist() == [1, 1, 1] and hit[:3].tolist() == [1, 1, 1] and prims[:3].tolist() == [[0, 0xFFFFFFFF]] * 3
    # a scene without triangles
    counts, prims, hit = tt.triangle_records(odd, np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), max_prims=3)
    assert counts.shape == (4,) and not counts.any() and prims.shape == (4, 3) and (prims == 0xFFFFFFFF).all() and not hit.any()
    # three NaN projections fail their condition: a scene triangle with a NaN vertex 0 intersects nothing
    verts = np.array([[np.nan, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32)
    assert not tt.triangle_records(odd, verts, TRI[1])[0].any()


def test_the_list_rule():
    """Twelve copies of the triangle, of which a query pierces those with an even index: the count is not clamped, the list holds the
    lowest max_prims indices ascending and 0xFFFFFFFF behind them"""
    verts = np.concatenate([TRI[0] + np.array([0, 0, 10.0 * (k % 2), 0], np.float32) for k in range(12)])
    idx = np.arange(36, dtype=np.uint32)
    q = np.array([[[1, 1, -1], [2, 1, 1], [1, 2, 1]], [[1, 1, 9], [2, 1, 11], [1, 2, 11]], [[1, 1, 4], [2, 1, 6], [1, 2, 6]], [[1, 1, -1], [1, 1, 11], [1.5, 1.5, 5]]], np.float32)
    for k in range(0, tt.MAX_PRIMS + 1):
        counts, prims, hit = tt.triangle_records(tt.as_records(q), verts, idx, max_prims=k)
        assert counts.tolist() == [6, 6, 0, 12] and hit.tolist() == [1, 1, 0, 1] and prims.shape == (4, k) and prims.dtype == np.uint32
        full = [[0, 2, 4, 6, 8, 10, 0xFFFFFFFF, 0xFFFFFFFF], [1, 3, 5, 7, 9, 11, 0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF] * 8, list(range(8))]
        assert prims.tolist() == [row[:k] for row in full]


# ---- the 17 axes against tests that know nothing of separating axes, in float64 ---------------------------------------------------

def _segment_hits_triangle(p, q, a, b, c):
    """bool [n]: does the segment p q cross the triangle a b c (Moeller-Trumbore, closed)"""
    d, e1, e2 = q - p, b - a, c - a
    h = np.cross(d, e2)
    det = (e1 * h).sum(axis=1)
    with np.errstate(all="ignore"):
        s = p - a
        u = (s * h).sum(axis=1) / det
        qq = np.cross(s, e1)
        v = (d * qq).sum(axis=1) / det
        t = (e2 * qq).sum(axis=1) / det
    return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)


def _pierce_test(A, B):
    """bool [n]: an edge of one triangle crosses the face of the other; A, B [n, 3, 3]"""
    hit = np.zeros(A.shape[0], bool)
    for X, Y in ((A, B), (B, A)):
        for i in range(3):
            hit |= _segment_hits_triangle(X[:, i], X[:, (i + 1) % 3], Y[:, 0], Y[:, 1], Y[:, 2])
    return hit


def _orient(a, b, c):
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def _flat_test(A, B):
    """bool [n]: the 2D test of triangles A, B [n, 3, 2]: two edges cross, or a vertex of one lies in the other"""
    hit = np.zeros(A.shape[0], bool)
    for i in range(3):
        for j in range(3):
            p, q, r, s = A[:, i], A[:, (i + 1) % 3], B[:, j], B[:, (j + 1) % 3]
            hit |= (_orient(p, q, r) * _orient(p, q, s) <= 0) & (_orient(r, s, p) * _orient(r, s, q) <= 0) & \
                   ((_orient(p, q, r) != 0) | (_orient(p, q, s) != 0))
    for X, Y in ((A, B), (B, A)):
        o = [_orient(Y[:, j], Y[:, (j + 1) % 3], X[:, 0]) for j in range(3)]
        hit |= ((o[0] >= 0) & (o[1] >= 0) & (o[2] >= 0)) | ((o[0] <= 0) & (o[1] <= 0) & (o[2] <= 0))
    return hit


def _statement64(A, B):
    return tt.tri_tri_intersect(A[:, 0], A[:, 1], A[:, 2], B[:, 0], B[:, 1] - B[:, 0], B[:, 2] - B[:, 0])


def test_the_17_axes_against_independent_float64_tests():
    n = 100000
    rng = np.random.default_rng(2024)
    # random pairs in general position: they intersect iff an edge of one pierces the other
    A = rng.uniform(-1.0, 1.0, (n, 3, 3))
    B = rng.uniform(-1.0, 1.0, (n, 3, 3)) + rng.uniform(-1.0, 1.0, (n, 1, 3))
    got, want = _statement64(A, B), _pierce_test(A, B)
    print("random pairs: %d of %d intersect, %d differ" % (want.sum(), n, (got != want).sum()))
    assert 0.1 < want.mean() < 0.9 and np.array_equal(got, want)
    # coplanar pairs in the plane z = 0.25, y = 0.25 or x = 0.25 (exactly coplanar): the 2D test
    A2 = rng.uniform(-1.0, 1.0, (n, 3, 2))
    B2 = rng.uniform(-1.0, 1.0, (n, 3, 2)) + rng.uniform(-1.5, 1.5, (n, 1, 2))
    want = _flat_test(A2, B2)
    for plane in range(3):
        A3, B3 = np.full((n, 3, 3), 0.25), np.full((n, 3, 3), 0.25)
        keep = [k for k in range(3) if k != plane]
        A3[:, :, keep], B3[:, :, keep] = A2, B2
        got = _statement64(A3, B3)
        assert np.array_equal(got, want), (plane, (got != want).sum())
        # without the six in-plane axes every coplanar pair is kept
        g = tt.conditions(A3[:, 0], A3[:, 1], A3[:, 2], B3[:, 0], B3[:, 1] - B3[:, 0], B3[:, 2] - B3[:, 0])
        boxes_apart = (~g["boxes"]).mean()
        assert (g["normals"] & g["edges"]).all() and boxes_apart < (~want).mean()
    print("coplanar pairs: %d of %d intersect; the 11 axes alone keep all of them, the boxes reject %.3f" % (want.sum(), n, boxes_apart))
    assert 0.2 < want.mean() < 0.8


@pytest.fixture(scope="module")
def cornell():
    """scene file -> (verts, idx, {set: (records, fp32 intersection matrix)}): the brute force, computed once, shared, never written"""
    cam = ((278.0, 273.0, -900.0), (-616.7, 0.0, 0.0), (0.0, 387.8, 0.0), (0.0, 0.0, 1230.0))         # close to the default view at 97 x 61
    out = {}
    for scene in ("cornell_box.obj", "cornell_box_diffuse.obj"):
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
        verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
        sets = {}
        for name in tt.QUERY_SETS:
            r = tt.query_set(name, verts, idx, camera=cam)
            m = tt.intersect_matrix(r, verts, idx)
            r.setflags(write=False); m.setflags(write=False)
            sets[name] = (r, m)
        out[scene] = (verts, idx, sets)
    return out


def test_fp32_statement_against_float64(cornell):
    verts, idx, sets = cornell["cornell_box.obj"]
    lo, hi = nr.scene_box(verts, idx)
    S = float(max(np.abs(lo).max(), np.abs(hi).max()))
    v0, e1, e2 = (a.astype(np.float64) for a in nr.records_of_scene(verts, idx))
    worst, differ, kept = 0.0, 0, 0
    for name in FP64_SETS:
        r, m32 = sets[name]
        m64 = tt.intersect_matrix(r, verts, idx, np.float64)
        rows, cols = np.nonzero(m32 != m64)
        gap = 0.0
        if rows.size:
            a = tt.vertices_of(r)[rows].astype(np.float64)
            g = tt.normalised_gaps(a[:, 0], a[:, 1], a[:, 2], v0[cols], e1[cols], e2[cols])
            gap = float(np.abs(g.min(axis=0)).max())
        print("%s: %d pairs kept, %d differ from float64, largest |gap| %.3e of S" % (name, m32.sum(), rows.size, gap / S))
        worst, differ, kept = max(worst, gap / S), differ + rows.size, kept + int(m32.sum())
    print("all: %d of %d pairs differ, |gap| %.3e of S (held to %.3e)" % (differ, kept, worst, GAP_BOUND))
    assert kept > 10000 and 0 < differ < kept // 20        # there are contacts (the sets build them), and they are not the rule
    assert worst <= GAP_BOUND, worst
    # random triangles make no contacts
    assert np.array_equal(sets["random"][1], tt.intersect_matrix(sets["random"][0], verts, idx, np.float64))


@pytest.mark.parametrize("scene", ["cornell_box.obj", "cornell_box_diffuse.obj"])
def test_query_sets_shares_on_the_reference(cornell, scene):
    """The shares the GPU tests rely on, by the brute force alone"""
    verts, idx, sets = cornell[scene]
    n_tris = len(idx) // 3
    for name in tt.QUERY_SETS:
        assert sets[name][0].shape == (tt.SET_SIZE, 12) and tt.searchable(sets[name][0]).all(), name
    counts = sets["random"][1].sum(axis=1)
    above = {k: float((counts > k).mean()) for k in (1, 4, 8)}
    print("%s random: %.3f empty, above 1 / 4 / 8: %.3f / %.3f / %.3f, %d triangles named" % (scene, (counts == 0).mean(), above[1], above[4], above[8], sets["random"][1].any(axis=0).sum()))
    assert (counts == 0).mean() >= 0.10 and (counts != 0).mean() >= 0.25 and min(above.values()) >= 0.01, above
    r, m = sets["self"]
    pick = np.resize(np.random.default_rng(919).permutation(n_tris), tt.SET_SIZE)
    counts = m.sum(axis=1)
    print("%s self: %.3f above 8" % (scene, (counts > 8).mean()))
    assert m[np.arange(tt.SET_SIZE), pick].all() and (counts >= 1).all() and (counts > 8).mean() >= 0.5
    assert (sets["edge"][1].sum(axis=1) >= 1).all()                   # the shared edge is a contact the statement keeps exactly
    for name in ("coplanar", "wall_touch", "degenerate", "far"):       # both answers, so that neither can pass vacuously
        hit = sets[name][1].any(axis=1)
        print("%s %s: %.3f hit" % (scene, name, hit.mean()))
        assert hit.mean() >= 0.25 and (~hit).mean() >= 0.10, (name, hit.mean())
    counts = sets["whole"][1].sum(axis=1)
    print("%s whole: %.1f triangles per query, at most %d" % (scene, counts.mean(), counts.max()))
    assert (counts > 8).mean() >= 0.5 and counts.max() >= 100
    assert not sets["outside"][1].any()
    r = tt.vertices_of(sets["far"][0])
    lo, hi = nr.scene_box(verts, idx)
    diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    assert (np.abs(r - 0.5 * (lo + hi)).max(axis=(1, 2)) > 9.0 * diag).all()


def test_build_lists_and_abi():
    assert "tritri.hip" in _build.HIP_SOURCES and "tritri.h" in _build.HIP_HEADERS
    for name in ("tritri.hip", "tritri.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    assert "pt_query_triangles" in _native.ABI_SYMBOLS and "pt_query_triangles_any" in _native.ABI_SYMBOLS and "pt_debug_triangles_visits" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4 and _native.QUERY_TRIANGLES_MAX == tt.MAX_PRIMS == 8
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert "#define PT_QUERY_TRIANGLES_MAX 8" in hdr
    assert "int pt_query_triangles(pt_ctx* ctx, const float* tris, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts);" in hdr
    assert "int pt_query_triangles_any(pt_ctx* ctx, const float* tris, size_t n, uint8_t* hit);" in hdr


def test_triangle_kernels_use_no_scratch_memory_and_spill_nothing(built):
    """The twelve k_query_triangles instantiations (two node formats; lists of 0, 1, 4 and 8, any, the counting twin): no private
    segment, no spilled vector or scalar register, five waves per SIMD at the least"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_query_triangles<" in k["name"]]
    assert len(rows) == 12, [k["name"] for k in rows]
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] <= 96, k


def test_querytriangles_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for fn in (pt.queryTriangles, pt.queryTrianglesAny):
        for bad in (np.zeros((4, 8), np.float32), np.zeros(12, np.float32), np.zeros((2, 3, 4), np.float32), [[1, 2, 3]]):
            with pytest.raises(pt.PathTracerError, match="expected"):
                fn(state, bad)
        with pytest.raises(pt.PathTracerError, match="numbers"):
            fn(state, np.zeros((2, 9), np.complex64))
    for bad in (9, -1, 2.5, "x", None):
        with pytest.raises(pt.PathTracerError, match="max_prims"):
            pt.queryTriangles(state, np.zeros((4, 9), np.float32), max_prims=bad)
    with pytest.raises(pt.PathTracerError, match="counts=True"):
        pt.queryTriangles(state, np.zeros((4, 9), np.float32), max_prims=0, counts=False)
    # no triangles: nothing to do, in every form of the argument
    for empty in (np.zeros((0, 3, 3), np.float32), np.zeros((0, 9)), np.zeros((0, 12), np.float32)):
        got = pt.queryTriangles(state, empty, max_prims=3)
        assert sorted(got) == ["count", "prim"] and got["prim"].shape == (0, 3) and got["prim"].dtype == np.uint32 and got["count"].shape == (0,)
        assert sorted(pt.queryTriangles(state, empty, counts=False)) == ["prim"]
        assert pt.queryTrianglesAny(state, empty).shape == (0,) and pt.queryTrianglesAny(state, empty).dtype == np.bool_
    torch = pytest.importorskip("torch")
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.queryTriangles(state, torch.zeros((4, 12), dtype=torch.float32))


def test_triangle_records_and_mesh_collisions_without_a_device():
    verts = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], np.float64)
    idx = np.array([[0, 1, 2], [0, 1, 3]], np.int32)
    r = pt.triangleRecords(verts, idx)
    assert r.shape == (2, 12) and r.dtype == np.float32 and np.array_equal(r, tt.as_records(verts[idx]))
    assert np.array_equal(pt.triangleRecords(np.concatenate([verts, np.ones((4, 1))], axis=1), idx.reshape(-1)), r)      # (V, 4) vertices, flat indices
    # a pose: x -> R x + t, as 3 x 4 and as 4 x 4
    pose = np.array([[0, -1, 0, 10], [1, 0, 0, 20], [0, 0, 1, 30]], np.float64)
    moved = verts @ pose[:, :3].T + pose[:, 3]
    assert np.array_equal(pt.triangleRecords(verts, idx, pose), tt.as_records(moved[idx]))
    assert np.array_equal(pt.triangleRecords(verts, idx, np.concatenate([pose, [[0, 0, 0, 1]]])), tt.as_records(moved[idx]))
    for bad_v, bad_i, bad_p, what in ((verts[:, :2], idx, None, "vertices"), (verts, idx.astype(np.float32), None, "indices"), (verts, [0, 1], None, "indices"),
                                      (verts, [[0, 1, 4]], None, "outside"), (verts, idx, np.eye(3), "pose"), (verts, idx, np.zeros((2, 3, 4)), "pose")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.triangleRecords(bad_v, bad_i, bad_p)
    state = pt.PathTracerState()
    with pytest.raises(pt.PathTracerError, match="pose"):
        pt.meshCollisions(state, verts, idx, poses=np.zeros((2, 2, 4)))
    # a mesh without triangles touches nothing, in every pose, and the library is never asked
    assert pt.meshCollisions(state, verts, np.zeros((0, 3), np.int32), poses=np.stack([pose, pose])).tolist() == [False, False]
    got = pt.meshCollisions(state, verts, np.zeros((0, 3), np.int32), pairs=True)
    assert got["pairs"].shape == (0, 3) and got["counts"].shape == (1, 0)
