"""pt_query_overlap without a GPU: the NumPy statement of the triangle-box test (tests/overlap_ref.py) on hand-checked boxes, the
miss table, the list rule, fp32 against the same algorithm in float64, the box sets' shares on the Cornell fixtures, and the argument
checks of queryOverlap and bakeOccupancy that need no device."""
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import nearest_ref as nr
import overlap_ref as ov

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fp32 against float64.  A pair (box, triangle) on which the two differ must be a contact: the float64 answer at h - delta is "apart"
# and at h + delta "overlap".  The smallest delta, relative to the scene's largest |coordinate| S, that brackets every differing pair of
# FP64_SETS on the Cornell box, measured once on the CPU (the figure DESIGN.md section 27 quotes), and the bound the test holds the
# fp32 statement to: four times that.
FP64_SETS = ("random", "grid", "centroids", "wall_faces")
DELTA_MEASURED = 3.42e-9
DELTA_BOUND = 4.0 * DELTA_MEASURED

# A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0)
TRI = (np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32), np.array([0, 1, 2], np.uint32))


def _one(c, h, verts=TRI[0], idx=TRI[1]):
    m = ov.overlap_matrix(ov.as_boxes([c], [h]), verts, idx)
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    groups = ov.conditions(np.array(c, np.float32), np.array(h, np.float32), v0[0], e1[0], e2[0])
    return bool(m[0, 0]), tuple(bool(g) for g in groups)


def test_hand_checked_boxes_of_one_triangle():
    """Every value below is exact in fp32.  (overlap, (faces, plane, edges)): which group of conditions separates"""
    cases = [
        ((1, 1, 0), (0.5, 0.5, 0.5), True, (True, True, True)),                 # inside the face
        ((1, 1, 0.5), (0.25, 0.25, 0.5), True, (True, True, True)),             # resting on the face from above: touching counts
        ((1, 1, 0.75), (0.25, 0.25, 0.5), False, (False, False, False)),        # a quarter above it (cross(x, AB) is the z axis too)
        ((2, 0, 0), (0.5, 0.5, 0.5), True, (True, True, True)),                 # through edge AB
        ((2, 2, 0), (0.25, 0.25, 0.25), True, (True, True, True)),              # through edge BC
        ((4.5, 0, 0), (0.5, 0.5, 0.5), True, (True, True, True)),               # touching vertex B with a face
        ((4.5, 0.5, 0.5), (0.5, 0.5, 0.5), True, (True, True, True)),           # touching vertex B with a corner
        ((4.5, 0.5, 0.5), (0.4375, 0.5, 0.5), False, (False, True, False)),     # and a sixteenth short of it
        ((3.5, 3.5, 0), (1, 1, 1), False, (True, True, False)),                 # beside BC inside the bounding box: only the edge axes separate
        ((3, 3, 0), (1, 1, 1), True, (True, True, True)),                       # its corner on BC
        ((1, 1, 0), (0, 0, 0), True, (True, True, True)),                       # a point box on the triangle
        ((1, 1, 0.25), (0, 0, 0), False, (False, False, False)),                # a point box off it
        ((2, 2, 0), (0, 0, 0), True, (True, True, True)),                       # a point box on edge BC
        ((1, 1, 0), (0, 0, 3), True, (True, True, True)),                       # a segment piercing it
        ((1, 1, 2), (0, 0, 2), True, (True, True, True)),                       # a segment ending on it
        ((3.5, 3.5, 0), (0, 0, 3), False, (True, True, False)),                 # a segment beside BC
        ((1, 1, 0), (1, 1, 0), True, (True, True, True)),                       # a rectangle in the triangle's plane
        ((-1, -1, 0), (1, 1, 0), True, (True, True, True)),                     # a rectangle touching A with a corner
    ]
    for c, h, want, groups in cases:
        got, g = _one(c, h)
        assert got == want and g == groups, (c, h, got, g)
    # the case only the plane axis rejects: a tilted triangle, a box inside its bounding box, beside no edge (seen along every axis the
    # box's shadow lies inside the triangle's) and off its plane
    verts = np.array([[0, 0, 0, 1], [8, 0, 8, 1], [0, 8, 8, 1]], np.float32)
    got, g = _one((2, 2, 1), (0.5, 0.5, 0.5), verts)
    assert got is False and g == (True, False, True)
    got, g = _one((2, 2, 3), (0.5, 0.5, 0.5), verts)
    assert got is True and g == (True, True, True)
    # a zero-area triangle is tested like any other: the collapsed edge A-B-A at y = z = 0
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [2, 0, 0, 1]], np.float32)
    assert _one((3, 0, 0), (0.5, 0.5, 0.5), verts)[0] is True and _one((3, 0, 0), (0, 0, 0), verts)[0] is True
    assert _one((3, 1, 0), (0.5, 0.5, 0.5), verts)[0] is False and _one((5, 0, 0), (0.5, 0.5, 0.5), verts)[0] is False


def test_the_miss_table():
    good = ov.as_boxes([[1, 1, 0]], [[0.5, 0.5, 0.5]])[0]
    bad, why = ov.bad_boxes(good)
    assert bad.shape[0] == 24 and not ov.searchable(bad).any(), [w for w, s in zip(why, ov.searchable(bad)) if s]
    counts, prims, hit = ov.overlap_records(bad, *TRI, max_prims=4)
    assert not counts.any() and (prims == 0xFFFFFFFF).all() and not hit.any()
    # boxes that look odd and are boxes: h = 0 and h = -0 (a point on the triangle, then the reserved floats set), an h whose
    # products overflow (r = +inf keeps, every s is finite), the largest finite h
    odd = np.array([[1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 0, -0.0, -0.0, -0.0, 0, 0], [1, 1, 0, -0.0, 0.5, 0, np.nan, -7],
                    [1, 1, 0, 1e30, 1e30, 1e30, 0, 0], [100, 100, 100, 3e38, 3e38, 3e38, 0, 0], [1, 1, 0.25, -0.0, 0, 0, 0, 0]], np.float32)
    assert ov.searchable(odd).all()
    counts, prims, hit = ov.overlap_records(odd, *TRI, max_prims=2)
    assert counts.tolist() == [1, 1, 1, 1, 1, 0] and hit.tolist() == [1, 1, 1, 1, 1, 0]
    assert prims.tolist() == [[0, 0xFFFFFFFF]] * 5 + [[0xFFFFFFFF] * 2]
    # a scene without triangles
    counts, prims, hit = ov.overlap_records(odd, np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), max_prims=3)
    assert counts.shape == (6,) and not counts.any() and prims.shape == (6, 3) and (prims == 0xFFFFFFFF).all() and not hit.any()
    # a NaN radius or three NaN projections fail their condition: a triangle with an infinite vertex overlaps nothing
    verts = np.array([[0, 0, 0, 1], [np.inf, 0, 0, 1], [0, 4, 0, 1]], np.float32)
    assert not ov.overlap_records(odd[:1], verts, TRI[1])[0].any()


def test_the_list_rule():
    """Twelve copies of the triangle, of which the box overlaps those with an even index: the count is not clamped, the list holds the
    lowest max_prims indices ascending and 0xFFFFFFFF behind them"""
    verts = np.concatenate([TRI[0] + np.array([0, 0, 10.0 * (k % 2), 0], np.float32) for k in range(12)])
    idx = np.arange(36, dtype=np.uint32)
    boxes = ov.as_boxes([[1, 1, 0], [1, 1, 10], [1, 1, 5], [1, 1, 5]], [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [1, 1, 5]])
    for k in range(0, ov.MAX_PRIMS + 1):
        counts, prims, hit = ov.overlap_records(boxes, verts, idx, max_prims=k)
        assert counts.tolist() == [6, 6, 0, 12] and hit.tolist() == [1, 1, 0, 1] and prims.shape == (4, k) and prims.dtype == np.uint32
        full = [[0, 2, 4, 6, 8, 10, 0xFFFFFFFF, 0xFFFFFFFF], [1, 3, 5, 7, 9, 11, 0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF] * 8, list(range(8))]
        assert prims.tolist() == [row[:k] for row in full]


@pytest.fixture(scope="module")
def cornell():
    """scene file -> (verts, idx, {set: (boxes, fp32 overlap matrix)}): the brute force, computed once, shared, never written"""
    cam = ((278.0, 273.0, -900.0), (-616.7, 0.0, 0.0), (0.0, 387.8, 0.0), (0.0, 0.0, 1230.0))         # close to the default view at 97 x 61
    out = {}
    for scene in ("cornell_box.obj", "cornell_box_diffuse.obj"):
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
        verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
        sets = {}
        for name in ov.BOX_SETS:
            b = ov.box_set(name, verts, idx, camera=cam, n=4096 if name == "grid" else ov.SET_SIZE)
            m = ov.overlap_matrix(b, verts, idx)
            b.setflags(write=False); m.setflags(write=False)
            sets[name] = (b, m)
        out[scene] = (verts, idx, sets)
    return out


def _bracket_delta(c, h, v0, e1, e2, keeps, top):
    """The smallest delta (to 2^-60 of top) at which the float64 test on h + delta (keeps) or h - delta (not keeps) agrees with `keeps`"""
    sign = 1.0 if keeps else -1.0
    lo, hi = 0.0, top
    if bool(ov.tri_box_overlap(c, h + sign * hi, v0, e1, e2)) != keeps:
        return np.inf
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if bool(ov.tri_box_overlap(c, h + sign * mid, v0, e1, e2)) == keeps:
            hi = mid
        else:
            lo = mid
    return hi


def test_fp32_statement_against_float64(cornell):
    verts, idx, sets = cornell["cornell_box.obj"]
    lo, hi = nr.scene_box(verts, idx)
    S = float(max(np.abs(lo).max(), np.abs(hi).max()))
    v0, e1, e2 = (a.astype(np.float64) for a in nr.records_of_scene(verts, idx))
    worst, differ, kept = 0.0, 0, 0
    for name in FP64_SETS:
        b, m32 = sets[name]
        m64 = ov.overlap_matrix(b, verts, idx, np.float64)
        rows, cols = np.nonzero(m32 != m64)
        d = [_bracket_delta(b[r, 0:3].astype(np.float64), b[r, 3:6].astype(np.float64), v0[t], e1[t], e2[t], bool(m32[r, t]), S) for r, t in zip(rows, cols)]
        print("%s: %d pairs kept, %d differ from float64, largest bracketing delta %.3e of S" % (name, m32.sum(), rows.size, max(d, default=0.0) / S))
        worst, differ, kept = max(worst, max(d, default=0.0) / S), differ + rows.size, kept + int(m32.sum())
    print("all: %d of %d pairs differ, delta %.3e of S (held to %.3e)" % (differ, kept, worst, DELTA_BOUND))
    assert kept > 20000 and 0 < differ < kept // 500         # there are contacts, and they are rare
    assert worst <= DELTA_BOUND, worst
    # the boxes far from the scene: the rounding of v0 - c is an ulp of |c|, so the same bound holds relative to |c| there
    b, m32 = sets["far"]
    m64 = ov.overlap_matrix(b, verts, idx, np.float64)
    rows, cols = np.nonzero(m32 != m64)
    far = [_bracket_delta(b[r, 0:3].astype(np.float64), b[r, 3:6].astype(np.float64), v0[t], e1[t], e2[t], bool(m32[r, t]), 1e3 * S) / float(np.abs(b[r, 0:3]).max())
           for r, t in zip(rows, cols)]
    print("far: %d pairs kept, %d differ, largest delta %.3e of |c|" % (m32.sum(), rows.size, max(far, default=0.0)))
    assert rows.size > 0 and max(far) <= 2.0 ** -23          # one ulp of |c|: p = v0 - c rounds once, by half an ulp of about |c|


@pytest.mark.parametrize("scene", ["cornell_box.obj", "cornell_box_diffuse.obj"])
def test_box_sets_shares_on_the_reference(cornell, scene):
    """The shares the GPU tests rely on, by the brute force alone"""
    verts, idx, sets = cornell[scene]
    n_tris = len(idx) // 3
    for name in ov.MIXED_SETS:
        b, m = sets[name]
        counts = m.sum(axis=1)
        above = {k: float((counts > k).mean()) for k in (1, 4, 8)}
        print("%s %s: %.3f empty, above 1 / 4 / 8: %.3f / %.3f / %.3f, %d triangles named" % (scene, name, (counts == 0).mean(), above[1], above[4], above[8], m.any(axis=0).sum()))
        assert np.isfinite(b).all() and ov.searchable(b).all()
        assert (counts == 0).mean() >= 0.10 and (counts != 0).mean() >= 0.25, name
        assert min(above.values()) >= 0.01, (name, above)
        assert m.any(axis=0).sum() >= 64, name
    b, m = sets["centroids"]
    assert m.sum(axis=1).min() >= 1 and (b[:, 3:6].min(axis=1) < 1e-5 * 960).any()       # every box names a triangle, down to tiny boxes
    b, m = sets["first_hits"]
    h = b[:, 3:6]
    assert ((h == 0).sum(axis=1) == 3).mean() >= 0.2 and ((h == 0).sum(axis=1) == 2).mean() >= 0.2 and ((h == 0).sum(axis=1) == 1).mean() >= 0.2
    assert m.any(axis=1).mean() >= 0.25                               # flat boxes on the surface still find it
    b, m = sets["wall_faces"]
    assert m.any(axis=1).mean() >= 0.25 and (~m.any(axis=1)).mean() >= 0.10
    b, m = sets["far"]
    lo, hi = nr.scene_box(verts, idx)
    diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    dist = np.abs(b[:, 0:3] - 0.5 * (lo + hi)).max(axis=1)
    assert (dist > 9.0 * diag).all() and m.any(axis=1).mean() >= 0.25 and (~m.any(axis=1)).mean() >= 0.10
    b, m = sets["whole"]
    assert (m.sum(axis=1) == n_tris).all()
    b, m = sets["outside"]
    assert not m.any()


def test_build_lists_and_abi():
    assert "overlap.hip" in _build.HIP_SOURCES and "overlap.h" in _build.HIP_HEADERS
    for name in ("overlap.hip", "overlap.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    assert "pt_query_overlap" in _native.ABI_SYMBOLS and "pt_query_overlap_any" in _native.ABI_SYMBOLS and "pt_debug_overlap_visits" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4 and _native.QUERY_OVERLAP_MAX == ov.MAX_PRIMS == 8
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert "#define PT_QUERY_OVERLAP_MAX 8" in hdr
    assert "int pt_query_overlap(pt_ctx* ctx, const float* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts);" in hdr
    assert "int pt_query_overlap_any(pt_ctx* ctx, const float* boxes, size_t n, uint8_t* hit);" in hdr


def test_queryoverlap_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    c3, h3 = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    for fn in (pt.queryOverlap, pt.queryOverlapAny):
        for bad in (np.zeros((4, 5), np.float32), np.zeros(4, np.float32), np.zeros((2, 8, 1), np.float32), [[1, 2]]):
            with pytest.raises(pt.PathTracerError, match="expected"):
                fn(state, bad, 1.0)
        with pytest.raises(pt.PathTracerError, match="numbers"):
            fn(state, np.zeros((2, 3), np.complex64), 1.0)
        with pytest.raises(pt.PathTracerError, match="numbers"):
            fn(state, c3, np.zeros(3, np.complex64))
        with pytest.raises(pt.PathTracerError, match="need half_extents"):
            fn(state, c3)
        with pytest.raises(pt.PathTracerError, match="carry their half extents"):
            fn(state, np.zeros((4, 8), np.float32), 1.0)
        with pytest.raises(pt.PathTracerError, match="broadcast"):
            fn(state, c3, np.ones((3, 3), np.float32))
        for bad in (-1.0, float("nan"), [1.0, -0.5, 1.0]):
            with pytest.raises(pt.PathTracerError, match="non-negative"):
                fn(state, c3, bad)
    for bad in (9, -1, 2.5, "x", None):
        with pytest.raises(pt.PathTracerError, match="max_prims"):
            pt.queryOverlap(state, c3, h3, max_prims=bad)
    with pytest.raises(pt.PathTracerError, match="counts=True"):
        pt.queryOverlap(state, c3, h3, max_prims=0, counts=False)
    # no boxes: nothing to do, in every form of the arguments
    for args in ((np.zeros((0, 3), np.float32), 1.0), (np.zeros((0, 3), np.float32), (1, 2, 3)), (np.zeros((0, 8), np.float32),)):
        got = pt.queryOverlap(state, *args, max_prims=3)
        assert sorted(got) == ["count", "prim"] and got["prim"].shape == (0, 3) and got["prim"].dtype == np.uint32 and got["count"].shape == (0,)
        assert sorted(pt.queryOverlap(state, *args, counts=False)) == ["prim"]
        assert pt.queryOverlapAny(state, *args).shape == (0,) and pt.queryOverlapAny(state, *args).dtype == np.bool_
    torch = pytest.importorskip("torch")
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.queryOverlap(state, torch.zeros((4, 8), dtype=torch.float32))
    with pytest.raises(pt.PathTracerError, match="half_extents must be None"):
        pt.queryOverlapAny(state, torch.zeros((4, 8), dtype=torch.float32), 1.0)


def test_occupancy_grid_order_and_bounds():
    b = pt.occupancyBoxes((2, 3, 4), (0.0, 10.0, 100.0), (4.0, 13.0, 102.0))
    assert b.shape == (24, 8) and b.dtype == np.float32
    assert np.array_equal(b[:, 0:3], pt.distanceFieldPoints((2, 3, 4), (0.0, 10.0, 100.0), (4.0, 13.0, 102.0)))
    assert np.array_equal(b[:, 3:6], np.broadcast_to(np.array([0.5, 0.5, 0.5], np.float32), (24, 3))) and not b[:, 6:8].any()
    assert np.array_equal(b[1, 0:3] - b[0, 0:3], [1, 0, 0]) and np.array_equal(b[4, 0:3] - b[0, 0:3], [0, 1, 0])                   # x fastest
    # half a cell that is no fp32 number is rounded up: the cells cover the grid
    b = pt.occupancyBoxes((3, 3, 3), (0, 0, 0), (1, 1, 1))
    assert (b[:, 3:6].astype(np.float64) >= 1.0 / 6.0).all() and (b[:, 3:6] == np.nextafter(F(1.0 / 6.0), F(0)) ).sum() == 0
    assert np.array_equal(ov.grid_boxes((3, 5, 7), (-1, 0, 2), (1, 3, 9)), pt.occupancyBoxes((3, 5, 7), (-1, 0, 2), (1, 3, 9)))
    state = pt.PathTracerState()
    for res in ((0, 4, 4), (4, 4), 7, (4, -1, 4), (2048, 2048, 2048)):
        with pytest.raises(pt.PathTracerError, match="bakeOccupancy: .*(resolution|grid)"):
            pt.bakeOccupancy(state, res, bounds=((0, 0, 0), (1, 1, 1)))
    for bounds in (((0, 0, 0), (1, 1, -1)), ((0, 0), (1, 1)), ((0, 0, 0), (1, 1, np.inf)), ((0, 0, np.nan), (1, 1, 1)), 5):
        with pytest.raises(pt.PathTracerError, match="bakeOccupancy: bounds"):
            pt.bakeOccupancy(state, (2, 2, 2), bounds=bounds)
