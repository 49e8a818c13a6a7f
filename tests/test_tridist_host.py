"""pt_query_triangle_distance without a GPU: the NumPy statement of the record (tests/tridist_ref.py) on hand-checked pairs and against
the float64 formulation (the minimum of six float64 segment-to-triangle calls), the tie and crossing rules, the queries that are a
miss before any traversal, the two box bounds of the walk against the float64 distance, the query sets' shares on the Cornell fixtures
and the icosphere by the brute force alone, the build lists, and the argument checks of queryTriangleDistance and meshClearance that
need no device."""
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import query_scenes as qs
import tridist_ref as tr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest |fp32 - float64| of the distance over _random_pairs() below (coordinates up to 12, edges up to 3.5), measured once on the
# CPU against the float64 six-call formulation (the figure DESIGN.md section 33 quotes), and the bound the test holds the fp32
# statement to: four times that (section 24's convention).
DIST_MEASURED = 1.02e-6
DIST_BOUND = 4.0 * DIST_MEASURED

TRI = (np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32), np.array([0, 1, 2], np.uint32))


def _one(a0, a1, a2, r=np.inf, verts=TRI[0], idx=TRI[1], mats=(0x05000007,)):
    rec = tr.triangle_distance_records(tr.as_records(np.array([list(a0) + list(a1) + list(a2)], np.float32), r), verts, idx, np.array(mats, np.uint32))
    return rec[0], rec.view(np.float32)[0]


def test_hand_checked_triangles_against_one_triangle():
    """A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0); every value below is exact in fp32"""
    cases = [
        # a0, a1, a2, distance, feature, point on the query, point on the scene triangle
        ((1, 1, 2), (2, 1, 5), (1, 2, 5), 2.0, 0, (1, 1, 2), (1, 1, 0)),                 # a vertex of the query over the face
        ((2, 1, 5), (1, 1, 2), (1, 2, 5), 2.0, 1, (1, 1, 2), (1, 1, 0)),                 # the same vertex second
        ((2, 1, 5), (1, 2, 5), (1, 1, 2), 2.0, 2, (1, 1, 2), (1, 1, 0)),                 # and third
        ((-8, -8, 3), (24, -8, 3), (-8, 24, 3), 3.0, 3, (0, 0, 3), (0, 0, 0)),           # a large face above: the scene's vertices are closest, v0 first
        ((5, -8, -8), (5, 24, -8), (5, -8, 24), 1.0, 4, (5, 0, 0), (4, 0, 0)),           # a wall beside B: w1
        ((-8, 6, -8), (24, 6, -8), (-8, 6, 24), 2.0, 5, (0, 6, 0), (0, 4, 0)),           # a wall behind C: w2
        ((1, -2, 3), (3, -2, -3), (2, -9, 0), 2.0, 6, (2, -2, 0), (2, 0, 0)),            # query edge 0 skew to scene edge 0
        ((2, -9, 0), (1, -2, 3), (3, -2, -3), 2.0, 12, (2, -2, 0), (2, 0, 0)),           # the same pair of edges as query edge 2
        ((1, 1, 2), (1, 1, -2), (9, 9, 2), 0.0, 15, (1, 1, 0), (1, 1, 0)),               # query edge 0 through the face
        ((9, 9, 2), (1, 1, 2), (1, 1, -2), 0.0, 17, (1, 1, 0), (1, 1, 0)),               # query edge 2 through the face
        ((1, -1, -1), (1, -1, 1), (1, 9, 0), 0.0, 18, (1, 0, 0), (1, 0, 0)),             # scene edge AB through the query's face, no query edge through the scene's
    ]
    for a0, a1, a2, dist, feature, q, c in cases:
        u32, f = _one(a0, a1, a2)
        assert f[0] == F(dist) and f[2] == F(feature), (a0, a1, a2, f[0], f[2])
        assert u32[1] == 0 and u32[3] == 7, (a0, a1, a2)                  # the material id without the flags above bit 24
        assert tuple(f[4:7]) == q and tuple(f[8:11]) == c, (a0, a1, a2, f[4:7], f[8:11])
        assert u32[7] == 0 and u32[11] == 0
    names = pt.TRIANGLE_DISTANCE_DTYPE.names
    assert pt.TRIANGLE_DISTANCE_DTYPE.itemsize == 48 and [pt.TRIANGLE_DISTANCE_DTYPE.fields[k][1] for k in names] == [0, 4, 8, 12, 16, 28, 32, 44]


def test_ties_crossings_and_the_radius_rule():
    # two coincident scene triangles: the lower index answers; a crossing overrides a vertex that lies ON the scene triangle (d2 = 0 too)
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32)
    idx = np.array([0, 1, 2, 0, 1, 2], np.uint32)
    u32, f = _one((1, 1, 0), (1, 1, 4), (3, 3, 4), verts=verts, idx=idx, mats=(1, 2))
    assert u32[1] == 0 and u32[3] == 1 and f[0] == 0 and f[2] == 15          # a0 on the face (feature 0, d2 = 0) and edge 0 starting there: the crossing's record
    # of several accepted crossings the lowest feature number: edges 0 and 1 both pass through the face
    u32, f = _one((1, 1, 2), (1, 1, -2), (2, 1, -2))
    assert f[0] == 0 and f[2] == 15 and tuple(f[4:7]) == (1, 1, 0)
    # the radius: d2 <= r * r in fp32, -0 is 0, a square that overflows is +inf
    for r, found in ((2.0, True), (np.nextafter(F(2.0), F(0.0)), False), (1e30, True), (np.inf, True)):
        u32, f = _one((1, 1, 2), (2, 1, 5), (1, 2, 5), r=r)
        assert (u32[1] == 0) == found, r
    u32, f = _one((1, 1, 0), (2, 1, 5), (1, 2, 5), r=-0.0)
    assert u32[1] == 0 and f[0] == 0
    assert np.array_equal(_one((1, 1, 2), (2, 1, 5), (1, 2, 5), r=1.0)[0], tr.miss_records(1)[0])
    assert tuple(tr.miss_records(1)[0]) == (F(-1.0).view(np.uint32), 0xFFFFFFFF, 0, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0, 0, 0)


def test_degenerate_queries_are_their_vertices_and_edges():
    """a2 == a1: a segment; three equal vertices: a point.  The face features of the query may give a NaN (no candidate); the vertex and
    edge features answer."""
    u32, f = _one((1, -2, 3), (3, -2, -3), (3, -2, -3))
    assert u32[1] == 0 and f[0] == F(2.0) and tuple(f[8:11]) == (2, 0, 0)
    u32, f = _one((1, 1, 2), (1, 1, 2), (1, 1, 2))
    assert u32[1] == 0 and f[0] == F(2.0) and f[2] == 0 and tuple(f[8:11]) == (1, 1, 0)
    u32, f = _one((1, 1, 2), (1, 1, -2), (1, 1, -2))                          # a segment through the face
    assert f[0] == 0 and f[2] == 15


def test_bad_triangles_are_misses_and_the_ignored_floats_are_ignored():
    good = tr.as_records(np.array([[1, 1, 2, 2, 1, 5, 1, 2, 5]], np.float32))[0]
    bad, why = tr.bad_triangles(good)
    assert bad.shape[0] < 32 and len(why) == bad.shape[0]
    assert tr.searchable(good[None]).all() and not tr.searchable(bad).any(), [w for w, s in zip(why, tr.searchable(bad)) if s]
    rec = tr.triangle_distance_records(bad, TRI[0], TRI[1], np.array([7], np.uint32))
    assert np.array_equal(rec, tr.miss_records(bad.shape[0]))
    want = tr.triangle_distance_records(good[None], TRI[0], TRI[1], np.array([7], np.uint32))
    for val in (np.nan, np.inf, -1.0):
        g = good.copy(); g[7] = val; g[11] = val
        assert tr.searchable(g[None]).all()
        assert np.array_equal(tr.triangle_distance_records(g[None], TRI[0], TRI[1], np.array([7], np.uint32)), want)
    empty = tr.triangle_distance_records(good[None], np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert np.array_equal(empty, tr.miss_records(1))


def _random_pairs(n=20000, seed=41):
    """Pairs of random triangles with vertices within 1 of their centres, the centres up to 10 from the origin and 0 to 3 apart: about a
    twelfth of the pairs intersect, the rest are up to a few units apart"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-10.0, 10.0, (n, 3))
    away = rng.normal(size=(n, 3))
    away /= np.sqrt((away * away).sum(axis=1, keepdims=True))
    other = centre + away * rng.uniform(0.0, 3.0, (n, 1))
    a = [(centre + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32) for _ in range(3)]
    v = [(other + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32) for _ in range(3)]
    return a[0], a[1], a[2], v[0], v[1] - v[0], v[2] - v[0]


def test_fp32_statement_against_the_float64_six_call_formulation():
    a0, a1, a2, v0, e1, e2 = _random_pairs()
    d2, feat, q, c = tr.triangle_triangle(a0, a1, a2, v0, e1, e2)
    assert d2.dtype == np.float32 and q.dtype == np.float32 and c.dtype == np.float32 and not np.isnan(d2).any()
    dist = np.sqrt(d2)
    dist64 = tr.distance_f64(a0, a1, a2, v0, e1, e2)
    # both agree on exactly which pairs have distance 0
    zero, zero64 = dist == 0, dist64 == 0
    print("pairs at distance 0: %.1f %% (fp32), mismatches %d" % (100 * zero.mean(), int((zero != zero64).sum())))
    assert np.array_equal(zero, zero64) and 0.05 <= zero.mean() <= 0.5
    assert np.array_equal(zero, feat >= 15)
    # every group of features wins somewhere
    shares = np.bincount(tr.group_of(feat), minlength=5) / feat.size
    print("group shares: " + " / ".join("%.1f %%" % (100 * x) for x in shares))
    assert shares.min() >= 0.01, shares
    worst = np.abs(dist - dist64).max()
    print("largest |fp32 - float64| distance deviation over %d pairs: %.3e (bound %.3e)" % (a0.shape[0], worst, DIST_BOUND))
    assert worst <= DIST_BOUND
    assert worst >= DIST_MEASURED / 4.0          # the figure quoted is this set's, not a stale one
    # the two witness points lie on their triangles' planes' sides consistently: they are as far apart as the distance says
    gap = np.linalg.norm(q.astype(np.float64) - c, axis=1)
    print("largest | |q - c| - distance |: %.3e" % np.abs(gap - dist).max())
    assert np.abs(gap - dist).max() <= DIST_BOUND
    # the same statement in float64 is the six-call minimum to rounding: the twenty-one sub-tests leave nothing out
    d2_64 = tr.triangle_triangle(*(x.astype(np.float64) for x in (a0, a1, a2, v0, e1, e2)))[0]
    assert np.abs(np.sqrt(d2_64) - dist64).max() <= 1e-12


def test_both_box_bounds_stay_below_the_distance_to_every_triangle_in_the_box():
    """Bounds (a) and (b) of the walk, in float64, on random query triangles and boxes: neither exceeds the float64 squared distance from
    the query to a triangle that lies in the box.  Bound (b) is the larger one somewhere: it prunes."""
    rng = np.random.default_rng(43)
    n = 4000
    a = [rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32) for _ in range(3)]
    a[2][:200] = a[1][:200]                                  # segments
    a[1][:100] = a[0][:100]                                  # points
    lo = rng.uniform(-6.0, 6.0, (n, 3))
    hi = lo + rng.uniform(0.0, 3.0, (n, 3)) * (rng.random((n, 3)) > 0.1)      # a tenth of the extents are 0
    lo, hi = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
    a64 = [x.astype(np.float64) for x in a]
    ba, bb = tr.bound_a(*a64, lo, hi), tr.bound_b(*a64, lo, hi)
    worst = 0.0
    for _ in range(4):
        v = [(lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32) for _ in range(3)]
        v = [np.clip(x, lo, hi).astype(np.float32) for x in v]
        d = tr.distance_f64(a[0], a[1], a[2], v[0], v[1] - v[0], v[2] - v[0]) + 1e-5        # the fp32 edge vectors move the triangle by an ulp
        worst = max(worst, float((np.sqrt(np.maximum(ba, bb)) - d).max()))
        assert (np.sqrt(ba) <= d).all() and (np.sqrt(bb) <= d).all()
    assert (bb > ba).mean() >= 0.02 and (ba > 0).mean() >= 0.2
    assert not bb[:100].any()                                # a point has no normal: (b) contributes 0


@pytest.mark.parametrize("scene", ["cornell_box.obj", "cornell_box_diffuse.obj"])
def test_query_sets_do_what_they_are_there_for(scene):
    """By the brute force alone: a set that lost its purpose must not pass vacuously."""
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
    verts, idx, mats = obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()
    for name in tr.QUERY_SETS:
        tris = tr.query_set(name, verts, idx)
        assert tris.shape == (tr.SET_SIZE, 9) and tris.dtype == np.float32
        rec_inf, d2 = tr.triangle_distance_records(tr.as_records(tris), verts, idx, mats, return_d2=True)
        rec = tr.records_within(rec_inf, d2, tr.set_radius(name, verts, idx))
        found = rec[:, 1] != 0xFFFFFFFF
        groups = np.bincount(tr.group_of(rec_inf.view(np.float32)[:, 2]), minlength=5) / tr.SET_SIZE
        print("%-9s found %.3f, distance 0 %.3f, groups %s" % (name, found.mean(), (rec_inf.view(np.float32)[:, 0] == 0).mean(), np.round(groups, 3)))
        assert (rec_inf[:, 1] != 0xFFFFFFFF).all()
        assert found.mean() >= 0.25 and (~found).mean() >= 0.10, (name, found.mean())
        assert np.unique(rec[found, 1]).size >= 8, name
        if name in ("large", "touching"):
            assert groups[3] >= 0.05 and groups[4] >= 0.05, (name, groups)
        # records_within is the brute force at that radius
        sub = slice(0, 64)
        again = tr.triangle_distance_records(tr.as_records(tris[sub], tr.set_radius(name, verts, idx)), verts, idx, mats)
        assert np.array_equal(again, rec[sub]), name


def test_tangent_triangles_find_scene_vertices_and_edge_pairs():
    v, idx, ids, _ = qs.sphere()
    tris = tr.tangent_triangles(v, idx, n=257)
    rec = tr.triangle_distance_records(tr.as_records(tris), v, idx.reshape(-1), ids, chunk=4)
    f = rec.view(np.float32)
    groups = np.bincount(tr.group_of(f[:, 2]), minlength=5) / tris.shape[0]
    print("tangent groups", np.round(groups, 3))
    assert groups[1] >= 0.20 and groups[2] >= 0.20 and (f[:, 0] > 0).all()


def test_build_lists_and_abi():
    assert "tridist.hip" in _build.HIP_SOURCES and {"tridist.h", "segment_device.h", "closest_point.h", "bvh_walk.h"} <= set(_build.HIP_HEADERS)
    for name in ("tridist.hip", "tridist.h", "segment_device.h", "closest_point.h", "bvh_walk.h", "segment.hip", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    assert "pt_query_triangle_distance" in _native.ABI_SYMBOLS and "pt_debug_triangle_distance_visits" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4


def test_querytriangledistance_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for bad in (np.zeros((4, 8), np.float32), np.zeros((4, 3, 4), np.float32), np.zeros(9, np.float32)):
        with pytest.raises(pt.PathTracerError, match="expected"):
            pt.queryTriangleDistance(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.queryTriangleDistance(state, np.zeros((2, 9), object))
    for r in (-1.0, float("nan")):
        with pytest.raises(pt.PathTracerError, match="max_radius"):
            pt.queryTriangleDistance(state, np.zeros((2, 9), np.float32), r)
        with pytest.raises(pt.PathTracerError, match="max_radius"):
            pt.meshClearance(state, np.zeros((3, 3), np.float32), [0, 1, 2], max_radius=r)
    with pytest.raises(pt.PathTracerError, match="indices"):
        pt.meshClearance(state, np.zeros((3, 3), np.float32), [0, 1])
    with pytest.raises(pt.PathTracerError, match="pose"):
        pt.meshClearance(state, np.zeros((3, 3), np.float32), [0, 1, 2], poses=np.zeros((2, 2, 2)))
    assert pt.queryTriangleDistance(state, np.zeros((0, 9), np.float32))["distance"].shape == (0,)
