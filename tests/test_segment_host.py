"""pt_query_segments without a GPU: the NumPy statement of the record (tests/segment_ref.py) on hand-checked segments and against the
same statement in float64, the tie rules, the segments that are a miss before any traversal, the radius rule, the two box bounds of
the walk against the float64 distance on every node box of the Cornell trees, the segment sets' shares on the Cornell fixtures and the
icosphere, the kernels' registers, and the argument checks of querySegments and capsuleClearance that need no device."""
import os
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import nearest_ref as nr
import segment_ref as sr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest |fp32 - float64| of the distance over _random_pairs() below, measured once on the CPU (the figure DESIGN.md section 30
# quotes), and the bound the test holds the fp32 statement to: four times that (section 24's convention).
DIST_MEASURED = 1.19e-6
DIST_BOUND = 4.0 * DIST_MEASURED

TRI = (np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32), np.array([0, 1, 2], np.uint32))


def _one(p0, p1, r=np.inf, verts=TRI[0], idx=TRI[1], mats=(0x05000007,)):
    rec = sr.segment_records(sr.with_radius(np.array([list(p0) + list(p1)], np.float32), r), verts, idx, np.array(mats, np.uint32))
    return rec[0], rec.view(np.float32)[0]


def test_hand_checked_segments_of_one_triangle():
    """A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0); every value below is exact in fp32"""
    r2 = float(np.sqrt(F(2.0)))
    cases = [
        # p0, p1, distance, s, feature, point on the triangle
        ((1, 1, 2), (1, 1, 5), 2.0, 0.0, 0, (1, 1, 0)),                # above the face, the first end nearest
        ((1, 1, 5), (1, 1, 2), 2.0, 1.0, 1, (1, 1, 0)),                # the second end nearest
        ((1, -2, 3), (3, -2, -3), 2.0, 0.5, 2, (2, 0, 0)),             # skew to edge AB: through the plane outside the triangle
        ((-2, 1, 3), (-2, 3, -3), 2.0, 0.5, 3, (0, 2, 0)),             # skew to edge AC
        ((3, 3, 2), (3, 3, -2), r2, 0.5, 4, (2, 2, 0)),                # skew to edge BC
        ((1, 1, 2), (1, 1, -2), 0.0, 0.5, 5, (1, 1, 0)),               # through the face
        ((1, 1, -6), (1, 1, 2), 0.0, 0.75, 5, (1, 1, 0)),              # through it from below: two-sided
        ((1, 1, 0), (1, 1, 4), 0.0, 0.0, 5, (1, 1, 0)),                # starting on the face: T = 0 is accepted
        ((5, 5, 0), (6, 7, 0), float(np.sqrt(F(18.0))), 0.0, 0, (2, 2, 0)),      # in the plane, outside: no crossing (det = 0); end 0 ties with edge BC
        ((1, -2, 0), (3, -2, 0), 2.0, 0.0, 0, (1, 0, 0)),              # parallel to AB: the whole stretch is at distance 2, end 0 ties with the edge
        ((1, 1, 2), (1, 1, 2), 2.0, 0.0, 0, (1, 1, 0)),                # a segment without length over the face
        ((6, -2, 0), (6, -2, 0), float(np.sqrt(F(8.0))), 0.0, 0, (4, 0, 0)),     # and one beyond B
    ]
    for p0, p1, dist, s, feature, c in cases:
        u32, f = _one(p0, p1)
        assert f[0] == F(dist), (p0, p1, f[0])
        assert u32[1] == 0 and u32[7] == 7, (p0, p1)                   # the material id without the flags above bit 24
        assert f[2] == F(s) and f[3] == F(feature), (p0, p1, f[2], f[3])
        assert tuple(f[4:7]) == c, (p0, p1, f[4:7])
    assert pt.SEGMENT_HIT_DTYPE.itemsize == 32 and [pt.SEGMENT_HIT_DTYPE.fields[k][1] for k in pt.SEGMENT_HIT_DTYPE.names] == [0, 4, 8, 12, 16, 28]
    # the parallel case inside the edge test itself: no 0 / 0, s = 0, the point of the edge under p0
    p0, d = np.array([1, -2, 0], F), np.array([2, 0, 0], F)
    d2, s, c = sr.segment_edge(p0, d, F(4.0), np.array([0, 0, 0], F), np.array([4, 0, 0], F))
    assert d2 == F(4.0) and s == F(0.0) and tuple(c) == (1, 0, 0)
    # an edge and a segment without length, alone and together
    d2, s, c = sr.segment_edge(p0, d, F(4.0), np.array([0, 0, 0], F), np.array([0, 0, 0], F))
    assert d2 == F(5.0) and s == F(0.0) and tuple(c) == (0, 0, 0)          # (1, -2, 0) is the segment's nearest point to the origin: s = clamp(-2 / 4)
    d2, s, c = sr.segment_edge(p0, np.zeros(3, F), F(0.0), np.array([0, 0, 0], F), np.array([0, 0, 0], F))
    assert d2 == F(5.0) and s == F(0.0)
    d2, s, c = sr.segment_edge(p0, np.zeros(3, F), F(0.0), np.array([0, 0, 0], F), np.array([4, 0, 0], F))
    assert d2 == F(4.0) and s == F(0.0) and tuple(c) == (1, 0, 0)


def test_a_zero_area_triangle_is_its_edges():
    """v2 on the edge v0 v1: features 0 and 1 may give a NaN (0 / 0 in the region of the collapsed side, no candidate), the edges
    answer"""
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [2, 0, 0, 1]], np.float32)
    u32, f = _one((1, 3, 1), (1, 3, -1), verts=verts)
    assert f[0] == F(3.0) and f[2] == F(0.5) and f[3] == F(2.0) and tuple(f[4:7]) == (1, 0, 0)
    u32, f = _one((1, 3, 1), (1, 3, 1), verts=verts)                          # and a point against it
    assert u32[1] == 0 and f[0] == F(np.sqrt(F(10.0))) and tuple(f[4:7]) == (1, 0, 0)
    # all three vertices in one place: every sub-test that is not a NaN says the same
    verts = np.array([[2, 0, 0, 1], [2, 0, 0, 1], [2, 0, 0, 1]], np.float32)
    u32, f = _one((2, 3, -1), (2, 3, 1), verts=verts)
    assert u32[1] == 0 and f[0] == F(3.0) and f[2] == F(0.5) and tuple(f[4:7]) == (2, 0, 0)


def _random_pairs(n=8704, seed=31):
    """Random triangles of edge ~1 around points up to 10 from the origin (area at least 0.1), each with a segment of length 0.2 .. 6 whose
    middle lies 0.3 .. 8 from the triangle's neighbourhood; a third of the segments are aimed at a point of the triangle or just
    beside it and reach it, pass it or stop short: every feature gets its share"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-10.0, 10.0, (n, 3))
    v = [(centre + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32) for _ in range(3)]
    unit = lambda a: a / np.sqrt((a * a).sum(axis=1, keepdims=True))           # noqa: E731
    away = unit(rng.normal(size=(n, 3)))
    direction = unit(rng.normal(size=(n, 3)))
    length = rng.uniform(0.2, 6.0, (n, 1))
    mid = centre + away * rng.uniform(0.3, 8.0, (n, 1))
    aim = rng.random((n, 1)) < 1.0 / 3.0
    b = rng.random((n, 2)); fold = b.sum(axis=1) > 1.0; b[fold] = 1.0 - b[fold]
    target = v[0] + b[:, 0:1] * (v[1].astype(np.float64) - v[0]) + b[:, 1:2] * (v[2].astype(np.float64) - v[0]) + rng.uniform(-0.5, 0.5, (n, 3))
    direction = np.where(aim, unit(target - mid), direction)
    reach = np.linalg.norm(target - mid, axis=1, keepdims=True)
    start = np.where(aim, mid + direction * (reach - length * rng.uniform(0.0, 1.2, (n, 1))), mid - 0.5 * length * direction)
    p0, p1 = start.astype(np.float32), (start + direction * length).astype(np.float32)
    nrm = np.cross(v[1].astype(np.float64) - v[0], v[2].astype(np.float64) - v[0])
    keep = np.linalg.norm(nrm, axis=1) >= 0.2
    return p0[keep], p1[keep], v[0][keep], v[1][keep], v[2][keep]


def test_fp32_distance_against_float64():
    p0, p1, v0, v1, v2 = _random_pairs()
    assert p0.shape[0] >= 8000
    d2, s, feat, c = sr.segment_triangle(p0, p1, v0, v1 - v0, v2 - v0)
    assert d2.dtype == np.float32 and c.dtype == np.float32 and s.dtype == np.float32 and not np.isnan(d2).any()
    dist = np.sqrt(d2)
    dist64, s64, feat64, c64 = sr.segment_f64(p0, p1, v0, v1, v2)
    # by the float64 side alone every feature wins its share
    shares = [float((feat64 == k).mean()) for k in range(6)]
    print("feature shares (float64): " + " / ".join("%.1f %%" % (100 * x) for x in shares))
    assert min(shares) >= 0.05, shares
    assert ((s64 >= 0) & (s64 <= 1)).all()
    # float64 is the same algorithm; an independent check of it: its distance is not above that of 60 points sampled along the segment
    best = np.full(p0.shape[0], np.inf)
    a64, b64 = p0.astype(np.float64), p1.astype(np.float64)
    for t in np.linspace(0.0, 1.0, 60):
        best = np.minimum(best, nr.closest_f64(a64 + (b64 - a64) * t, v0, v1, v2)[0])
    print("float64 statement above the sampled minimum by at most %.3e" % (dist64 - best).max())
    assert (dist64 - best).max() <= 1e-6
    assert ((best - dist64) < 0.2).all()               # and not far below it either: the samples are 0.1 apart at the most
    # the witness points are that far apart
    p64 = a64 + (b64 - a64) * s64[:, None]
    assert np.abs(np.linalg.norm(p64 - c64, axis=1) - dist64).max() <= 1e-9
    worst = np.abs(dist - dist64).max()
    print("largest |fp32 - float64| distance deviation over %d pairs: %.3e (bound %.3e)" % (p0.shape[0], worst, DIST_BOUND))
    assert worst <= DIST_BOUND
    assert worst >= DIST_MEASURED / 4.0          # the figure quoted is this set's, not a stale one


def test_ties_go_to_the_lower_feature_and_the_lowest_triangle_index():
    # features: an end exactly as far as an edge's closest point (both d2 = 18 as bits); the end wins
    p0, p1 = np.array([5, 5, 0], F), np.array([6, 7, 0], F)
    v0, e1, e2 = nr.records_of_scene(*TRI)
    d0 = nr.closest_on_triangle(p0, v0[0], e1[0], e2[0])[0]
    d4 = sr.segment_edge(p0, p1 - p0, F(5.0), v0[0] + e1[0], e2[0] - e1[0])[0]
    assert d0.view(np.uint32) == d4.view(np.uint32) == F(18.0).view(np.uint32)
    assert _one(p0, p1)[1][3] == F(0.0)
    # edges 2 and 3 meet at A: a segment nearest to A with both ends farther, equally near to both edges; edge 2 (AB) wins over 3 (AC)
    u32, f = _one((-1, -1, 2), (-1, -1, -2))
    d2s = [sr.segment_edge(np.array([-1, -1, 2], F), np.array([0, 0, -4], F), F(16.0), v0[0], e)[0] for e in (e1[0], e2[0])]
    assert d2s[0].view(np.uint32) == d2s[1].view(np.uint32) == F(2.0).view(np.uint32)
    assert f[3] == F(2.0) and f[2] == F(0.5) and tuple(f[4:7]) == (0, 0, 0) and f[0] == F(np.sqrt(F(2.0)))
    # triangles: two sharing the edge (0,0,0)-(0,4,0), a segment over the edge and along it: d2 to both the same bits.  Whichever order
    # the index buffer lists them in, triangle 0 wins.  And two coplanar triangles crossed at their shared edge: both d2 = 0.
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1], [-4, 0, 0, 1]], np.float32)
    for idx in (np.array([0, 1, 2, 0, 2, 3], np.uint32), np.array([0, 2, 3, 0, 1, 2], np.uint32)):
        for seg, dist in (((0, 1, 3, 0, 3, 3), 3.0), ((0, 1, 3, 0, 1, -3), 0.0)):
            g = sr.with_radius(np.array([seg], np.float32), np.inf)
            w0, w1, w2 = nr.records_of_scene(verts, idx)
            d2 = sr.segment_triangle(g[:, None, 0:3], g[:, None, 4:7], w0[None], w1[None], w2[None])[0][0]
            assert d2[0].view(np.uint32) == d2[1].view(np.uint32) and d2[0] == F(dist * dist)
            rec = sr.segment_records(g, verts, idx, np.array([3, 4], np.uint32))
            assert rec[0, 1] == 0 and rec[0, 7] == 3 and rec.view(np.float32)[0, 0] == F(dist)


def test_segments_that_miss_before_any_traversal():
    good = np.array([1.0, 1.0, 2.0, 50.0, 1.0, 1.0, 5.0, 0.0], np.float32)
    bad, why = sr.bad_segments(good)
    assert bad.shape[0] == 18 + 1 + 4
    ok = sr.searchable(bad)
    assert not ok.any(), [w for w, k in zip(why, ok) if k]
    rec = sr.segment_records(bad, TRI[0], TRI[1], np.zeros(1, np.uint32))
    assert np.array_equal(rec, sr.miss_records(bad.shape[0]))
    allowed = np.array([good] * 6, np.float32)
    allowed[1, 3] = np.inf
    allowed[2, 3] = -0.0                 # a radius of zero, whatever its sign bit
    allowed[3, 7] = np.nan               # the eighth float is nobody's business
    allowed[4, 7] = np.inf
    allowed[5, 7] = -1.0
    assert sr.searchable(allowed).all()
    rec = sr.segment_records(allowed, TRI[0], TRI[1], np.zeros(1, np.uint32))
    assert rec[0, 1] == 0 and rec[1, 1] == 0 and rec[2, 1] == 0xFFFFFFFF
    assert np.array_equal(rec[3], rec[0]) and np.array_equal(rec[4], rec[0]) and np.array_equal(rec[5], rec[0])
    # a scene without triangles: all misses
    rec = sr.segment_records(allowed, TRI[0], np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert np.array_equal(rec, sr.miss_records(6))


def test_radius_rule():
    a, b = (1, 1, 2), (1, 1, 5)                      # distance 2, d2 = 4
    assert _one(a, b, 2.0)[0][1] == 0                # d2 <= r * r: the rim counts
    assert _one(a, b, np.nextafter(F(2.0), F(0.0)))[0][1] == 0xFFFFFFFF
    assert _one(a, b, np.inf)[1][0] == F(2.0)
    assert _one(a, b, 1e30)[1][0] == F(2.0)          # r * r overflows to +inf: everything is a candidate
    for touching in (((1, 1, 0), (1, 1, 4)), ((1, 1, 2), (1, 1, -2)), ((2, 0, 0), (2, -3, 0)), ((1, 1, 0), (3, 1, 0))):
        u32, f = _one(*touching, r=0.0)              # r = 0 on a segment that touches: an end on the face, through it, an end on an edge, in the face
        assert u32[1] == 0 and f[0] == F(0.0), touching
    assert _one((1, 1, 1e-3), (1, 1, 4), 0.0)[0][1] == 0xFFFFFFFF
    # the radius picks among candidates, it does not change the winner
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1], [0, 0, 9, 1], [4, 0, 9, 1], [0, 4, 9, 1]], np.float32)
    idx = np.arange(6, dtype=np.uint32)
    for r, prim in ((np.inf, 0), (8.0, 0), (2.0, 0), (1.5, 0xFFFFFFFF)):
        assert _one((1, 1, 2), (1, 1, 3), r, verts, idx, (0, 1))[0][1] == prim
    assert _one((1, 1, 5), (1, 1, 6), 3.5, verts, idx, (0, 1))[0][1] == 1
    # records_within is the brute force at that radius
    segs = sr.with_radius(np.array([[1, 1, 2, 1, 1, 3], [1, 1, 5, 1, 1, 6], [1, 1, 4, 1, 1, 5], [1, 1, -1, 1, 1, 10]], np.float32), np.inf)
    rec_inf, d2 = sr.segment_records(segs, verts, idx, np.array([0, 1], np.uint32), return_d2=True)
    for r in (0.0, 1.5, 2.0, 3.5, 1e30):
        segs[:, 3] = r
        assert np.array_equal(sr.records_within(rec_inf, d2, F(r)), sr.segment_records(segs, verts, idx, np.array([0, 1], np.uint32))), r


# ---- the Cornell fixtures ----------------------------------------------------------------------------------------------------------
SCENE_FILES = ("cornell_box.obj", "cornell_box_diffuse.obj")


@pytest.fixture(scope="module")
def cornell_sets():
    """scene -> name -> (segments, records at +inf, records at the set's finite radius): computed once, shared, never written"""
    out = {}
    for scene in SCENE_FILES:
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
        verts, idx, mats = obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()
        out[scene] = {}
        for name in sr.SEGMENT_SETS:
            segs = sr.segment_set(name, verts, idx)
            rec_inf, d2 = sr.segment_records(sr.with_radius(segs, np.inf), verts, idx, mats, return_d2=True)
            rec_r = sr.records_within(rec_inf, d2, sr.set_radius(name, verts, idx))
            for a in (segs, rec_inf, rec_r):
                a.setflags(write=False)
            out[scene][name] = (segs, rec_inf, rec_r)
    return out


@pytest.mark.parametrize("scene", SCENE_FILES)
def test_segment_sets_find_and_miss_on_the_reference(cornell_sets, scene):
    """The shares the GPU tests rely on, by the brute force alone: with each set's finite radius at least a quarter of its segments find
    something and at least a tenth find nothing, the winners are at least eight different triangles, and the segment crosses the
    winner on at least 5 % of long, axis and touching; without a radius every segment finds something."""
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    lo, hi = nr.scene_box(verts, idx)
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    for name in sr.SEGMENT_SETS:
        segs, rec_inf, rec_r = cornell_sets[scene][name]
        assert segs.shape == (sr.SET_SIZE, 6) and segs.dtype == np.float32 and np.isfinite(segs).all()
        assert sr.searchable(sr.with_radius(segs, np.inf)).all()
        assert (rec_inf[:, 1] != 0xFFFFFFFF).all(), name
        found = rec_r[:, 1] != 0xFFFFFFFF
        f = rec_inf.view(np.float32)
        crossing = float((f[:, 3] == 5).mean())
        print("%s %s: %.3f found within the finite radius, %d distinct winners, %.3f crossing, features %s"
              % (scene, name, found.mean(), np.unique(rec_r[found, 1]).size, crossing, [round(float((f[:, 3] == k).mean()), 3) for k in range(6)]))
        assert found.mean() >= 0.25 and (~found).mean() >= 0.10, (name, found.mean())
        assert np.unique(rec_r[found, 1]).size >= 8 and np.unique(rec_inf[:, 1]).size >= 8, name
        assert np.array_equal(rec_r[found], rec_inf[found]), name
        assert (f[:, 2] >= 0).all() and (f[:, 2] <= 1).all() and np.isin(f[:, 3], np.arange(6)).all()
        assert ((f[:, 3] == 5) == (f[:, 0] == 0)).all() or name == "touching"      # distance 0 without a crossing: an end on the surface
        if name in ("long", "axis", "touching"):
            assert crossing >= 0.05, (name, crossing)
        length = np.linalg.norm(segs[:, 3:6].astype(np.float64) - segs[:, 0:3], axis=1)
        if name == "short":
            assert np.abs(length / diag - 0.02).max() < 1e-4
        if name == "axis":
            assert ((segs[:, 0:3] != segs[:, 3:6]).sum(axis=1) <= 1).all() and (length <= 0.5 * (hi - lo).max() + 1e-3).all()
        if name == "shell":
            assert (f[:, 0] > 8.5 * diag).all()
        if name == "touching":
            assert (f[:, 0] == 0).mean() >= 0.5


def test_the_tangent_set_lets_the_edges_win():
    """On the Cornell walls an edge feature almost never wins: coplanar neighbours make an end win.  Segments tangent to a sphere
    around the icosphere do it: by the reference alone features 2 to 4 win at least a tenth."""
    import query_scenes as qs
    v, idx, ids, _ = qs.SCENES["sphere"].arrays()
    segs = sr.tangent_set(v, idx, n=257)
    rec = sr.segment_records(sr.with_radius(segs, np.inf), v, idx, ids, chunk=qs._chunk(len(idx)))
    f = rec.view(np.float32)
    shares = [float((f[:, 3] == k).mean()) for k in range(6)]
    print("tangent set on the icosphere, feature shares: %s" % [round(x, 3) for x in shares])
    assert (rec[:, 1] != 0xFFFFFFFF).all() and sum(shares[2:5]) >= 0.10, shares
    assert np.unique(rec[:, 1]).size >= 8


@pytest.fixture(scope="module")
def cornell_trees():
    """scene -> (child boxes lo, hi [m, 2, 3] float64, per child the triangle indices under it): a PLOC tree of tests/build_ref.py over
    the leaf boxes the build makes"""
    import build_ref as br
    out = {}
    for scene in SCENE_FILES:
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
        verts, idx = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4), np.asarray(obj.getIndexBuffer(), np.uint32).reshape(-1, 3)
        prims = br.morton_order(verts, idx)[1]
        leaf_lo, leaf_hi = br.leaf_boxes(verts, idx, prims)
        ch, lo, hi = br.split(br.ploc(leaf_lo, leaf_hi)[0])
        under = {}

        def collect(ref):
            if ref < 0:
                return [int(prims[~ref])]
            if ref not in under:
                under[ref] = (collect(int(ch[ref, 0])), collect(int(ch[ref, 1])))
            return under[ref][0] + under[ref][1]

        sys.setrecursionlimit(max(sys.getrecursionlimit(), 4000))
        assert sorted(collect(0)) == list(range(len(idx)))
        out[scene] = (lo.astype(np.float64), hi.astype(np.float64), under)
    return out


@pytest.mark.parametrize("scene", SCENE_FILES)
def test_both_box_bounds_stay_below_the_distance_to_every_triangle_under_the_box(cornell_trees, scene):
    """Bounds (a) and (b) of the walk, in float64, for every child box of every inner node and 200 segments (40 of each set): neither
    exceeds the float64 distance from the segment to any triangle under the box.  Bound (b) is the larger one somewhere: it prunes."""
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    lo, hi, under = cornell_trees[scene]
    segs = np.concatenate([sr.segment_set(name, verts, idx)[:40] for name in sr.SEGMENT_SETS]).astype(np.float64)
    p0, p1 = segs[:, None, 0:3], segs[:, None, 3:6]
    v = np.asarray(verts, np.float64).reshape(-1, 4)[:, :3][np.asarray(idx, np.int64).reshape(-1, 3)]
    dist = sr.segment_f64(p0, p1, v[None, :, 0], v[None, :, 1], v[None, :, 2])[0]                  # [200, n_tris]
    assert not np.isnan(dist).any()
    b_wins = 0
    for node, tris in under.items():
        for k in (0, 1):
            if not tris[k]:
                continue
            below = dist[:, tris[k]].min(axis=1)
            a = np.sqrt(sr.bound_a(segs[:, 0:3], segs[:, 3:6], lo[node, k], hi[node, k]))
            b = np.sqrt(sr.bound_b(segs[:, 0:3], segs[:, 3:6], lo[node, k], hi[node, k]))
            slack = 1e-9 * (1.0 + below)
            assert (a <= below + slack).all() and (b <= below + slack).all(), (node, k, float((a - below).max()), float((b - below).max()))
            b_wins += int((b > a).sum())
    assert b_wins > 0


# ---- the layers ---------------------------------------------------------------------------------------------------------------------
def test_build_lists_and_abi():
    assert "segment.hip" in _build.HIP_SOURCES and "segment.h" in _build.HIP_HEADERS
    for name in ("segment.hip", "segment.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert "pt_query_segments" in _native.ABI_SYMBOLS and "pt_debug_segments_visits" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert "int pt_query_segments(pt_ctx* ctx, const float* segments, size_t n, pt_segment_hit* out);" in hdr
    assert "static_assert(sizeof(pt_segment_hit) == 32" in open(os.path.join(ROOT, "acgpathtracing_amd", "csrc", "capi_query.hip")).read()


def test_segment_kernels_use_no_scratch_memory_and_spill_nothing(built):
    """The four k_query_segments instantiations (two node formats, each with its counting twin): no private segment, no spilled vector
    or scalar register"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_query_segments<" in k["name"]]
    assert len(rows) == 4, [k["name"] for k in rows]
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


def test_querysegments_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 7), np.float32), np.zeros(8, np.float32), np.zeros((2, 8, 1), np.float32), [[1, 2, 3]]):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.querySegments(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.querySegments(state, np.zeros((2, 6), np.complex64))
    for bad in (-1.0, float("nan")):
        with pytest.raises(pt.PathTracerError, match="max_radius"):
            pt.querySegments(state, np.zeros((2, 6), np.float32), bad)
    empty = pt.querySegments(state, np.zeros((0, 6), np.float32))
    assert sorted(empty) == ["distance", "feature", "material", "point", "prim", "s"]
    assert empty["distance"].shape == (0,) and empty["point"].shape == (0, 3) and empty["prim"].dtype == np.uint32
    assert pt.querySegments(state, np.zeros((0, 8), np.float32), 2.0)["s"].shape == (0,)
    torch = pytest.importorskip("torch")
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.querySegments(state, torch.zeros((4, 8), dtype=torch.float32))


def test_capsuleclearance_argument_checks_need_no_device():
    state = pt.PathTracerState()
    ok = np.zeros((2, 3), np.float32)
    for a, b in ((np.zeros((2, 4)), np.zeros((2, 4))), (ok, np.zeros((3, 3))), (np.zeros(3), np.zeros(3)), (ok, np.zeros((2, 3, 1)))):
        with pytest.raises(pt.PathTracerError, match="two \\(n, 3\\) arrays"):
            pt.capsuleClearance(state, a, b, 1.0)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.capsuleClearance(state, ok.astype(np.complex64), ok, 1.0)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, -2.0], [1.0, 2.0, 3.0], "wide"):
        with pytest.raises(pt.PathTracerError, match="radius"):
            pt.capsuleClearance(state, ok, ok, bad)
    empty = pt.capsuleClearance(state, np.zeros((0, 3)), np.zeros((0, 3)), 0.5)
    assert sorted(empty) == ["clearance", "feature", "on_axis", "on_mesh", "prim", "s"]
    assert empty["clearance"].shape == (0,) and empty["on_axis"].shape == (0, 3) and empty["clearance"].dtype == np.float32
