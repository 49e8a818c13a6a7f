"""pt_query_box_cast without a GPU: the NumPy statement of the time of impact (tests/boxcast_ref.py) on hand-checked casts, its float64
evaluation against a bisection that knows nothing of the 13 axes, fp32 against float64 on the Cornell box, what the reference alone
must show (every feature wins its share, t = 0 is oriented_ref's overlap, what the 12-triangle route gets wrong, the tie rule, the
closed tmax, the casts that miss before any traversal), the interface (build lists, prototypes, symbols, kernel resources) and the
argument checks of queryBoxCast that need no device."""
import os
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import boxcast_ref as br
import nearest_ref as nr
import oriented_ref as ot
from test_capsule_host import SPHERE_CONTACT_MEASURED

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = os.path.join(pt.SCENES, "cornell_box.obj")

# fp32 against float64 (scene units, the box is 556 wide; DESIGN.md section 40 quotes both figures).  The yardstick is the sphere
# sweep's figure of section 28, SPHERE_CONTACT_MEASURED = 8.93e-5: what one subtraction o - P and one projection at coordinates of
# ~550 leave of a contact.  The box statement subtracts v0 - c and then takes every local coordinate through a three-term dot product
# (three more roundings at the same magnitude, for the triangle and again for the direction, whose error is multiplied by t); the
# reported point is measured against the box at c + d t32, itself two roundings.  Four times the roundings of the sphere's form at the
# same magnitude: FRAME_MARGIN = 4, fixed before the statement was evaluated.  Measured: 1.58e-4 (grazing), against the bar 3.57e-4.
FRAME_MARGIN = 4.0
BOX_CONTACT_MEASURED = 1.58e-4
# the float64 statement against the bisection: at most this many times the bisection's own resolution (below), as section 39 sets it
BISECTION_MULTIPLE = 4.0

TRI = (np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32), np.array([0, 1, 2], np.uint32))
INF = np.inf
EYE = np.eye(3)
R45Z = np.array([[np.sqrt(0.5), -np.sqrt(0.5), 0], [np.sqrt(0.5), np.sqrt(0.5), 0], [0, 0, 1]])
R3 = np.array([[2, -1, 2], [2, 2, -1], [-1, 2, 2]]) / 3.0          # a rotation with rational entries: its corner (+, -, -) points down


def _cast(c, h, rot, d, tmax=INF):
    return br.pack(ot.as_oboxes([c], [h], rot), [d], tmax)


def _one(cast, verts=TRI[0], idx=TRI[1], mats=(0x05000007,)):
    rec = br.box_records(cast, verts, idx, np.array(mats, np.uint32))
    return rec[0], rec.view(np.float32)[0]


def test_hand_checked_casts_of_one_triangle():
    """A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0).  One cast per class of features; every t below follows from the picture."""
    r2 = np.sqrt(2.0)
    cases = [
        # centre, half extent, rotation, d -> t, feature, normal, point, tolerance
        ((1, 1, 0.5), (1, 1, 1), EYE, (0, 0, -1), 0.0, 13, (0, 0, 0), (0, 0, 0), 0.0),                 # starts in contact
        ((1, 1, 5), (1, 1, 1), EYE, (0, 0, -1), 4.0, 2, (0, 0, 1), (0, 0, 0), 0.0),                    # face on face: the box face z and the plane tie, the lower axis wins; one representative point
        ((8, -0.5, 0.25), (1, 1, 1), EYE, (-1, 0, 0), 3.0, 0, (1, 0, 0), (4, 0, 0), 0.0),              # the triangle's corner B onto the box face x
        ((-0.5, 8, 0.25), (1, 1, 1), EYE, (0, -2, 0), 1.5, 1, (0, 1, 0), (0, 4, 0), 0.0),              # C onto the box face y, d of length 2
        ((0.5, 0.5, 9), (3, 3, 3), R3, (0, 0, -2), 2.0, 3, (0, 0, 1), (1.5, 1.5, 0), 4e-6),            # a box corner onto the face
        ((2, -5, 0), (1, 1, 1), R45Z, (0, 1, 0), 5.0 - r2, 6, (0, -1, 0), (2, 0, 0), 4e-6),            # the upright box edge onto edge AB
        ((1, 1, 5), (1, 1, 0), EYE, (0, 0, -1), 5.0, 2, (0, 0, 1), (0, 0, 0), 0.0),                    # a half extent of 0: a swept rectangle
        ((1, 1, 5), (0, 0, 0), EYE, (0, 0, -1), 5.0, 2, (0, 0, 1), (0, 0, 0), 0.0),                    # a swept point
    ]
    for c, h, rot, d, t, feature, normal, point, tol in cases:
        u32, f = _one(_cast(c, h, rot, d))
        assert abs(f[0] - F(t)) <= tol * max(t, 1.0) and f[2] == F(feature), (c, d, f[0], f[2])
        assert u32[1] == 0 and u32[3] == 7, c                     # the material id without the flags above bit 24
        assert np.abs(f[4:7] - np.array(normal, np.float32)).max() <= tol and np.abs(f[8:11] - np.array(point, np.float32)).max() <= tol * 8, (c, f[4:11])
        assert u32[7] == 0 and u32[11] == 0
    # tmax is closed: on the contact it hits, one ulp below it misses
    assert _one(_cast((1, 1, 5), (1, 1, 1), EYE, (0, 0, -1), 4.0))[1][0] == 4.0
    assert np.array_equal(_one(_cast((1, 1, 5), (1, 1, 1), EYE, (0, 0, -1), np.nextafter(F(4.0), F(0.0))))[0], br.miss_records(1)[0])
    misses = [((1, 1, 5), (0, 0, -1), 3.5), ((1, 1, 5), (0, 0, 1), INF), ((9, 9, 5), (0, 0, -1), INF), ((1, 1, 5), (0, 0, 0), INF), ((-3, -3, 0), (1, -1, 0), INF)]
    for c, d, tmax in misses:
        assert np.array_equal(_one(_cast(c, (1, 1, 1), EYE, d, tmax))[0], br.miss_records(1)[0]), (c, d)
    assert _one(_cast((1, 1, 0.5), (1, 1, 1), EYE, (0, 0, 0), 0.0))[1][0] == 0.0     # d = 0 and tmax = 0: the start overlap answers
    # a triangle wholly inside the solid box starts in contact: no triangle of the box's surface touches it
    u32, f = _one(_cast((1, 1, 0), (9, 9, 9), R3, (1, 0, 0)))
    assert f[0] == 0.0 and f[2] == 13.0
    assert br.twelve_triangle_route(_cast((1, 1, 0), (9, 9, 9), R3, (1, 0, 0)), TRI[0], TRI[1], np.zeros(1, np.uint32))[0] != 0.0
    assert pt.BOX_CAST_DTYPE.itemsize == 48 and pt.BOX_CAST_DTYPE.names == ("t", "prim", "feature", "material", "normal", "point")
    assert [pt.BOX_CAST_DTYPE.fields[k][1] for k in pt.BOX_CAST_DTYPE.names] == [0, 4, 8, 12, 16, 32]
    assert pt.BOX_CAST_DTYPE is _native.BOX_CAST_DTYPE
    assert np.array_equal(br.miss_records(1)[0], np.array([0xBF800000, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0, 0, 0], np.uint32))


@pytest.fixture(scope="module")
def cornell():
    obj = pt.TinyObjWrapper(BOX)
    return obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()


@pytest.fixture(scope="module")
def cornell_sets(cornell):
    """name -> (casts, records) by the fp32 brute force: computed once per set, shared, never written"""
    verts, idx, mats = cornell
    cache = {}

    def get(name):
        if name not in cache:
            c = br.cast_set(name, verts, idx, None, mats)
            rec = br.box_records(c, verts, idx, mats)
            c.setflags(write=False); rec.setflags(write=False)
            cache[name] = (c, rec)
        return cache[name]
    return get


def test_float64_statement_against_an_independent_bisection(cornell, cornell_sets):
    """The 13-axis clip is the geometric truth.  Box and triangle are convex, so oriented_ref.tri_obox_overlap(c + t d) holds on one
    interval of t; its lower end by bisection knows nothing of entry and exit times.  The bisection's own resolution, per cast: its
    last bracket, and what float64 leaves of the static test at coordinates of ~550 (an overlap decided at 1e-13 of the coordinates
    moves the time by that over the speed of approach along the winning axis, bounded below by 1e-15 of max(t, 1) per unit); on a
    graze the closing speed is small and it is the bisection that cannot tell, not the statement: the resolution is widened until
    the static test one step before it is clear by more than RES_DIST.  The bar is BISECTION_MULTIPLE times that.  Hit / no hit
    agree on every pair."""
    RES_DIST = 1e-10
    verts, idx, mats = cornell
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    worst, worst_rel, total = 0.0, 0.0, 0
    for name in br.COVERAGE_SETS:
        c, rec = cornell_sets(name)
        hit = rec[:, 1] != 0xFFFFFFFF
        c, w = c[hit], rec[hit, 1].astype(np.int64)
        t64, feat = br.impact_f64(c, v0[w], e1[w], e2[w])
        tb, width = br.bisect_impact_f64(c, v0[w], e1[w], e2[w])
        h64, hb = np.isfinite(t64), np.isfinite(tb)
        assert np.array_equal(h64, hb), (name, np.flatnonzero(h64 != hb)[:8])
        assert np.array_equal(t64[h64] == 0, tb[h64] == 0), name
        both = h64 & (tb > 0)
        assert both.mean() >= 0.2, (name, both.mean())
        cb, wb, tbb = c[both], w[both], tb[both]
        A, cc, hh, dd, _ = br.parts(cb, np.float64)
        res = np.maximum(width[both], 1e-15 * np.maximum(tbb, 1.0))
        for _ in range(60):
            before = np.maximum(tbb - res, 0.0)
            gap = br.box_triangle_distance_f64(A, cc + dd * before[:, None], hh, v0[wb].astype(np.float64), (v0[wb] + e1[wb]).astype(np.float64), (v0[wb] + e2[wb]).astype(np.float64))
            clear = (gap > RES_DIST) | (before == 0.0)
            res = np.where(clear, res, 2.0 * res)
        err = np.abs(t64[both] - tbb)
        assert (err <= BISECTION_MULTIPLE * res).all(), (name, float((err / res).max()))
        rel = err / np.maximum(tbb, 1.0)
        worst, worst_rel, total = max(worst, float((err / res).max())), max(worst_rel, float(rel.max())), total + int(both.sum())
        print("%s: %d moving hits, largest |t - bisection| %.3e of max(t, 1), %.3f of the bisection's resolution" % (name, both.sum(), rel.max(), (err / res).max()))
    print("all four sets: %d hits, largest relative difference %.3e, largest multiple of the resolution %.3f (bar %.1f)" % (total, worst_rel, worst, BISECTION_MULTIPLE))


def test_fp32_statement_against_float64_on_the_cornell_sets(cornell, cornell_sets):
    """Where fp32 says the box stops, float64 finds the reported point on the box's surface at c + d t32, within the sphere sweep's own
    figure times FRAME_MARGIN; the normal is a unit vector against the motion."""
    bar = SPHERE_CONTACT_MEASURED * FRAME_MARGIN
    worst = 0.0
    for name in br.COVERAGE_SETS:
        c, rec = cornell_sets(name)
        col = br.columns(rec)
        moving = col["t"] > 0
        assert moving.sum() >= 200, name
        err = br.obb_distance_f64(c[moving], col["t"][moving], col["point"][moving])
        print("%s: %d moving hits, largest distance of the point from the box %.3e by feature %d (bar %.3e)" % (name, moving.sum(), err.max(), col["feature"][moving][np.argmax(err)], bar))
        worst = max(worst, float(err.max()))
        assert err.max() <= bar, name
        n64 = col["normal"][moving].astype(np.float64)
        assert np.abs(np.sqrt((n64 * n64).sum(axis=1)) - 1.0).max() <= 1e-6, name
        assert ((n64 * c[moving, 16:19]).sum(axis=1) <= 0).all(), name
    print("largest over the four sets %.3e (quoted %.3e)" % (worst, BOX_CONTACT_MEASURED))
    assert BOX_CONTACT_MEASURED / 1.05 <= worst <= BOX_CONTACT_MEASURED * 1.05


def test_every_feature_wins_its_share(cornell_sets):
    counts = np.zeros(br.N_FEATURES)
    for name in br.COVERAGE_SETS:
        c, rec = cornell_sets(name)
        col = br.columns(rec)
        counts += np.bincount(col["feature"][col["t"] >= 0].astype(np.int64), minlength=br.N_FEATURES)
        assert np.unique(rec[:, 1]).size >= 32, name
    shares = counts / counts.sum()
    print(", ".join("%d: %.4f" % (k, shares[k]) for k in range(br.N_FEATURES)))
    assert (shares >= 0.005).all(), shares


def test_time_zero_is_the_oriented_overlap(cornell, cornell_sets):
    """t == 0 iff oriented_ref's statement accepts some triangle for the first sixteen floats, bit for bit"""
    verts, idx, mats = cornell
    for name in ("overlap", "contain", "zero_d"):
        c, rec = cornell_sets(name)
        touching = rec[:, 0].view(np.float32) == 0
        counts, prims, any_ = ot.overlap_records(c[:, :16], verts, idx, max_prims=1)
        assert np.array_equal(touching, any_.astype(bool)), name
        assert np.array_equal(rec[touching, 1], prims[touching, 0]), name          # and the winner is the lowest overlapping triangle
        assert touching.sum() >= 100, name
    c, rec = cornell_sets("zero_d")
    t = rec[:, 0].view(np.float32)
    assert (c[:, 16:19] == 0).all() and np.isin(t, (0.0, -1.0)).all() and 0.2 <= (t == 0).mean() <= 0.8
    assert (cornell_sets("contain")[1][:, 0] == 0).all()


ROUTE_CASTS = 250          # the route is twelve brute forces per cast


def test_the_twelve_triangle_route(cornell, cornell_sets):
    """What callers do today: pt_query_triangle_cast's statement on the 12 n surface triangles and a reduction.  On "contain" the solid
    box starts with whole triangles inside it and its surface may touch nothing: the route reports no impact or a later one.  Outside
    start overlaps the two routes agree in float64, within the bisection's bar."""
    RES_DIST = 1e-10
    verts, idx, mats = cornell
    shares = {}
    for name in ("contain", "links"):
        c, rec = cornell_sets(name)
        c, rec = c[:ROUTE_CASTS], rec[:ROUTE_CASTS]
        t = rec[:, 0].view(np.float32).astype(np.float64)
        route = br.twelve_triangle_route(c, verts, idx, mats)
        wrong = (t >= 0) & ((route < 0) | (route > t * (1.0 + 2.0 ** -12) + 2.0 ** -12))
        shares[name] = wrong.mean()
        print("%s: the 12-triangle route reports no impact or a later one for %.3f of the first %d casts" % (name, wrong.mean(), ROUTE_CASTS))
    assert shares["contain"] > 0.0
    c, rec = cornell_sets("aimed")
    c = c[:ROUTE_CASTS]
    v0, e1, e2 = (a.astype(np.float64) for a in nr.records_of_scene(verts, idx))
    A, cc, hh, dd, _ = br.parts(c, np.float64)
    t64, w64 = np.full(c.shape[0], np.inf), np.zeros(c.shape[0], np.int64)
    for start in range(0, c.shape[0], 50):
        sl = slice(start, start + 50)
        t = br.box_triangle(A[sl, None], cc[sl, None], hh[sl, None], dd[sl, None], v0[None], e1[None], e2[None])[0]
        t64[sl], w64[sl] = t.min(axis=1), t.argmin(axis=1)
    route64 = br.twelve_triangle_route_f64(c, verts, idx)
    assert np.array_equal(np.isfinite(t64), np.isfinite(route64)) and np.array_equal(t64 == 0, route64 == 0)
    moving = (t64 > 0) & np.isfinite(t64)
    assert moving.sum() >= 100
    tm, wm = t64[moving], w64[moving]
    res = 1e-15 * np.maximum(tm, 1.0)
    for _ in range(60):          # the bisection's resolution: widened until the box one step earlier is clear of the winner by RES_DIST
        before = np.maximum(tm - res, 0.0)
        gap = br.box_triangle_distance_f64(A[moving], cc[moving] + dd[moving] * before[:, None], hh[moving], v0[wm], v0[wm] + e1[wm], v0[wm] + e2[wm])
        res = np.where((gap > RES_DIST) | (before == 0.0), res, 2.0 * res)
    err = np.abs(route64[moving] - tm)
    print("aimed: %d moving casts, largest |12-triangle t - box t| %.3e of max(t, 1), %.3f of the bisection's resolution" % (moving.sum(), (err / np.maximum(tm, 1.0)).max(), (err / res).max()))
    assert (err <= BISECTION_MULTIPLE * res).all(), float((err / res).max())


def test_ties_go_to_the_lowest_triangle_index():
    """Two copies of one triangle: every time of impact is the same bits.  Whichever copy the index buffer lists first is triangle 0 and wins."""
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1], [0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32)
    casts = np.concatenate([_cast((1, 1, 5), (0.5, 1, 0.7), R3, (0.1, 0.2, -1)), _cast((2, -5, 0), (1, 1, 1), R45Z, (0, 1, 0)), _cast((-5, -4, 1), (1, 0.5, 0.25), R3, (1, 0.8, -0.2))])
    for idx in (np.array([0, 1, 2, 3, 4, 5], np.uint32), np.array([3, 4, 5, 0, 1, 2], np.uint32)):
        v0, e1, e2 = nr.records_of_scene(verts, idx)
        A, c, h, d, _ = br.parts(casts)
        t = br.box_triangle(A[:, None], c[:, None], h[:, None], d[:, None], v0[None], e1[None], e2[None])[0]
        assert np.array_equal(t[:, 0].view(np.uint32), t[:, 1].view(np.uint32)) and np.isfinite(t).all()
        rec = br.box_records(casts, verts, idx, np.array([3, 4], np.uint32))
        assert (rec[:, 1] == 0).all() and (rec[:, 3] == 3).all()


def test_casts_that_miss_before_any_traversal():
    good = _cast((1, 1, 5), (1, 1, 1), EYE, (0, 0, -1), 10.0)[0]
    bad, why = br.bad_casts(good)
    assert bad.shape[0] == 54 + 6 + 4 + 1
    ok = br.castable(bad)
    assert not ok.any(), [w for w, k in zip(why, ok) if k]
    assert np.array_equal(br.box_records(bad, TRI[0], TRI[1], np.zeros(1, np.uint32)), br.miss_records(bad.shape[0]))
    allowed = np.array([good] * 5, np.float32)
    allowed[1, 19] = np.inf
    allowed[2, 12:15] = -0.0             # half extents of zero, whatever their sign bit
    allowed[3, 16:19] = 0.0              # d = 0 is a cast: it misses by the test, not before it
    allowed[4, 15] = np.nan              # the sixteenth float decides nothing
    assert br.castable(allowed).all()
    rec = br.box_records(allowed, TRI[0], TRI[1], np.zeros(1, np.uint32))
    assert (rec[[0, 1, 2, 4], 1] == 0).all() and rec[3, 1] == 0xFFFFFFFF
    assert np.array_equal(rec[0], rec[4])
    assert np.array_equal(br.box_records(allowed, TRI[0], np.zeros(0, np.uint32), np.zeros(0, np.uint32)), br.miss_records(5))


def test_sets_are_what_they_say(cornell, cornell_sets):
    verts, idx, mats = cornell
    lo, hi = nr.scene_box(verts, idx)
    for name in br.CAST_SETS:
        c, rec = cornell_sets(name)
        assert c.shape == (br.SET_SIZE, 20) and c.dtype == np.float32, name
        if name not in ("short",):           # fixed seeds ("short" is made from a brute force: once is enough)
            assert np.array_equal(c.view(np.uint32), br.cast_set(name, verts, idx, None, mats).view(np.uint32)), name
        if name not in ("bad", "tolerance"):
            assert br.castable(c).all(), name
    c, rec = cornell_sets("bad")
    bad = ~br.castable(c)
    assert bad.sum() == len(range(1, br.SET_SIZE, 3)) and np.array_equal(rec[bad], br.miss_records(int(bad.sum())))
    assert (rec[~bad, 1] != 0xFFFFFFFF).mean() >= 0.9
    c, rec = cornell_sets("tolerance")
    ok = br.castable(c)
    inside = ot.tolerance_kinds() < 3
    assert np.array_equal(ok, inside) and np.array_equal(rec[~ok], br.miss_records(int((~ok).sum()))) and (rec[ok, 1] != 0xFFFFFFFF).mean() >= 0.5
    c, rec = cornell_sets("outside")
    centre = c[:, [3, 7, 11]]
    assert ((centre < lo) | (centre > hi)).any(axis=1).all()
    t = rec[:, 0].view(np.float32)
    assert (t > 0).mean() >= 0.25 and (t < 0).mean() >= 0.2 and not (t == 0).any()
    c, rec = cornell_sets("short")
    t = rec[:, 0].view(np.float32)
    assert (t >= 0).mean() >= 0.25 and (t < 0).mean() >= 0.2 and (t == c[:, 19]).mean() >= 0.1          # tmax = t: the closed end decides
    base_t = cornell_sets("aimed")[1][:, 0].view(np.float32)
    below = (np.arange(br.SET_SIZE) % 3 == 0) & (base_t > 0)
    assert (t[below] != base_t[below]).all()                       # one ulp short of the impact: another triangle later, or none
    c, rec = cornell_sets("links")
    h = np.sort(c[:, 12:15], axis=1)
    assert (h[:, 2] >= 2.4 * h[:, 1]).all()
    c, rec = cornell_sets("cells")
    assert (c[:, 12] == c[:, 13]).all() and (c[:, 13] == c[:, 14]).all()
    c, rec = cornell_sets("flat")
    assert ((c[:, 12:15] == 0).sum(axis=1) >= 1).mean() >= 0.7 and all((((c[:, 12:15] == 0).sum(axis=1)) == k).sum() >= 100 for k in (1, 2, 3))
    assert (rec[:, 0].view(np.float32) > 0).mean() >= 0.3
    c, rec = cornell_sets("identity")
    assert np.array_equal(c[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], np.broadcast_to(np.eye(3, dtype=np.float32).reshape(9), (br.SET_SIZE, 9)))
    c, rec = cornell_sets("axis_turns")
    assert np.isin(c[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], (-1.0, 0.0, 1.0)).all() and (rec[:, 0].view(np.float32) > 0).mean() >= 0.2
    c, rec = cornell_sets("grazing")
    assert (rec[:, 0].view(np.float32) > 0).mean() >= 0.5


def test_build_lists_and_abi():
    assert "boxcast.hip" in _build.HIP_SOURCES
    for name in ("boxcast.h", "boxcast_device.h", "oriented_device.h", "overlap_device.h"):
        assert name in _build.HIP_HEADERS, name
    for name in ("boxcast.hip", "boxcast.h", "boxcast_device.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
        assert os.path.exists(os.path.join(_build.CSRC, name)), name
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    for name in ("pt_query_box_cast", "pt_query_box_cast_any"):
        assert name in _native.ABI_SYMBOLS
    assert "pt_debug_box_cast_visits" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert "typedef struct { float t; uint32_t prim; float feature; uint32_t material; float nx, ny, nz, pad0; float cx, cy, cz, pad1; } pt_box_cast_hit;" in hdr
    assert "int pt_query_box_cast(pt_ctx* ctx, const float* casts, size_t n, pt_box_cast_hit* hits);" in hdr
    assert "int pt_query_box_cast_any(pt_ctx* ctx, const float* casts, size_t n, uint8_t* blocked);" in hdr
    test_hdr = open(os.path.join(ROOT, "include", "acgpt_test.h")).read()
    assert "int pt_debug_box_cast_visits(pt_ctx* ctx, const float* casts, size_t n, pt_box_cast_hit* hits, uint32_t* visits, uint32_t mode);" in test_hdr
    assert "static_assert(sizeof(pt_box_cast_hit) == 48" in open(os.path.join(_build.CSRC, "capi_query.hip")).read()
    # the leaf reuses the static query's record and test by inclusion
    dev = open(os.path.join(_build.CSRC, "boxcast_device.h")).read()
    assert '#include "oriented_device.h"' in dev and "tri_box_overlap(" in dev


def test_symbols_are_exported_and_bound(built):
    L = _native.hip()
    for name in ("pt_query_box_cast", "pt_query_box_cast_any", "pt_debug_box_cast_visits"):
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (6 if name == "pt_debug_box_cast_visits" else 4), name
    assert L.pt_abi_version() == 4
    assert L.pt_kernel_source_hash().decode() == "0ae80f7fe3d9b38b"
    assert L.pt_query_box_cast(None, None, 0, None) != 0                     # a null context is refused before anything else
    assert L.pt_query_box_cast_any(None, None, 0, None) != 0


def test_box_cast_kernels_fit_the_register_file(built):
    """The eight k_query_obox_toi instantiations (two node formats; the product's, and the counting twin with and without the extra
    axes) and the two any-hit kernels: no private segment, no spilled register, three waves per SIMD at the least"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_query_obox_toi" in k["name"]]
    main = [k for k in rows if "k_query_obox_toi<" in k["name"]]
    assert len(main) == 6 and len(rows) == 8, [k["name"] for k in rows]
    for k in rows:
        assert "cast" not in k["name"], k["name"]             # tests/test_tricast_host.py counts kernels by that substring
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] <= 168, k
    print("vgpr_count: %s" % sorted(set(k["vgpr_count"] for k in rows)))


def test_queryboxcast_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for bad in (np.zeros((4, 8), np.float32), np.zeros(20, np.float32), np.zeros((2, 20, 1), np.float32), [[1, 2]], np.zeros((4, 16), np.float32)):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.queryBoxCast(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.queryBoxCast(state, np.zeros((2, 20), np.complex64))
    boxes = pt.orientedBoxes(np.zeros((2, 3)), 1.0, np.eye(3))
    with pytest.raises(pt.PathTracerError, match="directions go with"):
        pt.queryBoxCast(state, np.zeros((2, 20), np.float32), np.ones((2, 3)))
    for bad in (np.ones((3, 3)), np.ones((2, 4)), np.ones(4), np.ones((2, 3), np.complex64)):
        with pytest.raises(pt.PathTracerError, match="directions or one"):
            pt.queryBoxCast(state, boxes, bad)
    for bad in (-1.0, float("nan"), [1.0, 2.0, 3.0], np.ones((2, 2))):
        with pytest.raises(pt.PathTracerError, match="tmax"):
            pt.queryBoxCast(state, boxes, np.ones(3), tmax=bad)
    empty = pt.queryBoxCast(state, np.zeros((0, 20), np.float32))
    assert sorted(empty) == ["feature", "material", "normal", "point", "prim", "t"]
    assert empty["t"].shape == (0,) and empty["point"].shape == (0, 3) and empty["normal"].shape == (0, 3) and empty["prim"].dtype == np.uint32
    assert pt.queryBoxCast(state, np.zeros((0, 16)), np.zeros((0, 3)), any_hit=True).shape == (0,)
    with pytest.raises(pt.PathTracerError, match=r"local_box is \(lo, hi\)"):
        pt.poseBoxCasts(state, np.zeros((1, 12), np.float32), 3.0, np.ones(3))
    with pytest.raises(pt.PathTracerError, match="lo and hi"):
        pt.poseBoxCasts(state, np.zeros((1, 12), np.float32), ((1, 1, 1), (0, 0, 0)), np.ones(3))
    torch = pytest.importorskip("torch")
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.queryBoxCast(state, torch.zeros((4, 20), dtype=torch.float32))
    with pytest.raises(pt.PathTracerError, match="a tensor holds whole records"):
        pt.queryBoxCast(state, torch.zeros((4, 20), dtype=torch.float32), np.ones(3))
    with pytest.raises(pt.PathTracerError, match="tensor poses take"):
        pt.poseBoxCasts(state, torch.zeros((4, 12), dtype=torch.float32), ((0, 0, 0), (1, 1, 1)), np.ones(3))


def test_box_cast_contacts():
    casts = np.concatenate([_cast((1, 1, 5), (1, 1, 1), EYE, (0, 0, -1)), _cast((1, 1, 0.5), (1, 1, 1), EYE, (0, 0, -1)), _cast((9, 9, 5), (1, 1, 1), EYE, (0, 0, -1)),
                            _cast((8, -0.5, 0.25), (1, 1, 1), EYE, (-2, 1, 0))])
    col = br.columns(br.box_records(casts, TRI[0], TRI[1], np.zeros(1, np.uint32)))
    centre, normal, point, start, slide = pt.boxCastContacts(col, casts)
    assert np.array_equal(centre[0], [1, 1, 1]) and np.array_equal(normal[0], [0, 0, 1]) and np.array_equal(point[0], [0, 0, 0]) and not start[0]
    assert np.array_equal(slide[0], [0, 0, 0])                                  # head on: nowhere to go
    assert start[1] and np.array_equal(centre[1], [1, 1, 0.5]) and np.array_equal(normal[1], [0, 0, 0]) and np.array_equal(slide[1], [0, 0, -1])
    assert all(np.isnan(x[2]).all() for x in (centre, normal, point, slide)) and not start[2]
    assert np.array_equal(centre[3], [5, 1, 0.25]) and np.array_equal(normal[3], [1, 0, 0]) and np.array_equal(slide[3], [0, 1, 0])       # slides along the face
    for x in (centre, normal, point, slide):
        assert x.dtype == np.float32 and x.shape == (4, 3)
    with pytest.raises(pt.PathTracerError, match="expected the"):
        pt.boxCastContacts(col, casts[:, :16])
