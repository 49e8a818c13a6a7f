"""pt_query_capsule_cast without a GPU: the NumPy statement of the time of impact (tests/capsule_ref.py) on hand-checked casts, its
float64 evaluation against a bisection that knows nothing of the decomposition, fp32 against float64 on the Cornell box, what the
reference alone must show (every group of features wins its share, p1 = p0 is the sphere sweep, t = 0 is a clearance <= 0, the tie
rule, the casts that miss before any traversal, what five sampled spheres get wrong), the interface (build lists, prototypes, symbols,
kernel resources) and the argument checks of queryCapsuleCast that need no device."""
import os
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import capsule_ref as cr
import nearest_ref as nr
import segment_ref as sg
import sweep_ref as sw

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = os.path.join(pt.SCENES, "cornell_box.obj")

# fp32 against float64 (scene units, the box is 556 wide; DESIGN.md section 39 quotes both figures).  The yardstick is the sphere sweep's:
# the largest float64 | dist(o + d * t32, winning triangle) - r | over the hits with t32 > 0 of sweep_ref's "aimed" set, measured with
# sweep_ref as it stands before this query existed, 8.93e-5.  The capsule's bar is that figure times AXIS_MARGIN = 2: the axis edge and
# the side face run the same edge and face forms on a vector as long as the capsule, whose projections lose as much again as a triangle's
# own edge does (csrc/capsule.h derives R the same way).  Not taken from anything the capsule statement gives.
SPHERE_CONTACT_MEASURED = 8.93e-5
AXIS_MARGIN = 2.0
# the float64 statement against the bisection: at most this many times the bisection's own resolution (below)
BISECTION_MULTIPLE = 4.0

TRI = (np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32), np.array([0, 1, 2], np.uint32))
INF = np.inf


def _cast(p0, p1, d, r, tmax=INF):
    return np.array([tuple(p0) + (r,) + tuple(p1) + (tmax,) + tuple(d) + (np.nan,)], np.float32)       # the twelfth float decides nothing


def _one(cast, verts=TRI[0], idx=TRI[1], mats=(0x05000007,)):
    rec, kind = cr.capsule_records(cast, verts, idx, np.array(mats, np.uint32), kinds=True)
    return rec[0], rec.view(np.float32)[0], int(kind[0])


def test_hand_checked_casts_of_one_triangle():
    """A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0).  One cast per group of features; every t below follows from the picture, and all but
    the parameter 1 / 3 are exact in fp32."""
    third = F(1.0) / F(3.0)
    cases = [
        # p0, p1, d, r -> t, group, s, feature of pt_query_segments, contact point
        ((1, 1, 0.5), (1, 1, 3), (0, 0, -1), 1.0, 0.0, cr.START, 0.0, 0, (1, 1, 0)),              # starts in contact
        ((1, 1, 5), (1, 1, 8), (0, 0, -1), 1.0, 4.0, cr.P0_FACE, 0.0, 0, (1, 1, 0)),               # upright over the face, p0 below
        ((1, 1, 8), (1, 1, 5), (0, 0, -2), 1.0, 2.0, cr.P1_FACE, 1.0, 1, (1, 1, 0)),               # p1 below, d of length 2
        ((-5, 0, 0), (-8, 0, 3), (1, 0, 0), 1.0, 4.0, cr.P0_VERTEX, 0.0, 0, (0, 0, 0)),            # p0's sphere against A, the axis trailing
        ((-8, 0, 3), (-5, 0, 0), (1, 0, 0), 1.0, 4.0, cr.P1_VERTEX, 1.0, 1, (0, 0, 0)),
        ((2, -5, 0), (2, -8, 3), (0, 1, 0), 1.0, 4.0, cr.P0_EDGE, 0.0, 0, (2, 0, 0)),              # p0's sphere against edge AB
        ((2, -8, 3), (2, -5, 0), (0, 1, 0), 1.0, 4.0, cr.P1_EDGE, 1.0, 1, (2, 0, 0)),
        # the cylinder's side meets B a third of the way along the axis, between the first two of five sample spheres (s = 0, 1/4, ...)
        ((9, 0, -1), (9, 0, 2), (-1, 0, 0), 1.0, 4.0, cr.AXIS_EDGE, third, 2, (4, 0, 0)),
        # edge against edge: the upright axis crosses AB's line at x = 2 and meets it with its side
        ((2, -5, -1), (2, -5, 2), (0, 1, 0), 1.0, 4.0, cr.SIDE_FACE, third, 2, (2, 0, 0)),
        ((1, 1, 5), (1, 1, 8), (0, 0, -1), 0.0, 5.0, cr.P0_FACE, 0.0, 5, (1, 1, 0)),               # radius 0: a swept segment, its end on the triangle (the crossing feature)
        ((1, 1, 5), (1, 1, 8), (0, 0, -1), 1.0, 4.0, cr.P0_FACE, 0.0, 0, (1, 1, 0)),               # tmax on the contact (set below): closed
    ]
    for i, (p0, p1, d, r, t, group, s, feat, c) in enumerate(cases):
        u32, f, k = _one(_cast(p0, p1, d, r, 4.0 if i == len(cases) - 1 else INF))
        assert f[0] == F(t) and k == group, (p0, p1, f[0], cr.GROUP_NAMES[k])
        assert u32[1] == 0 and u32[7] == 7, p0                   # the material id without the flags above bit 24
        assert abs(f[2] - F(s)) <= 2.0 ** -22 and f[3] == F(feat) and tuple(f[4:7]) == c, (p0, p1, f[2:7])
    # five spheres on the axis of the axis-edge case all pass B: the nearest, at z = -1 / 4, touches it a little later
    c = _cast((9, 0, -1), (9, 0, 2), (-1, 0, 0), 1.0)
    sampled = cr.sampled_spheres(c, TRI[0], TRI[1], np.array([7], np.uint32))
    assert sampled[0] > F(4.0)
    misses = [((1, 1, 5), (1, 1, 8), (0, 0, -1), 1.0, 3.5), ((1, 1, 5), (1, 1, 8), (0, 0, 1), 1.0, INF), ((9, 9, 5), (9, 9, 8), (0, 0, -1), 1.0, INF),
              ((1, 1, 5), (1, 1, 8), (0, 0, 0), 1.0, INF)]
    for p0, p1, d, r, tmax in misses:
        u32, f, k = _one(_cast(p0, p1, d, r, tmax))
        assert np.array_equal(u32, cr.miss_records(1)[0]) and k == cr.NONE, (p0, d)
    assert _one(_cast((1, 1, 0.5), (1, 1, 3), (0, 0, 0), 1.0, 0.0))[1][0] == 0.0     # d = 0 and tmax = 0: the start overlap answers
    # an axis that pierces the triangle at more than r from both ends starts in contact: no sphere on its ends says so
    u32, f, k = _one(_cast((1, 1, -3), (1, 1, 5), (1, 0, 0), 0.5))
    assert f[0] == 0.0 and k == cr.START and f[3] == 5.0
    assert pt.CAPSULE_CAST_DTYPE.itemsize == 32 and [pt.CAPSULE_CAST_DTYPE.fields[k][1] for k in pt.CAPSULE_CAST_DTYPE.names] == [0, 4, 8, 12, 16, 28]
    assert np.array_equal(cr.miss_records(1)[0], np.array([0xBF800000, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0xFFFFFFFF], np.uint32))
    assert np.array_equal(cr.miss_records(3), sg.miss_records(3))


@pytest.fixture(scope="module")
def cornell():
    obj = pt.TinyObjWrapper(BOX)
    cam = pt.initCamera()
    cam.setAspectRatio(np.float32(97) / np.float32(61))
    camera = (cam.eye(),) + tuple(cam.UVWFrame())
    return obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), camera


@pytest.fixture(scope="module")
def cornell_sets(cornell):
    """name -> (casts, records, groups) by the fp32 brute force: computed once per set, shared, never written"""
    verts, idx, mats, camera = cornell
    cache = {}

    def get(name):
        if name not in cache:
            c = cr.cast_set(name, verts, idx, camera, mats)
            rec, kind = cr.capsule_records(c, verts, idx, mats, kinds=True)
            for a in (c, rec, kind):
                a.setflags(write=False)
            cache[name] = (c, rec, kind)
        return cache[name]
    return get


def test_float64_statement_against_an_independent_bisection(cornell, cornell_sets):
    """The decomposition is the geometric truth.  The distance between the moving axis and a triangle is convex in t, so
    distance <= r holds on one interval; its lower end by bisection on segment_f64 knows nothing of prisms, cylinders and offset
    planes.  The bisection's own resolution, per cast: its last bracket, widened until the distance one step before it exceeds r
    by more than RES_DIST = 1e-10 — what float64 leaves of a distance at coordinates of ~550, a hundred times over.  On a graze that
    is a long way in t, and it is the bisection that cannot tell, not the statement.  The bar is BISECTION_MULTIPLE times that."""
    RES_DIST = 1e-10
    verts, idx, mats, camera = cornell
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    worst, worst_rel, total = 0.0, 0.0, 0
    for name in cr.COVERAGE_SETS:
        c, rec, kind = cornell_sets(name)
        hit = rec[:, 1] != 0xFFFFFFFF
        c, w = c[hit], rec[hit, 1].astype(np.int64)
        t64, group = cr.impact_f64(c, v0[w], e1[w], e2[w])
        tb, width = cr.bisect_impact_f64(c, v0[w], e1[w], e2[w])
        h64, hb = np.isfinite(t64), np.isfinite(tb)
        differ = h64 != hb
        if differ.any():         # the two may call a cast differently only on a graze: the closest approach within 1e-9 of r
            graze = np.abs(cr.axis_distance_f64(np.where(np.isinf(c[differ]), 1e30, c[differ]), v0[w[differ]], e1[w[differ]], e2[w[differ]]) - c[differ, 3].astype(np.float64))
            assert (graze <= 1e-9).all(), (name, graze.max())
        both = h64 & hb & (tb > 0)
        assert both.mean() >= 0.2, (name, both.mean())
        cb, wb, tbb = c[both], w[both], tb[both]
        res = np.maximum(width[both], 1e-15 * np.maximum(tbb, 1.0))
        r64 = cb[:, 3].astype(np.float64)
        for _ in range(60):
            before = np.maximum(tbb - res, 0.0)
            clear = (cr.distance_at_f64(cb, v0[wb], e1[wb], e2[wb], before) - r64 > RES_DIST) | (before == 0.0)
            res = np.where(clear, res, 2.0 * res)
        err = np.abs(t64[both] - tbb)
        assert (err <= BISECTION_MULTIPLE * res).all(), (name, float((err / res).max()))
        # the groups' start overlaps agree too
        assert np.array_equal(t64[h64 & hb] == 0, tb[h64 & hb] == 0), name
        rel = err / np.maximum(tbb, 1.0)
        worst, worst_rel, total = max(worst, float((err / res).max())), max(worst_rel, float(rel.max())), total + int(both.sum())
        print("%s: %d moving hits, largest |t - bisection| %.3e of max(t, 1), %.3f of the bisection's resolution" % (name, both.sum(), rel.max(), (err / res).max()))
    print("all four sets: %d hits, largest relative difference %.3e, largest multiple of the resolution %.3f (bar %.1f)" % (total, worst_rel, worst, BISECTION_MULTIPLE))


def _sphere_contact(cornell):
    """the sphere sweep's figure on its "aimed" set, as tests/test_sweep_host.py measures it"""
    verts, idx, mats, camera = cornell
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    s = sw.sweep_set("aimed", verts, idx)
    rec = sw.sweep_records(s, verts, idx, mats)
    t32, p32 = rec[:, 0].view(np.float32), rec[:, 1].astype(np.int64)
    hit = t32 > 0
    s64 = s.astype(np.float64)
    centre = s64[hit, 0:3] + s64[hit, 3:6] * t32[hit, None].astype(np.float64)
    a = v0[p32[hit]].astype(np.float64)
    return float(np.abs(nr.closest_f64(centre, a, a + e1[p32[hit]], a + e2[p32[hit]])[0] - s64[hit, 6]).max())


def test_fp32_statement_against_float64_on_the_cornell_sets(cornell, cornell_sets):
    """Where fp32 says the capsule stops, float64 finds its axis at the radius from the winning triangle, within the sphere sweep's own
    figure times AXIS_MARGIN; and the quoted figure is what sweep_ref gives now."""
    verts, idx, mats, camera = cornell
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    sphere = _sphere_contact(cornell)
    print("sphere sweep, aimed: largest |dist - r| %.3e (quoted %.3e)" % (sphere, SPHERE_CONTACT_MEASURED))
    assert SPHERE_CONTACT_MEASURED / 1.05 <= sphere <= SPHERE_CONTACT_MEASURED * 1.05
    bar = SPHERE_CONTACT_MEASURED * AXIS_MARGIN
    worst = 0.0
    for name in ("aimed", "grazing", "upright", "links", "parallel", "along"):
        c, rec, kind = cornell_sets(name)
        t32, w = rec[:, 0].view(np.float32), rec[:, 1].astype(np.int64)
        hit = t32 > 0
        assert hit.sum() >= 200, name
        err = np.abs(cr.distance_at_f64(c[hit], v0[w[hit]], e1[w[hit]], e2[w[hit]], t32[hit]) - c[hit, 3].astype(np.float64))
        print("%s: %d moving hits, largest |dist - r| %.3e by %s (bar %.3e)" % (name, hit.sum(), err.max(), cr.GROUP_NAMES[kind[hit][np.argmax(err)]], bar))
        worst = max(worst, float(err.max()))
        assert err.max() <= bar, name
    print("largest over the six sets %.3e" % worst)


def test_every_group_of_features_wins_its_share(cornell_sets):
    counts = np.zeros(10)
    for name in cr.COVERAGE_SETS:
        c, rec, kind = cornell_sets(name)
        counts += np.bincount(kind, minlength=10)
        assert np.unique(rec[:, 1]).size >= 32, name
    shares = counts / (len(cr.COVERAGE_SETS) * cr.SET_SIZE)
    print(", ".join("%s %.3f" % (cr.GROUP_NAMES[g], shares[g]) for g in cr.GROUPS))
    assert all(shares[g] >= 0.01 for g in cr.GROUPS), shares


def test_a_point_capsule_is_the_sphere_sweep(cornell):
    """p1 = p0: t and prim are sweep_ref's bit for bit wherever neither statement starts in contact (there the winner is the lowest
    index among all triangles in contact for both, but the two start tests are different statements).  Counted over the three sets
    together the reference leaves out fewer than 15 % ("aimed" alone starts a fifth in contact: an eighth by construction, the rest
    because the walls are near)."""
    verts, idx, mats, camera = cornell
    out_n, n = 0, 0
    for name in ("aimed", "grazing", "camera"):
        s = sw.sweep_set(name, verts, idx, camera, mats)
        rs = sw.sweep_records(s, verts, idx, mats)
        rc = cr.capsule_records(cr.from_sweeps(s), verts, idx, mats)
        out = (rs[:, 0] == 0) | (rc[:, 0] == 0)
        assert np.array_equal(rs[~out, 0:2], rc[~out, 0:2]), name
        assert (rs[~out, 1] != 0xFFFFFFFF).mean() >= 0.25, name
        out_n, n = out_n + int(out.sum()), n + s.shape[0]
    print("left out %.4f" % (out_n / n))
    assert out_n / n < 0.15


def test_time_zero_is_a_clearance_of_at_most_zero(cornell, cornell_sets):
    """t = 0 iff capsuleClearance's statement — pt_query_segments' distance with no limit, minus the radius — is <= 0"""
    verts, idx, mats, camera = cornell
    for name in ("aimed", "inside", "zero_d", "upright"):
        c, rec, kind = cornell_sets(name)
        g = c[:, 0:8].copy()
        g[:, 3] = np.inf
        seg = sg.segment_records(g, verts, idx, mats)
        clearance = seg[:, 0].view(np.float32) - c[:, 3]
        touching = rec[:, 0].view(np.float32) == 0
        assert np.array_equal(touching, clearance <= 0), name
        assert touching.sum() >= 100 and (name in ("inside",) or (~touching).sum() >= 100), name
    c, rec, kind = cornell_sets("inside")
    assert (kind == cr.START).all()
    # a quarter of "inside" pierces: pt_query_segments' crossing feature, at more than r from both ends of the axis
    feat = rec[:, 3].view(np.float32)
    assert (feat == 5).mean() >= 0.2


def test_ties_go_to_the_lowest_triangle_index():
    """Two copies of one triangle: every time of impact is the same bits.  Whichever copy the index buffer lists first is triangle 0 and wins."""
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1], [0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32)
    casts = np.concatenate([_cast((1, 1, 5), (2, 1.5, 7), (0.1, 0.2, -1), 0.7), _cast((2, -5, -1), (2.5, -5, 2), (0, 1, 0), 1.0), _cast((-5, -4, 1), (-6, -4, 2), (1, 0.8, -0.2), 0.5)])
    for idx in (np.array([0, 1, 2, 3, 4, 5], np.uint32), np.array([3, 4, 5, 0, 1, 2], np.uint32)):
        v0, e1, e2 = nr.records_of_scene(verts, idx)
        t = cr.capsule_triangle(casts[:, None, 0:3], casts[:, None, 4:7], casts[:, None, 8:11], casts[:, 3, None], v0[None], e1[None], e2[None])[0]
        assert np.array_equal(t[:, 0].view(np.uint32), t[:, 1].view(np.uint32)) and np.isfinite(t).all()
        rec = cr.capsule_records(casts, verts, idx, np.array([3, 4], np.uint32))
        assert (rec[:, 1] == 0).all() and (rec[:, 7] == 3).all()


def test_casts_that_miss_before_any_traversal():
    good = _cast((1, 1, 5), (1, 1, 8), (0, 0, -1), 1.0, 10.0)[0]
    bad, why = cr.bad_casts(good)
    assert bad.shape[0] == 27 + 1 + 5 + 4
    ok = cr.castable(bad)
    assert not ok.any(), [w for w, k in zip(why, ok) if k]
    assert np.array_equal(cr.capsule_records(bad, TRI[0], TRI[1], np.zeros(1, np.uint32)), cr.miss_records(bad.shape[0]))
    allowed = np.array([good] * 6, np.float32)
    allowed[1, 7] = np.inf
    allowed[2, 3] = -0.0                 # a radius of zero, whatever its sign bit
    allowed[3, 8:11] = 0.0               # d = 0 is a cast: it misses by the test, not before it
    allowed[4, 4:7] = allowed[4, 0:3]    # p1 = p0 is a sphere
    allowed[5, 11] = np.inf              # the twelfth float decides nothing
    assert cr.castable(allowed).all()
    rec = cr.capsule_records(allowed, TRI[0], TRI[1], np.zeros(1, np.uint32))
    assert (rec[[0, 1, 2, 4, 5], 1] == 0).all() and rec[3, 1] == 0xFFFFFFFF
    assert np.array_equal(cr.capsule_records(allowed, TRI[0], np.zeros(0, np.uint32), np.zeros(0, np.uint32)), cr.miss_records(6))


def test_sets_are_what_they_say(cornell, cornell_sets):
    verts, idx, mats, camera = cornell
    lo, hi = nr.scene_box(verts, idx)
    diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    for name in cr.CAST_SETS:
        c, rec, kind = cornell_sets(name)
        assert c.shape == (cr.SET_SIZE, 12) and c.dtype == np.float32, name
        if name not in ("short",):           # fixed seeds ("short" is made from a brute force: once is enough)
            assert np.array_equal(c.view(np.uint32), cr.cast_set(name, verts, idx, camera, mats).view(np.uint32)), name
        if name != "bad":
            assert cr.castable(c).all(), name
    c, rec, kind = cornell_sets("bad")
    bad = ~cr.castable(c)
    assert bad.sum() == len(range(1, cr.SET_SIZE, 3)) and np.array_equal(rec[bad], cr.miss_records(int(bad.sum())))
    assert (rec[~bad, 1] != 0xFFFFFFFF).mean() >= 0.9
    c, rec, kind = cornell_sets("zero_d")
    t = rec[:, 0].view(np.float32)
    assert (c[:, 8:11] == 0).all() and np.isin(t, (0.0, -1.0)).all() and 0.2 <= (t == 0).mean() <= 0.8
    c, rec, kind = cornell_sets("outside")
    assert ((c[:, 0:3] < lo) | (c[:, 0:3] > hi)).any(axis=1).all() and ((c[:, 4:7] < lo) | (c[:, 4:7] > hi)).any(axis=1).all()
    t = rec[:, 0].view(np.float32)
    assert (t > 0).mean() >= 0.25 and (t < 0).mean() >= 0.2 and not (t == 0).any()
    c, rec, kind = cornell_sets("short")
    t = rec[:, 0].view(np.float32)
    assert (t >= 0).mean() >= 0.25 and (t < 0).mean() >= 0.2 and (t == c[:, 7]).mean() >= 0.1          # tmax = 1 x t: the closed end decides
    c, rec, kind = cornell_sets("point")
    assert np.array_equal(c[:, 0:3], c[:, 4:7])
    c, rec, kind = cornell_sets("along")
    a, d = (c[:, 4:7] - c[:, 0:3]).astype(np.float64), c[:, 8:11].astype(np.float64)
    assert (np.linalg.norm(np.cross(a, d), axis=1) <= 1e-6 * np.linalg.norm(a, axis=1) * np.linalg.norm(d, axis=1)).all()
    assert (rec[:, 0].view(np.float32) > 0).mean() >= 0.25
    c, rec, kind = cornell_sets("upright")
    a = c[:, 4:7] - c[:, 0:3]
    assert (a[:, 0] == 0).all() and (a[:, 2] == 0).all() and (a[:, 1] >= 1.99 * c[:, 3]).all() and (a[:, 1] <= 4.01 * c[:, 3]).all()
    assert (np.abs(c[:, 9]) <= 0.051 * np.hypot(c[:, 8], c[:, 10])).all() and (rec[:, 0].view(np.float32) > 0).mean() >= 0.4
    c, rec, kind = cornell_sets("links")
    length = np.linalg.norm((c[:, 4:7] - c[:, 0:3]).astype(np.float64), axis=1)
    assert (length >= 0.199 * diag).all() and (length <= 0.501 * diag).all()
    assert (np.abs((c[:, 4:7] - c[:, 0:3]) / length[:, None]).min(axis=1) >= 0.3).all()          # diagonal to the walls
    c, rec, kind = cornell_sets("parallel")
    assert (rec[:, 0].view(np.float32) > 0).mean() >= 0.3
    c, rec, kind = cornell_sets("aimed")
    assert np.isnan(c[::2, 11]).all()             # and the twelfth float is a NaN on every other cast


def test_five_sampled_spheres_miss_what_the_side_meets(cornell, cornell_sets):
    """What callers do today, on "grazing": five spheres along the axis through sweep_ref.  For the share printed here they report no
    impact or a later one: the README's motivating figure.  Never an earlier one: a sphere on the axis is part of the capsule."""
    verts, idx, mats, camera = cornell
    c, rec, kind = cornell_sets("grazing")
    t = rec[:, 0].view(np.float32)
    sampled = cr.sampled_spheres(c, verts, idx, mats)
    wrong = (t >= 0) & ((sampled < 0) | (sampled > t))
    print("grazing: five sampled spheres report no impact or a later one for %.3f of the casts (none at all for %.3f)" % (wrong.mean(), ((t >= 0) & (sampled < 0)).mean()))
    assert wrong.mean() >= 0.2
    moving = (t > 0) & (sampled >= 0)
    assert (sampled[moving] >= t[moving] * F(1.0 - 2.0 ** -12)).all()


def test_build_lists_and_abi():
    assert "capsule.hip" in _build.HIP_SOURCES
    for name in ("capsule.h", "sweep_device.h", "segment_device.h"):
        assert name in _build.HIP_HEADERS, name
    for name in ("capsule.hip", "capsule.h", "sweep_device.h", "segment_device.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
        assert os.path.exists(os.path.join(_build.CSRC, name)), name
    for name in ("pt_query_capsule_cast", "pt_query_capsule_cast_any"):
        assert name in _native.ABI_SYMBOLS
    assert "pt_debug_capsule_cast_visits" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert "typedef struct { float t; uint32_t prim; float s, feature; float cx, cy, cz; uint32_t material; } pt_capsule_cast_hit;" in hdr
    assert "int pt_query_capsule_cast(pt_ctx* ctx, const float* casts, size_t n, pt_capsule_cast_hit* hits);" in hdr
    assert "int pt_query_capsule_cast_any(pt_ctx* ctx, const float* casts, size_t n, uint8_t* blocked);" in hdr
    assert hdr.index("int pt_query_sweep_any(") < hdr.index("pt_capsule_cast_hit;") < hdr.index("pt_segment_hit;")          # the section after the swept spheres
    test_hdr = open(os.path.join(ROOT, "include", "acgpt_test.h")).read()
    assert "int pt_debug_capsule_cast_visits(pt_ctx* ctx, const float* casts, size_t n, pt_capsule_cast_hit* hits, uint32_t* visits, uint32_t mode);" in test_hdr
    assert "static_assert(sizeof(pt_capsule_cast_hit) == 32" in open(os.path.join(_build.CSRC, "capi_query.hip")).read()
    # the shared device functions live in the headers now, once
    for fn, header, unit in (("sweep_vertex", "sweep_device.h", "sweep.hip"), ("sweep_edge", "sweep_device.h", "sweep.hip"), ("sweep_face", "sweep_device.h", "sweep.hip"),
                             ("SegPoint segment_triangle", "segment_device.h", "segment.hip")):
        define = "__device__ __forceinline__ " + ("void " if fn.startswith("sweep") else "") + fn + "("
        assert define in open(os.path.join(_build.CSRC, header)).read(), fn
        assert define not in open(os.path.join(_build.CSRC, unit)).read(), fn
    # and the walk of the four cast families in cast_walk.h, once: the line slab, the child decode, the tie rule, the any-hit body
    assert "cast_walk.h" in _build.HIP_HEADERS and "cast_walk.h" not in _build.KERNEL_SOURCES
    walk = open(os.path.join(_build.CSRC, "cast_walk.h")).read()
    for text in ("__device__ __forceinline__ void cast_line_slab(", "__device__ __forceinline__ CastChild cast_child_hc(", "__device__ __forceinline__ CastChild cast_child_f32(",
                 "t_ == t && prim_ < prim", "fminf(x0, x1)", "(float)hx.y < 0.0f", "blocked[i] ="):
        assert walk.count(text) == 1, text
        for unit in ("sweep.hip", "capsule.hip", "boxcast.hip", "tricast_device.h", "tricast.hip"):
            assert text not in open(os.path.join(_build.CSRC, unit)).read(), (unit, text)


def test_symbols_are_exported_and_bound(built):
    L = _native.hip()
    for name in ("pt_query_capsule_cast", "pt_query_capsule_cast_any", "pt_debug_capsule_cast_visits"):
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (6 if name == "pt_debug_capsule_cast_visits" else 4), name
    assert L.pt_abi_version() == 4
    assert L.pt_query_capsule_cast(None, None, 0, None) != 0                     # a null context is refused before anything else
    assert L.pt_query_capsule_cast_any(None, None, 0, None) != 0


def test_capsule_kernels_fit_the_register_file(built):
    """The six k_query_capsule instantiations (two node formats; the product's, and the counting twin with and without the plane
    axis) and the two any-hit kernels: no private segment, no spilled register, four waves per SIMD at the least"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_query_capsule" in k["name"]]
    main = [k for k in rows if "k_query_capsule<" in k["name"]]
    assert len(main) == 6 and len(rows) == 8, [k["name"] for k in rows]
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] <= 128, k
    print("vgpr_count: %s" % sorted(set(k["vgpr_count"] for k in rows)))


def test_querycapsulecast_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for bad in (np.zeros((4, 8), np.float32), np.zeros(12, np.float32), np.zeros((2, 12, 1), np.float32), [[1, 2]]):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.queryCapsuleCast(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.queryCapsuleCast(state, np.zeros((2, 12), np.complex64))
    p0, p1, d = np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32), np.ones((2, 3), np.float32)
    with pytest.raises(pt.PathTracerError, match="need a radius"):
        pt.queryCapsuleCast(state, p0, p1, d)
    with pytest.raises(pt.PathTracerError, match="both p1 and directions"):
        pt.queryCapsuleCast(state, p0, p1, radius=1.0)
    with pytest.raises(pt.PathTracerError, match="both p1 and directions"):
        pt.queryCapsuleCast(state, p0, directions=d, radius=1.0)
    with pytest.raises(pt.PathTracerError, match="as many p1 and directions"):
        pt.queryCapsuleCast(state, p0, p1, np.ones((3, 3), np.float32), radius=1.0)
    with pytest.raises(pt.PathTracerError, match="as many p1 and directions"):
        pt.queryCapsuleCast(state, p0, np.ones((2, 4), np.float32), d, radius=1.0)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, 2.0, 3.0]):
        with pytest.raises(pt.PathTracerError, match="radius"):
            pt.queryCapsuleCast(state, p0, p1, d, radius=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(pt.PathTracerError, match="tmax"):
            pt.queryCapsuleCast(state, p0, p1, d, radius=1.0, tmax=bad)
    with pytest.raises(pt.PathTracerError, match="fourth column"):
        pt.queryCapsuleCast(state, np.zeros((2, 12), np.float32), radius=1.0)
    empty = pt.queryCapsuleCast(state, np.zeros((0, 12), np.float32))
    assert sorted(empty) == ["feature", "material", "point", "prim", "s", "t"]
    assert empty["t"].shape == (0,) and empty["point"].shape == (0, 3) and empty["prim"].dtype == np.uint32
    assert pt.queryCapsuleCast(state, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), radius=1.0, any_hit=True).shape == (0,)
    torch = pytest.importorskip("torch")
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.queryCapsuleCast(state, torch.zeros((4, 12), dtype=torch.float32))
    with pytest.raises(pt.PathTracerError, match="a tensor holds whole records"):
        pt.queryCapsuleCast(state, torch.zeros((4, 12), dtype=torch.float32), radius=1.0)


def test_capsule_contacts():
    casts = np.concatenate([_cast((1, 1, 5), (1, 1, 8), (0, 0, -1), 1.0), _cast((1, 1, 0.5), (1, 1, 3), (0, 0, -1), 1.0), _cast((9, 9, 5), (9, 9, 8), (0, 0, -1), 1.0),
                            _cast((2, -5, -1), (2, -5, 1), (0, 2, 0), 1.0), _cast((1, 1, -3), (1, 1, 5), (1, 0, 0), 0.5)])
    rec = cr.capsule_records(casts, TRI[0], TRI[1], np.zeros(1, np.uint32)).view(np.float32)
    result = {"t": rec[:, 0].copy(), "s": rec[:, 2].copy(), "point": rec[:, 4:7].copy()}
    q0, q1, on_axis, normal, start = pt.capsuleContacts(result, casts)
    assert np.array_equal(q0[0], [1, 1, 1]) and np.array_equal(q1[0], [1, 1, 4]) and np.array_equal(on_axis[0], [1, 1, 1]) and np.array_equal(normal[0], [0, 0, 1]) and not start[0]
    assert np.array_equal(q0[1], [1, 1, 0.5]) and np.array_equal(normal[1], [0, 0, 1]) and start[1]
    assert all(np.isnan(x[2]).all() for x in (q0, q1, on_axis, normal)) and not start[2]
    assert np.array_equal(q0[3], [2, -1, -1]) and np.array_equal(on_axis[3], [2, -1, 0]) and np.array_equal(normal[3], [0, -1, 0])     # the side, at s = 1 / 2
    assert start[4] and np.array_equal(on_axis[4], [1, 1, 0]) and np.array_equal(normal[4], [0, 0, 0])        # the axis through the triangle: no normal
    for x in (q0, q1, on_axis, normal):
        assert x.dtype == np.float32 and x.shape == (5, 3)
    with pytest.raises(pt.PathTracerError, match="expected the"):
        pt.capsuleContacts(result, casts[:, :8])
