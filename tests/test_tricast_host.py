"""The translating-triangle cast's statement on the host (tests/tricast_ref.py, include/acgpt.h pt_query_triangle_cast): hand-checked
cases for each of the 16 features, the tie, override and tmax rules, the float64 statement against an independent formulation (the
float64 triangle-to-triangle distance of the translated triangle), fp32 against float64 on the Cornell sets, the documented blind spot
(in-plane sliding) and the guards' promise on near-parallel casts, the posed reduction, the build lists and the wrappers' argument
checks.  No device."""
import os
import re

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import nearest_ref as nr
import poses_ref as pr
import tricast_ref as tc
import tridist_ref as tr

F = np.float32
BOX = os.path.join(pt.SCENES, "cornell_box.obj")

# The float64 distance between the query translated by the fp32 t and the winning scene triangle, over the hits of "aimed" and "links"
# on the Cornell box: measured 7.5e-5 units (test_fp32_against_float64_on_the_cornell_sets prints it).  Held at four times that
# (DESIGN.md section 24's convention); the GPU tests hold pt_query_triangle_distance at the moved triangle to it.
CONTACT_MEASURED = 7.5e-5
CONTACT_BOUND = 4 * CONTACT_MEASURED
CALLED_DIFFERENTLY_MAX = 0.01           # share of casts that fp32 and float64 may call differently (hit against miss)

# the scene triangle of the hand-checked cases, in the plane z = 0, and the motion straight down
V0, V1, V2 = np.array([0.0, 0.0, 0.0]), np.array([4.0, 0.0, 0.0]), np.array([0.0, 4.0, 0.0])
DOWN = np.array([0.0, 0.0, -1.0])


def _pair(a, d, v, dtype=np.float32):
    a, v = np.asarray(a, dtype)[:, None, :], np.asarray(v, dtype)[:, None, :]
    t, f, c = tc.cast_pair(a[0], a[1], a[2], np.asarray(d, dtype)[None], v[0], v[1] - v[0], v[2] - v[0])
    return float(t[0]), int(f[0]), c[0].astype(np.float64)


@pytest.fixture(scope="module")
def box():
    obj = pt.TinyObjWrapper(BOX)
    return obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()


@pytest.fixture(scope="module")
def sets(box):
    """set -> (casts, fp32 records) on the Cornell box: computed once, shared, never written"""
    cache = {}

    def get(name):
        if name not in cache:
            s = tc.cast_set(name, *box)
            rec = tc.cast_records(s, *box)
            s.setflags(write=False); rec.setflags(write=False)
            cache[name] = (s, rec)
        return cache[name]
    return get


# ---- 1. each feature answers, exactly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_corner_of_the_query_meets_the_scene_triangle(dtype):
    """the lowest corner (1, 1, 2) comes down on the triangle's inside at t = 2; the other two follow at t = 3"""
    low, b, c = [1.0, 1.0, 2.0], [2.0, 1.0, 3.0], [1.0, 2.0, 3.0]
    for k, a in enumerate(([low, b, c], [b, low, c], [b, c, low])):
        assert _pair(a, DOWN, (V0, V1, V2), dtype)[:2] == (2.0, k)
        assert np.array_equal(_pair(a, DOWN, (V0, V1, V2), dtype)[2], [1.0, 1.0, 0.0])
        # d is not normalised: t is in units of |d|
        assert _pair(a, 4 * DOWN, (V0, V1, V2), dtype)[:2] == (0.5, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_corner_of_the_scene_triangle_meets_the_query(dtype):
    """the scene triangle's apex (0, 0, 1) stands 1 above its other corners; a wide level triangle at z = 3 comes down on it at t = 2"""
    apex, b, c = np.array([0.0, 0.0, 1.0]), V1, V2
    a = [[-8.0, -8.0, 3.0], [8.0, -8.0, 3.0], [0.0, 8.0, 3.0]]
    for k, v in enumerate(([apex, b, c], [c, apex, b], [b, c, apex])):
        t, f, at = _pair(a, DOWN, v, dtype)
        assert (t, f) == (2.0, 3 + k) and np.array_equal(at, apex)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("j", [0, 1, 2])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_an_edge_of_the_query_meets_an_edge_of_the_scene_triangle(i, j, dtype):
    """A query edge from a low point 1 outside scene edge j to a high point 1 inside it crosses the edge's midpoint at height 2: the
    edges meet there at t = 2.  The low end comes down outside the triangle at t = 1, the high end on its inside at t = 3."""
    mid, out, along = (([2.0, 0.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]), ([0.0, 2.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]),
                       ([2.0, 2.0, 0.0], [0.5, 0.5, 0.0], [-1.0, 1.0, 0.0]))[j]
    mid, out, along = np.array(mid), np.array(out), np.array(along)
    low, high, third = mid + out + [0.0, 0.0, 1.0], mid - out + [0.0, 0.0, 3.0], mid - 0.5 * out + 0.25 * along + [0.0, 0.0, 9.0]
    a = ([low, high, third], [low, third, high], [third, low, high])[i]
    t, f, at = _pair(a, DOWN, (V0, V1, V2), dtype)
    assert (t, f) == (2.0, 6 + 3 * i + j) and np.array_equal(at, mid)


def test_a_start_overlap_overrides_and_answers_zero():
    a = [[1.0, 1.0, -1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 1.0]]                   # stands through the plane
    for d in (DOWN, -DOWN, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]):
        t, f, at = _pair(a, d, (V0, V1, V2))
        assert (t, f) == (0.0, tc.START) and not at.any() and not np.signbit(t)
    # touching counts: the corner rests on the triangle
    assert _pair([[1.0, 1.0, 0.0], [2.0, 1.0, 1.0], [1.0, 2.0, 1.0]], -DOWN, (V0, V1, V2))[:2] == (0.0, tc.START)


def test_every_feature_wins_somewhere_in_the_sets(sets):
    """By the brute force alone: a set that lost its purpose must not pass vacuously."""
    seen = np.zeros(16, np.int64)
    for name in tc.CAST_SETS:
        s, rec = sets(name)
        assert s.shape == (tc.SET_SIZE, 16) and s.dtype == np.float32
        col = tc.columns(rec)
        hit = col["t"] >= 0
        per = np.bincount(col["feature"][hit].astype(np.int64), minlength=16)
        seen += per
        print("%-10s hit %.3f, start overlaps %.3f, features %s" % (name, hit.mean(), (col["feature"][hit] == 15).mean() if hit.any() else 0.0, per.tolist()))
        assert hit.mean() >= 0.2 and np.unique(col["prim"][hit]).size >= 8, name
        if name in ("short", "outside", "zero_d", "bad"):
            assert (~hit).mean() >= 0.2, name
        if name == "zero_d":
            assert (col["feature"][hit] == 15).all() and (col["t"][hit] == 0).all()
        if name == "overlap":
            assert (col["feature"][hit] == 15).mean() >= 0.9
        if name == "degenerate":
            assert per[:15].sum() >= 300                      # segments and points still travel and touch
        if name == "bad":
            bad = ~tc.castable(s)
            assert 0.3 <= bad.mean() <= 0.34 and np.array_equal(rec[bad], tc.miss_records(int(bad.sum())))
            assert (rec[~bad] == sets("aimed")[1][~bad]).all()
    assert (seen > 0).all(), seen


# ---- 2. ties, the override, tmax, -0 -------------------------------------------------------------------------------------------------
def _scene(tris, mats=None):
    """(verts float32 flat float4, idx, mat_ids) of a list of (3, 3) triangles"""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    verts = np.zeros((t.shape[0] * 3, 4), np.float32)
    verts[:, :3] = t.reshape(-1, 3)
    return verts.reshape(-1), np.arange(t.shape[0] * 3, dtype=np.uint32), np.asarray(mats if mats is not None else np.arange(t.shape[0]), np.uint32)


def test_ties_go_to_the_lower_feature_and_the_lower_index():
    level = [[1.0, 1.0, 2.0], [2.0, 1.0, 2.0], [1.0, 2.0, 2.0]]                # all three corners land at t = 2
    assert _pair(level, DOWN, (V0, V1, V2))[:2] == (2.0, 0)
    assert _pair(level[::-1], DOWN, (V0, V1, V2))[:2] == (2.0, 0)
    tri = [V0, V1, V2]
    lower = [V0 - [0, 0, 1], V1 - [0, 0, 1], V2 - [0, 0, 1]]
    cast = tc.pack([level], [DOWN], np.inf)
    for order, want in (([lower, tri, tri], 1), ([tri, lower, tri], 0), ([lower, lower, tri], 2)):
        rec = tc.columns(tc.cast_records(cast, *_scene(order, [5, 6, 7])))
        assert rec["t"][0] == 2.0 and rec["prim"][0] == want and rec["material"][0] == 5 + want and rec["query_triangle"][0] == 0


def test_tmax_is_closed_and_a_miss_is_the_miss_record():
    level = [[1.0, 1.0, 2.0], [2.0, 1.0, 2.0], [1.0, 2.0, 2.0]]
    scene = _scene([[V0, V1, V2]])
    below = np.nextafter(F(2.0), F(0.0))
    casts = tc.pack([level] * 5, [DOWN] * 5, [np.inf, 2.0, below, 0.0, 3.4e38])
    rec = tc.cast_records(casts, *scene)
    assert (tc.columns(rec)["t"] == np.array([2.0, 2.0, -1.0, -1.0, 2.0], np.float32)).all()
    assert np.array_equal(rec[2], tc.miss_records(1)[0]) and list(tc.miss_records(1)[0]) == [0xBF800000, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0xFFFFFFFF]
    assert list(tc.blocked_of(rec)) == [1, 1, 0, 0, 1]
    # a start overlap answers under tmax = 0; moving away from the triangle never touches it
    through = [[1.0, 1.0, -1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 1.0]]
    assert tc.columns(tc.cast_records(tc.pack([through], [DOWN], 0.0), *scene))["feature"][0] == 15
    assert tc.cast_records(tc.pack([level], [-DOWN], np.inf), *scene)[0, 1] == 0xFFFFFFFF
    # a scene without triangles, and no casts
    assert np.array_equal(tc.cast_records(casts, np.zeros(0, np.float32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)), tc.miss_records(5))
    assert tc.cast_records(casts[:0], *scene).shape == (0, 8)


def test_a_negative_zero_becomes_zero():
    """With det < 0 the four numbers change sign: a T of +0 becomes -0, and t = T / det + 0 is +0 again"""
    o = np.array([1.0, 1.0, 0.0], np.float32)
    for k1, k2 in ((V1 - V0, V2 - V0), (V2 - V0, V1 - V0)):
        acc, t = tc._ray(o, np.asarray(DOWN, np.float32), V0.astype(np.float32), k1.astype(np.float32), k2.astype(np.float32))
        assert acc and t == 0 and not np.signbit(t)
    neg = np.float32(-0.0) / np.float32(8.0)
    assert np.signbit(neg) and not np.signbit(neg + np.float32(0))


def test_every_bad_cast_is_a_miss_before_any_traversal(sets):
    s, rec = sets("aimed")
    good = s[int(np.flatnonzero(rec[:, 1] != 0xFFFFFFFF)[0])]
    bad, why = tc.bad_casts(good)
    assert len(why) == 36 + 4 + 9 and not tc.castable(bad).any() and tc.castable(good[None]).all()
    scene = _scene([[V0, V1, V2]])
    assert np.array_equal(tc.cast_records(bad, *scene), tc.miss_records(bad.shape[0]))
    ok = good.copy(); ok[[7, 11, 15]] = np.nan                 # the dotted floats are never read into a decision
    assert tc.castable(ok[None]).all()


# ---- 3. the float64 statement against an independent formulation ---------------------------------------------------------------------
def _random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, (n, 3, 3)).astype(np.float32)
    u = rng.normal(size=(n, 3)); u /= np.sqrt((u * u).sum(axis=1, keepdims=True))
    a = (rng.uniform(-0.7, 0.7, (n, 3, 3)) - 3.0 * u[:, None, :] + rng.uniform(-0.6, 0.6, (n, 1, 3))).astype(np.float32)
    d = (u * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    return a, d, v


def test_the_float64_statement_against_the_distance_of_the_translated_triangle():
    """On 2 000 random pairs: where the statement finds t, the float64 triangle-to-triangle distance of the translated triangle is 0 at t
    and positive just before it — the distance is convex along the motion, so nothing touches before a positive value —; where it
    finds none, a ternary search of that convex distance finds no contact either."""
    a, d, v = _random_pairs(2000, 4101)
    a64, d64, v64 = a.astype(np.float64), d.astype(np.float64), v.astype(np.float64)
    t, f, c = tc.cast_pair(a64[:, 0], a64[:, 1], a64[:, 2], d64, v64[:, 0], v64[:, 1] - v64[:, 0], v64[:, 2] - v64[:, 0])

    def dist(at):
        m = a64 + (d64 * at[:, None])[:, None, :]
        return tr.distance_f64(m[:, 0], m[:, 1], m[:, 2], v64[:, 0], v64[:, 1] - v64[:, 0], v64[:, 2] - v64[:, 0])
    hit = np.isfinite(t)
    assert 0.3 <= hit.mean() <= 0.8 and (f[hit] != tc.START).mean() >= 0.9
    at = np.where(hit, t, 0.0)
    touching = dist(at)[hit]
    print("float64: %d hits of %d, the distance at t is at most %.2e" % (hit.sum(), hit.size, touching.max()))
    assert touching.max() <= 1e-12
    moving = hit & (t > 0)
    before = dist(np.maximum(at - 1e-6 * (1.0 + at), 0.0))
    assert (before[moving] > 1e-9).all(), before[moving].min()
    # the misses: the convex distance over [0, far] has no zero
    far = np.full(t.shape, 12.0)                               # |d| >= 0.5 and nothing is further than 6 apart
    lo_t, hi_t = np.zeros_like(far), far
    for _ in range(100):
        m1, m2 = lo_t + (hi_t - lo_t) / 3.0, hi_t - (hi_t - lo_t) / 3.0
        left = dist(m1) <= dist(m2)
        lo_t, hi_t = np.where(left, lo_t, m1), np.where(left, m2, hi_t)
    closest = dist(0.5 * (lo_t + hi_t))
    assert (closest[~hit] > 1e-9).all(), closest[~hit].min()
    assert (closest[hit] <= 1e-9).all()
    # the contact lies on both triangles at t
    cm = c[moving]
    on_scene = nr.closest_f64(cm, v64[moving, 0], v64[moving, 1], v64[moving, 2])[0]
    m = a64[moving] + (d64[moving] * t[moving, None])[:, None, :]
    on_query = nr.closest_f64(cm, m[:, 0], m[:, 1], m[:, 2])[0]
    assert on_scene.max() <= 1e-12 and on_query.max() <= 1e-12


# ---- 4. fp32 against float64 ---------------------------------------------------------------------------------------------------------
def test_fp32_against_float64_on_the_cornell_sets(box, sets):
    """The query translated by the fp32 t touches the winning triangle within CONTACT_BOUND in float64, and the two precisions call
    at most 1 % of the casts differently."""
    v0, e1, e2 = nr.records_of_scene(box[0], box[1])
    worst = 0.0
    for name in ("aimed", "links"):
        s, rec = sets(name)
        col = tc.columns(rec)
        rec64 = tc.columns(tc.cast_records(s, *box, dtype=np.float64))
        hit, hit64 = col["t"] >= 0, rec64["t"] >= 0
        differently = float((hit != hit64).mean())
        m = tc.moved(s[hit], col["t"][hit])
        p = col["prim"][hit]
        dist = tr.distance_f64(m[:, 0], m[:, 1], m[:, 2], v0[p], e1[p], e2[p])
        both = hit & hit64
        dt = np.abs(col["t"][both].astype(np.float64) - rec64["t"][both]) * np.sqrt((s[both, 12:15].astype(np.float64) ** 2).sum(axis=1))
        print("%-6s fp32 hits %d, float64 hits %d, called differently %.4f, distance at the fp32 t at most %.3e, |d| |t - t64| at most %.3e"
              % (name, hit.sum(), hit64.sum(), differently, dist.max(), dt.max()))
        assert differently <= CALLED_DIFFERENTLY_MAX, (name, differently)
        worst = max(worst, float(dist.max()))
    assert worst <= CONTACT_BOUND, worst
    assert worst >= CONTACT_MEASURED / 4, "the measured figure in this file and in DESIGN.md section 37 is stale: %g" % worst


# ---- 5. documented behaviour ---------------------------------------------------------------------------------------------------------
def test_a_slide_within_the_plane_is_seen_only_as_a_start_overlap():
    """Two coplanar triangles: every det is 0, so the one that slides into the other from outside is not stopped; the same motion from
    a start overlap answers 0."""
    outside = [[6.0, 1.0, 0.0], [7.0, 1.0, 0.0], [6.0, 2.0, 0.0]]
    along = [-1.0, 0.0, 0.0]
    for dtype in (np.float32, np.float64):
        t, f, _ = _pair(outside, along, (V0, V1, V2), dtype)
        assert t == np.inf and f == tc.NONE
        t, f, _ = _pair(np.asarray(outside) - [4.0, 0.0, 0.0], along, (V0, V1, V2), dtype)
        assert (t, f) == (0.0, tc.START)
    # lifted off the plane by any amount and moving down into it, it is stopped
    t, f, _ = _pair(np.asarray(outside) + [-4.0, 0.0, 0.5], [-1.0, 0.0, -1.0], (V0, V1, V2))
    assert t == 0.5 and f == 0


def test_near_parallel_casts_keep_the_guards_promise(box):
    """Triangles within 1e-7 of a wall's plane, moving almost within it: det is near-singular and t is noise, but every accepted
    contact is tied to both boxes — the float64 boxes of the translated query and of the winning triangle lie within 2 eps of each
    other on every axis (one eps per guard, eps = 2^-16 (S + mQ))."""
    verts, idx, mats = box
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    lo, hi = nr.scene_box(verts, idx)
    rng = np.random.default_rng(4303)
    n = 1000
    pick = rng.integers(0, v0.shape[0], n)
    p0, a, b = v0[pick].astype(np.float64), e1[pick].astype(np.float64), e2[pick].astype(np.float64)
    nrm = np.cross(a, b); nrm /= np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
    uw = rng.uniform(-1.5, 2.5, (n, 3, 2))
    q = p0[:, None] + uw[:, :, 0:1] * a[:, None] + uw[:, :, 1:2] * b[:, None] + (nrm * rng.uniform(1e-8, 1e-7, (n, 1)))[:, None, :]
    k = rng.uniform(-1.0, 1.0, (n, 2))
    d = k[:, 0:1] * a + k[:, 1:2] * b - nrm * rng.uniform(0.0, 1e-6, (n, 1))
    s = tc.pack(q, d, np.inf)
    col = tc.columns(tc.cast_records(s, verts, idx, mats))
    hit = (col["t"] >= 0) & (col["feature"] != 15)
    assert hit.sum() >= 50
    m = tc.moved(s[hit], col["t"][hit])
    p = col["prim"][hit]
    tri = np.stack([v0[p], v0[p] + e1[p], v0[p] + e2[p]], axis=1).astype(np.float64)
    gap = np.maximum(m.min(axis=1) - tri.max(axis=1), tri.min(axis=1) - m.max(axis=1)).max(axis=1)
    eps = 2.0 ** -16 * (np.abs(tri).max(axis=(1, 2)) + np.abs(tc.moved(s[hit], np.zeros(int(hit.sum())))).max(axis=(1, 2)))
    print("near-parallel: %d moving contacts, the boxes' largest gap is %.3e (2 eps = %.3e)" % (hit.sum(), gap.max(), 2 * eps.min()))
    assert (gap <= 2 * eps + 1e-4).all()                        # 1e-4: d t and the sums round in fp32 at a scale of 1e3


# ---- the posed reduction -------------------------------------------------------------------------------------------------------------
def test_the_posed_reduction_takes_the_smallest_t_and_the_lowest_triangle(box):
    v, f = tc.icosphere(0, 30.0)
    mesh = pr.records_of(v, f)
    poses = pr.as_poses(pr._translations([[150.0, 200.0, 300.0], [150.0, 60.0, 300.0], [1500.0, 0.0, 0.0], [np.nan, 0.0, 0.0]]))
    motions = np.array([[0.0, -1.0, 0.0, np.inf], [0.0, -1.0, 0.0, 10.0], [1.0, 0.0, 0.0, np.inf], [0.0, -1.0, 0.0, np.inf]], np.float32)
    casts = tc.posed_casts(poses, motions, mesh)
    assert casts.shape == (4 * 20, 16) and (casts[20:40, 3] == 10.0).all() and (casts[0:20, 13] == -1.0).all()
    per = tc.cast_records(casts, *box)
    rec = tc.reduce_casts(per, 4)
    col = tc.columns(rec)
    assert col["t"][0] > 0 and col["t"][1] == -1 and col["t"][2] == -1 and col["t"][3] == -1
    assert np.array_equal(rec[1], tc.miss_records(1, tc.MISS)[0]) and rec[1, 3] == 0xFFFFFFFF
    k = int(col["query_triangle"][0])
    t_all = tc.columns(per[0:20])["t"]
    assert t_all[k] == col["t"][0] and (t_all[t_all >= 0] >= col["t"][0]).all() and not (t_all[:k] == col["t"][0]).any()
    assert np.array_equal(rec[0, [0, 1, 2, 4, 5, 6, 7]], per[k, [0, 1, 2, 4, 5, 6, 7]])
    assert np.array_equal(tc.poses_cast(poses, motions, mesh, *box), rec)
    # a tie between two mesh triangles goes to the lower one
    two = np.concatenate([mesh[3:4], mesh[3:4], mesh[0:3]])
    tie = tc.poses_cast(poses[:1], motions[:1], two, *box)
    assert tie[0, 3] == 0 and tie[0, 0] == tc.cast_records(tc.posed_casts(poses[:1], motions[:1], mesh[3:4]), *box)[0, 0]


# ---- 6. the build lists, the dtype, the argument checks ----------------------------------------------------------------------------------
def test_build_lists_and_abi():
    assert "tricast.hip" in _build.HIP_SOURCES and {"tricast.h", "tricast_device.h", "tritri_device.h", "bvh_walk.h", "query_launch.h", "poses.h"} <= set(_build.HIP_HEADERS)
    for name in ("tricast.hip", "tricast.h", "tricast_device.h", "bvh_walk.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES             # pt_kernel_source_hash() does not move
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    for name in ("pt_query_triangle_cast", "pt_query_triangle_cast_any", "pt_query_poses_cast"):
        assert name in _native.ABI_SYMBOLS
    assert "pt_debug_triangle_cast_visits" in _native.TEST_SYMBOLS and "pt_debug_query_poses_cast" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4
    header = open(os.path.join(_build.ROOT, "include", "acgpt.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert "int pt_query_triangle_cast(pt_ctx* ctx, const float* casts, size_t n, pt_triangle_cast_hit* hits);" in flat
    assert "int pt_query_triangle_cast_any(pt_ctx* ctx, const float* casts, size_t n, uint8_t* blocked);" in flat
    assert "int pt_query_poses_cast(pt_ctx* ctx, const float* poses, const float* motions, size_t P, pt_triangle_cast_hit* out);" in flat
    assert "float t; uint32_t prim; float feature; uint32_t query_triangle; float cx, cy, cz; uint32_t material; } pt_triangle_cast_hit;" in flat
    assert pt.TRIANGLE_CAST_DTYPE.itemsize == 32 and pt.TRIANGLE_CAST_DTYPE.names == ("t", "prim", "feature", "query_triangle", "point", "material")
    assert [pt.TRIANGLE_CAST_DTYPE.fields[k][1] for k in pt.TRIANGLE_CAST_DTYPE.names] == [0, 4, 8, 12, 16, 28]


def test_the_kernels_use_no_scratch_and_spill_nothing():
    import sys
    sys.path.insert(0, os.path.join(_build.ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if "cast" in k["name"] and "ptd::k_" in k["name"]]
    names = sorted(set(re.sub(r"<.*", "", k["name"].replace("void ptd::", "")) for k in rows))
    assert names == ["k_cast_pose", "k_cast_pose_record", "k_query_triangle_cast", "k_query_triangle_cast_any"] and len(rows) == 10
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] <= 168, k                      # three waves per SIMD (512 / 168); DESIGN.md section 37 quotes the figures


def test_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for bad in (np.zeros((4, 8), np.float32), np.zeros((4, 3, 4), np.float32), np.zeros(16, np.float32)):
        with pytest.raises(pt.PathTracerError, match="expected"):
            pt.queryTriangleCast(state, bad)
    with pytest.raises(pt.PathTracerError, match="expected"):
        pt.queryTriangleCast(state, np.zeros((4, 16), np.float32), np.zeros((4, 3)))
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.queryTriangleCast(state, np.zeros((2, 16), object))
    with pytest.raises(pt.PathTracerError, match="direction"):
        pt.queryTriangleCast(state, np.zeros((2, 9), np.float32), np.zeros((3, 3)))
    for bad in (-1.0, float("nan"), [1.0, 2.0, 3.0]):
        with pytest.raises(pt.PathTracerError, match="tmax"):
            pt.queryTriangleCast(state, np.zeros((2, 9), np.float32), np.zeros(3), tmax=bad)
    assert pt.queryTriangleCast(state, np.zeros((0, 16), np.float32))["t"].shape == (0,)
    assert pt.queryTriangleCast(state, np.zeros((0, 16), np.float32), any_hit=True).shape == (0,)
    with pytest.raises(pt.PathTracerError, match="motions"):
        pt.queryPosesCast(state, np.zeros((2, 3, 4), np.float32), np.zeros((3, 4), np.float32))
    with pytest.raises(pt.PathTracerError, match="poses"):
        pt.queryPosesCast(state, np.zeros((2, 5), np.float32), np.zeros((2, 4), np.float32))
    with pytest.raises(pt.PathTracerError, match="at least two"):
        pt.advanceUntilContact(state, np.zeros((1, 3, 4), np.float32))
    with pytest.raises(pt.PathTracerError, match="expected"):
        pt.castContacts({"t": np.zeros(2, np.float32), "feature": np.zeros(2, np.float32), "prim": np.zeros(2, np.uint32)}, np.zeros((2, 8), np.float32),
                        np.zeros((3, 3), np.float32), [0, 1, 2])
