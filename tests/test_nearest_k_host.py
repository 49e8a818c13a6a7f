"""pt_query_nearest_k / pt_query_within_any without a GPU: tests/nearest_k_ref.py's brute force on hand-checked lists, against
nearest_ref's one-record brute force, on the points that miss before any traversal, the radius rule, a scene without triangles; the
shares of the point sets the GPU tests rely on; the build lists, the ABI, the kernels' registers; the wrappers' argument checks."""
import os
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import nearest_ref as nr
import nearest_k_ref as kr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF
SCENE_FILES = ("cornell_box.obj", "cornell_box_diffuse.obj")


def _verts(rows):
    v = np.zeros((len(rows), 4), np.float32)
    v[:, :3] = rows
    return v.reshape(-1)


# two triangles in the plane z = 0 that share the edge (1,0,0)-(0,1,0); a third that shares only the vertex (0,0,0)
PAIR = (_verts([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]), np.array([0, 1, 2, 1, 3, 2], np.uint32), np.array([3, 5], np.uint32))
FAN = (_verts([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (-1, 0, 0), (0, -1, 0)]), np.array([0, 1, 2, 1, 3, 2, 0, 4, 5], np.uint32),
       np.array([3, 5, 0x07000002], np.uint32))


def _lists(points, scene, k=kr.MAX_K):
    return kr.nearest_k(np.asarray(points, np.float32).reshape(-1, 4), *scene, k=k)


def test_hand_checked_lists():
    # above the midpoint of the shared edge: both triangles at d2 = 4 exactly, the lower index first; k = 8 on two triangles: six misses
    rec, counts, hit = _lists([[0.5, 0.5, 2.0, np.inf]], PAIR)
    f = rec.view(np.float32)
    assert counts[0] == 2 and hit[0] == 1
    assert rec[0, 0, 1] == 0 and rec[0, 1, 1] == 1 and f[0, 0, 0] == 2.0 and f[0, 1, 0] == 2.0
    assert np.array_equal(f[0, 0, 4:7], [0.5, 0.5, 0.0]) and np.array_equal(f[0, 1, 4:7], [0.5, 0.5, 0.0])
    assert rec[0, 0, 7] == 3 and rec[0, 1, 7] == 5
    assert np.array_equal(rec[0, 2:], kr.miss_lists(1, 6)[0])
    # above the shared vertex (0, 0, 0) of the fan: triangles 0 and 2 tie at d2 = 9, triangle 1 is further (its closest point is the
    # edge's midpoint, d2 = 9.5); the material's top byte is masked off
    rec, counts, hit = _lists([[0.0, 0.0, 3.0, np.inf]], FAN, k=3)
    f = rec.view(np.float32)
    assert counts[0] == 3 and [int(x) for x in rec[0, :, 1]] == [0, 2, 1]
    assert f[0, 0, 0] == 3.0 and f[0, 1, 0] == 3.0 and f[0, 2, 0] == np.sqrt(F(9.5))
    assert rec[0, 1, 7] == 2 and np.array_equal(f[0, 2, 4:7], [0.5, 0.5, 0.0])
    # a radius that takes the two at the vertex and not the third; the count follows, the list's tail is the miss record
    rec, counts, hit = _lists([[0.0, 0.0, 3.0, 3.0]], FAN, k=3)
    assert counts[0] == 2 and [int(x) for x in rec[0, :, 1]] == [0, 2, MISS] and rec[0, 2, 0] == F(-1.0).view(np.uint32)
    # the count is not clamped to k, and a smaller k is the head of the larger list
    full = _lists([[0.0, 0.0, 3.0, np.inf]], FAN, k=8)
    one = _lists([[0.0, 0.0, 3.0, np.inf]], FAN, k=1)
    assert one[1][0] == 3 and np.array_equal(one[0], full[0][:, :1])
    # nothing within the radius: no list, count 0, byte 0
    rec, counts, hit = _lists([[0.0, 0.0, 3.0, 2.5]], FAN, k=2)
    assert counts[0] == 0 and hit[0] == 0 and np.array_equal(rec, kr.miss_lists(1, 2))


@pytest.fixture(scope="module")
def cornell():
    """scene -> (verts, idx, mats, name -> (points, radius)): computed once, shared, never written"""
    out = {}
    for scene in SCENE_FILES:
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
        verts, idx, mats = obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()
        sets = {}
        for name in nr.POINT_SETS:
            pts = nr.point_set(name, verts, idx, _camera())
            pts.setflags(write=False)
            sets[name] = (pts, kr.set_radius(name, verts, idx))
        out[scene] = (verts, idx, mats, sets)
    return out


def _camera():
    """The Cornell view of the GPU tests' contexts, as (eye, U, V, W)"""
    cam = pt.initCamera()
    cam.setAspectRatio(np.float32(97) / np.float32(61))
    return (cam.eye(),) + tuple(cam.UVWFrame())


@pytest.mark.parametrize("scene", SCENE_FILES)
def test_record_0_is_nearest_refs_record_and_the_list_is_sorted(cornell, scene):
    verts, idx, mats, sets = cornell[scene]
    for name, (pts, radius) in sets.items():
        for r in (np.inf, radius):
            points = nr.with_radius(pts, r)
            rec, counts, hit, d2 = kr.nearest_k(points, verts, idx, mats, return_d2=True)
            assert np.array_equal(rec[:, 0], nr.nearest_records(points, verts, idx, mats)), (name, float(r))
            assert np.array_equal(hit != 0, rec[:, 0, 1] != MISS) and np.array_equal(hit != 0, counts != 0)
            listed = (rec[:, :, 1] != MISS).sum(axis=1)
            assert np.array_equal(listed, np.minimum(counts, 8))
            # ascending (d2, prim), strictly: no triangle twice
            a, b = d2[:, :-1], d2[:, 1:]
            both = (rec[:, :-1, 1] != MISS) & (rec[:, 1:, 1] != MISS)
            assert ((a < b) | ((a == b) & (rec[:, :-1, 1] < rec[:, 1:, 1])))[both].all(), (name, float(r))
            # a miss is never followed by a find
            assert not ((rec[:, :-1, 1] == MISS) & (rec[:, 1:, 1] != MISS)).any()
            # the list is what a stable sort on d2 leaves in front: the candidates' d2, everything else +inf behind them
            full = kr.all_d2(points, verts, idx)
            stable = np.argsort(np.where(np.isnan(full), np.inf, full.astype(np.float64)), axis=1, kind="stable")[:, :8]
            is_cand = ~np.isnan(np.take_along_axis(full, stable, axis=1))
            assert np.array_equal(np.where(is_cand, stable, MISS).astype(np.uint32), rec[:, :, 1]), (name, float(r))
            # and for several radii at once it is the same reference
            if not np.isinf(r):
                both_r = kr.nearest_k_radii(pts, (np.inf, r), verts, idx, mats)
                assert all(np.array_equal(a, b) for a, b in zip(both_r[1], (rec, counts, hit)))
            if np.isinf(r):
                assert (counts == len(idx) // 3).all()           # no NaN d2 on the fixtures: every triangle counts


def test_points_that_miss_before_any_traversal_the_radius_rule_and_no_triangles():
    good = np.array([0.25, 0.25, 1.0, np.inf], np.float32)
    bad, why = nr.bad_points(good)
    rec, counts, hit = _lists(bad, FAN)
    assert np.array_equal(rec, kr.miss_lists(len(bad), 8)) and not counts.any() and not hit.any(), why
    # the radius rule: d2 <= r * r in fp32, closed.  The point is at distance 1 of the plane: d2 = 1
    for r, n_found in ((1.0, 2), (np.nextafter(F(1.0), F(0.0)), 0), (0.0, 0), (-0.0, 0), (1e30, 3), (np.inf, 3)):
        rec, counts, hit = _lists([[0.25, 0.25, 1.0, r]], FAN)
        d2 = kr.all_d2(np.array([[0.25, 0.25, 1.0, np.inf]], np.float32), FAN[0], FAN[1])[0]
        with np.errstate(over="ignore"):
            want = int((d2 <= F(r) * F(r)).sum())
        assert counts[0] == want and (n_found == 0) == (want == 0) and hit[0] == (want != 0), (r, counts, d2)
    # on the surface with radius +-0: d2 = 0 is a candidate
    rec, counts, hit = _lists([[0.25, 0.25, 0.0, 0.0], [0.25, 0.25, 0.0, -0.0]], FAN)
    assert (counts == 1).all() and (rec[:, 0, 1] == 0).all() and (rec[:, 0, 0] == 0).all()
    # a zero-area triangle whose d2 is a NaN is neither listed nor counted
    degenerate = (_verts([(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 2, 2)]), np.array([3, 3, 3, 0, 1, 2], np.uint32), np.array([1, 2], np.uint32))
    d2 = kr.all_d2(np.array([[0.25, 0.25, 1.0, np.inf]], np.float32), degenerate[0], degenerate[1])[0]
    rec, counts, hit = _lists([[0.25, 0.25, 1.0, np.inf]], degenerate)
    assert counts[0] == int((~np.isnan(d2)).sum()) and rec[0, 0, 1] == 1
    # a scene without triangles
    none = (_verts([(0, 0, 0)]), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    rec, counts, hit = _lists([[0.0, 0.0, 0.0, np.inf]] * 3, none, k=4)
    assert np.array_equal(rec, kr.miss_lists(3, 4)) and not counts.any() and not hit.any()


@pytest.mark.parametrize("scene", SCENE_FILES)
def test_the_sets_split_into_none_few_and_many(cornell, scene):
    """The condition the GPU tests rely on, by the brute force alone: at its radius every set has points with no candidate, with 1 to
    7 (trailing misses in a list of 8) and, but for wall_planes and surface, with more than 8 (the list overflows and the cut bites),
    each class at least a tenth; and at +inf the last kept and the first dropped entry of a list of 8 tie exactly on at least a tenth of
    inside, shell, features and wall_planes, which is what makes the tie rule at the cut bite."""
    verts, idx, mats, sets = cornell[scene]
    for name, (pts, radius) in sets.items():
        counts = kr.nearest_k(nr.with_radius(pts, radius), verts, idx, mats)[1]
        none, few, eight, many = kr.classes(counts)
        print("%s %s (radius %g): none %.3f, 1 to 7 %.3f, exactly 8 %.3f, more than 8 %.3f" % (scene, name, float(radius), none, few, eight, many))
        if name == "surface":
            assert none > 0 and none < 1, (name, none)
            continue
        assert none >= 0.1 and few >= 0.1, (name, none, few)
        if name != "wall_planes":
            assert many >= 0.1, (name, many)
    for name in ("inside", "shell", "features", "wall_planes"):
        tie = kr.tie_at_the_cut(nr.with_radius(sets[name][0], np.inf), verts, idx)
        print("%s %s: entries 7 and 8 tie exactly on %.3f" % (scene, name, tie))
        assert tie >= 0.1, (name, tie)


# ---- the layers ---------------------------------------------------------------------------------------------------------------------
def test_build_lists_and_abi():
    assert "nearest_k.hip" in _build.HIP_SOURCES and "nearest_k.h" in _build.HIP_HEADERS
    for name in ("nearest_k.hip", "nearest_k.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert "pt_query_nearest_k" in _native.ABI_SYMBOLS and "pt_query_within_any" in _native.ABI_SYMBOLS
    assert "pt_debug_nearest_k_visits" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4 and _native.QUERY_NEAREST_MAX == kr.MAX_K == 8
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert "#define PT_QUERY_NEAREST_MAX 8" in hdr
    assert "int pt_query_nearest_k(pt_ctx* ctx, const float* points, size_t n, uint32_t max_k, pt_nearest* out, uint32_t* counts);" in hdr
    assert "int pt_query_within_any(pt_ctx* ctx, const float* points, size_t n, uint8_t* hit);" in hdr


def test_nearest_k_kernels_use_no_scratch_memory_and_spill_nothing(built):
    """Every instantiation — two node formats, the list of 1, 2, 4 and 8 with and without counts and the count-only form, the
    within-radius kernel, each with its counting twin: no private segment, no spilled vector or scalar register"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    table = kernel_meta.kernel_table(_native.hip_library_path())
    lists = [k for k in table if "k_query_nearest_k<" in k["name"]]
    within = [k for k in table if "k_query_within_any<" in k["name"]]
    assert len(lists) == 2 * 9 * 2 and len(within) == 2 * 2, ([k["name"] for k in lists], [k["name"] for k in within])
    for k in lists + within:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


def test_querynearestk_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros((2, 4, 1), np.float32), [[1, 2]]):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.queryNearestK(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.queryNearestK(state, np.zeros((2, 3), np.complex64))
    for bad in (-1.0, float("nan")):
        with pytest.raises(pt.PathTracerError, match="radius"):
            pt.queryNearestK(state, np.zeros((2, 3), np.float32), max_radius=bad)
    for bad in (-1, 9, 2.5, "many", None):
        with pytest.raises(pt.PathTracerError, match="k "):
            pt.queryNearestK(state, np.zeros((2, 3), np.float32), k=bad)
    with pytest.raises(pt.PathTracerError, match="counts"):
        pt.queryNearestK(state, np.zeros((2, 3), np.float32), k=0)
    empty = pt.queryNearestK(state, np.zeros((0, 3), np.float32), k=3, counts=True)
    assert sorted(empty) == ["count", "distance", "material", "point", "prim", "u", "v"]
    assert empty["distance"].shape == (0, 3) and empty["point"].shape == (0, 3, 3) and empty["prim"].dtype == np.uint32 and empty["count"].shape == (0,)
    assert "count" not in pt.queryNearestK(state, np.zeros((0, 4), np.float32))
    assert pt.queryNearestK(state, np.zeros((0, 4), np.float32))["distance"].shape == (0, 4)


def test_querywithinany_argument_checks_need_no_device():
    state = pt.PathTracerState()
    for bad in (np.zeros((4, 5), np.float32), np.zeros(4, np.float32), [[1, 2]]):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.queryWithinAny(state, bad, 1.0)
    with pytest.raises(pt.PathTracerError, match="need a radius"):
        pt.queryWithinAny(state, np.zeros((2, 3), np.float32))
    with pytest.raises(pt.PathTracerError, match="fourth column"):
        pt.queryWithinAny(state, np.zeros((2, 4), np.float32), 1.0)
    for bad in (-1.0, float("nan"), "wide"):
        with pytest.raises(pt.PathTracerError, match="radius"):
            pt.queryWithinAny(state, np.zeros((2, 3), np.float32), bad)
    got = pt.queryWithinAny(state, np.zeros((0, 3), np.float32), 1.0)
    assert got.shape == (0,) and got.dtype == bool
    assert pt.queryWithinAny(state, np.zeros((0, 4), np.float32)).shape == (0,)


def test_spherecontacts_argument_checks_need_no_device():
    state = pt.PathTracerState()
    ok = np.zeros((2, 3), np.float32)
    for bad in (np.zeros((2, 4)), np.zeros(3), np.zeros((2, 3, 1))):
        with pytest.raises(pt.PathTracerError, match="\\(n, 3\\) centres"):
            pt.sphereContacts(state, bad, 1.0)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.sphereContacts(state, ok.astype(np.complex64), 1.0)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, -2.0], [1.0, 2.0, 3.0], "wide"):
        with pytest.raises(pt.PathTracerError, match="radius"):
            pt.sphereContacts(state, ok, bad)
    for bad in (0, 9, 2.5, "all"):
        with pytest.raises(pt.PathTracerError, match="max_contacts"):
            pt.sphereContacts(state, ok, 1.0, max_contacts=bad)
    empty = pt.sphereContacts(state, np.zeros((0, 3)), 0.5, max_contacts=3)
    assert sorted(empty) == ["count", "material", "normal", "penetration", "point", "prim"]
    assert empty["point"].shape == (0, 3, 3) and empty["normal"].shape == (0, 3, 3) and empty["penetration"].shape == (0, 3) and empty["penetration"].dtype == np.float32
