"""pt_query_multi without a GPU: the reference of tests/multihit_ref.py on hand-checked cases and against the oracle's closest and any
hit on whole scenes, the conditions that make the ray sets of tests/query_scenes.py worth shooting at the multi-hit walk, the
declarations, and the argument checks of queryRaysMulti and pointsInside.

Conditions (held here by the reference alone, measured on the CPU with the oracle; the sets are query_scenes.ray_sets(name) as they
stand):
  pooled over a scene's sets    at least a tenth of the rays with no hit, a tenth with exactly one, a tenth with two or more
                                (box 45 % / 32 % / 23 %, sphere 48 % / 38 % / 15 %)
  "aimed" on box, sphere, flat  at least half the rays with two or more hits (73 %, 76 %, 71 %), a tenth with more than two
                                (57 %, 40 %, 49 %); on the box a tenth with more than four (21 %)
  copies                        every ray that hits has all 20 000 triangles at one t
  copies_lifted, "aimed"        at least a quarter of the 257 rays with more than 8 hits (64 %)"""
import os
import re

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import multihit_ref as mr
import query_ref as qr
import query_scenes as qs

F = np.float32
MISS = mr.MISS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ray(o, d, tmin=0.0, tmax=np.inf):
    return np.array([list(o) + list(d) + [tmin, tmax]], np.float32)


def _stack():
    """Three parallel triangles over the origin at z = 3, 1, 2 in index order (the order of the hits is not the order of the indices),
    each with its own vertices and material"""
    tri = np.array([[-10, -10, 0, 0], [30, -10, 0, 0], [-10, 30, 0, 0]], np.float32)
    v = np.concatenate([tri + np.array([0, 0, z, 0], np.float32) for z in (3.0, 1.0, 2.0)])
    return v, np.arange(9, dtype=np.uint32).reshape(3, 3), np.array([0, 1, 2], np.uint32), qs.box()[3]


def test_the_stack_of_three_in_order_and_cut(oracle):
    v, idx, ids, mats = _stack()
    up = _ray((1, 2, 0), (0, 0, 1))
    t, prim, count = mr.first_hits(oracle, v, idx, ids, mats, up)
    assert t[0, :3].tolist() == [1.0, 2.0, 3.0] and prim[0, :3].tolist() == [1, 2, 0] and count[0] == 3
    assert np.isinf(t[0, 3:]).all() and (prim[0, 3:] == MISS).all()
    for k in range(1, mr.KEEP + 1):                                             # truncation at each max_hits: the prefix, then misses
        rec = mr.records(up, t, prim, k, v, idx, ids)
        assert rec.shape == (1, k, 8)
        assert rec[0, :, 1].tolist() == [1, 2, 0][:k] + [MISS] * max(0, k - 3)
        assert rec[0, :, 0].view(np.float32).tolist() == [1.0, 2.0, 3.0][:k] + [-1.0] * max(0, k - 3)
        assert np.array_equal(rec[0, 3:], qr.miss_records(max(0, k - 3)))
        assert rec[0, :min(k, 3), 7].tolist() == [1, 2, 0][:k]                  # each record carries its own triangle's material
        assert (rec[0, :min(k, 3), 4:7].view(np.float32) == np.array([0, 0, -1], np.float32)).all()      # towards the origin of the ray
    down = _ray((1, 2, 10), (0, 0, -2))                                         # t in units of the direction's length
    t, prim, count = mr.first_hits(oracle, v, idx, ids, mats, down)
    assert t[0, :3].tolist() == [3.5, 4.0, 4.5] and prim[0, :3].tolist() == [0, 2, 1] and count[0] == 3


def test_the_interval_is_open_and_cuts_the_stack(oracle):
    v, idx, ids, mats = _stack()
    cases = {(0.0, 2.0): [1], (2.0, np.inf): [0], (1.0, 3.0): [2], (1.5, 2.5): [2], (0.0, 1.0): [], (3.0, np.inf): [], (0.5, 3.5): [1, 2, 0],
             (-np.inf, 2.5): [1, 2]}
    rays = np.concatenate([_ray((1, 2, 0), (0, 0, 1), a, b) for a, b in cases])
    t, prim, count = mr.first_hits(oracle, v, idx, ids, mats, rays)
    for i, want in enumerate(cases.values()):
        assert prim[i, :len(want)].tolist() == want and (prim[i, len(want):] == MISS).all() and count[i] == len(want), (i, prim[i], count[i])


def test_ties_go_to_the_lower_index(oracle):
    """Two coincident triangles (one the other with its vertices in another order) behind a third: the lower index first, both counted"""
    v, idx, ids, mats = _stack()
    v = np.concatenate([v[0:3], v[3:6], v[0:3]])              # z = 3, 1, 3
    idx = np.array([[0, 1, 2], [3, 4, 5], [7, 8, 6]], np.uint32)
    t, prim, count = mr.first_hits(oracle, v, idx, ids, mats, _ray((1, 2, 0), (0, 0, 1)))
    assert t[0, :3].tolist() == [1.0, 3.0, 3.0] and prim[0, :3].tolist() == [1, 0, 2] and count[0] == 3
    rec = mr.records(_ray((1, 2, 0), (0, 0, 1)), t, prim, 2, v, idx, ids)
    assert rec[0, :, 1].tolist() == [1, 0]                    # the cut falls between the two that tie: the lower index stays


@pytest.mark.parametrize("name", ["box", "two_triangles", "zero_area"])
def test_row_0_is_the_closest_hit_and_count_is_any_hit(oracle, name):
    ref, whole = mr.scene_reference(oracle, name), qs.ray_reference(oracle, name)
    for k, r in ref.items():
        rays, rec, occluded = whole[k]
        assert np.array_equal(r.rays, rays)
        assert np.array_equal(r.records(1)[:, 0], rec), k              # the oracle's brute-force trace_closest on the whole scene, as bits
        assert np.array_equal(r.count > 0, occluded), k
        assert np.array_equal((r.prim != MISS).sum(axis=1), np.minimum(r.count, mr.KEEP)), k
        t = np.where(r.prim != MISS, r.t, np.inf)
        assert (t[:, 1:] >= t[:, :-1]).all(), k
        tie = (t[:, 1:] == t[:, :-1]) & (r.prim[:, 1:] != MISS)
        assert (r.prim[:, 1:][tie] > r.prim[:, :-1][tie]).all(), k
        for j in range(1, mr.KEEP + 1):
            assert np.array_equal(r.records(j), r.records(mr.KEEP)[:, :j])


def test_bad_rays_hit_nothing(oracle):
    v, idx, ids, mats = qs.box()
    ref = mr.scene_reference(oracle, "box")["inside"]
    good = ref.rays[(ref.count >= 2) & np.isfinite(ref.rays[:, 7])][0]
    bad, why = qr.bad_rays(good)
    t, prim, count = mr.first_hits(oracle, v, idx, ids, mats, np.concatenate([good[None], bad]))
    assert count[0] >= 2 and prim[0, 1] != MISS
    assert (count[1:] == 0).all() and (prim[1:] == MISS).all(), [why[i] for i in np.flatnonzero(count[1:])]
    rec = mr.records(np.concatenate([good[None], bad]), t, prim, 4, v, idx, ids)
    assert np.array_equal(rec[1:].reshape(-1, 8), qr.miss_records(4 * len(bad)))


def _shares(count):
    return (count == 0).mean(), (count == 1).mean(), (count >= 2).mean()


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_pooled_shares(oracle, name):
    count = np.concatenate([r.count for r in mr.scene_reference(oracle, name).values()])
    shares = _shares(count)
    print(name, "no hit %.3f, one %.3f, two or more %.3f" % shares)
    assert min(shares) >= 0.10, shares


@pytest.mark.parametrize("name", ["box", "sphere", "flat"])
def test_aimed_rays_go_through_several_surfaces(oracle, name):
    count = mr.scene_reference(oracle, name)["aimed"].count
    print(name, "two or more %.3f, more than two %.3f, more than four %.3f" % ((count >= 2).mean(), (count > 2).mean(), (count > 4).mean()))
    assert (count >= 2).mean() >= 0.5 and (count > 2).mean() >= 0.10
    if name == "box":
        assert (count > 4).mean() >= 0.10


def test_copies_tie_twenty_thousand_times(oracle):
    ref = mr.scene_reference(oracle, "copies")
    hits = 0
    for k, r in ref.items():
        hit = r.count > 0
        hits += int(hit.sum())
        assert (r.count[hit] == 20000).all(), k
        assert (r.t[hit] == r.t[hit][:, :1]).all() and (r.prim[hit] == np.arange(mr.KEEP)).all(), k
    assert hits >= 100


def test_copies_lifted_overflow_the_list(oracle):
    r = mr.scene_reference(oracle, "copies_lifted")["aimed"]
    assert len(r.count) == 257
    print("more than 8 hits: %d of 257" % (r.count > mr.KEEP).sum())
    assert (r.count > mr.KEEP).mean() >= 0.25
    full = r.count > mr.KEEP
    assert (np.diff(r.t[full], axis=1) >= 0).all() and (np.diff(r.t[full], axis=1) > 0).any()


def test_inside_by_the_reference(oracle):
    """The default directions of pointsInside on the closed icosphere of tests/test_gpu_multihit.py: no error on 1 000 points, each
    direction alone and the three together"""
    centre, R = (278.0, 274.0, 280.0), 150.0
    v, idx = mr.icosphere(3, centre, R)
    assert idx.shape == (1280, 3)
    edges = np.sort(np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]]), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()          # closed: every edge has two triangles
    pts, inside = mr.shell_points(1000, centre, R)
    assert inside.sum() == 500
    rays, n, m = pt.pathtracer._inside_rays("pointsInside", pts, None)
    assert (n, m) == (1000, 3) and (rays[:, 6] == 0).all() and np.isinf(rays[:, 7]).all()
    count = mr.first_hits(oracle, v, idx, np.zeros(len(idx), np.uint32), qs.box()[3], rays)[2].reshape(n, m)
    odd = (count & 1) != 0
    assert (odd == inside[:, None]).all() and np.array_equal(2 * odd.sum(axis=1) > m, inside)


def test_declarations():
    text = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert re.search(r"\bint\s+pt_query_multi\s*\(\s*pt_ctx\*\s*ctx,\s*const float\*\s*rays,\s*size_t n,\s*uint32_t max_hits,\s*pt_hit\*\s*hits,\s*uint32_t\*\s*counts\)", text)
    assert re.search(r"#define\s+PT_QUERY_MULTI_MAX\s+8\b", text) and _native.QUERY_MULTI_MAX == 8 == mr.KEEP
    assert "pt_query_multi" in _native.ABI_SYMBOLS
    assert "NOT WATERTIGHT" in text
    from acgpathtracing_amd import _build
    assert "multihit.hip" in _build.HIP_SOURCES and "multihit.h" in _build.HIP_HEADERS
    assert not {"multihit.hip", "multihit.h"} & set(_build.KERNEL_SOURCES)


def test_argument_checks_of_the_wrappers():
    rays = np.zeros((4, 8), np.float32)
    E = pt.PathTracerError
    for kw, what in ((dict(max_hits=9), "max_hits"), (dict(max_hits=-1), "max_hits"), (dict(max_hits=2.5), "max_hits"), (dict(max_hits="a"), "max_hits"),
                     (dict(max_hits=0), "counts"), (dict(max_hits=0, counts=False), "counts")):
        with pytest.raises(E, match=what):
            pt.queryRaysMulti(None, rays, **kw)
    for bad in (np.zeros((4, 7), np.float32), np.zeros(8, np.float32), np.zeros((2, 2, 8), np.float32)):
        with pytest.raises(E, match="expected an"):
            pt.queryRaysMulti(None, bad)
    with pytest.raises(E, match="numbers"):
        pt.queryRaysMulti(None, np.zeros((4, 8), object))
    pts = np.zeros((5, 3), np.float32)
    for d in ([(0, 0, 1), (0, 1, 0)], np.zeros((4, 3)) + 1.0, np.zeros((0, 3))):
        with pytest.raises(E, match="odd number"):
            pt.pointsInside(None, pts, directions=d)
    for d, what in (([(0, 0, 1, 0)], "directions"), ([0, 0, 1], "directions"), ([(0, 0, 0)], "not zero"), ([(0, np.nan, 1)], "finite")):
        with pytest.raises(E, match=what):
            pt.pointsInside(None, pts, directions=d)
    for p in (np.zeros((5, 4)), np.zeros(3), np.zeros((5, 3), object)):
        with pytest.raises(E, match="points"):
            pt.pointsInside(None, p)
    assert len(pt.pathtracer.INSIDE_DIRECTIONS) == 3
    assert pt.pathtracer.INSIDE_DIRECTIONS[0] == (0.5377, 0.2673, 0.7996)
