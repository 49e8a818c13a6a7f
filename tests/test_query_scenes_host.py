"""The sets of tests/query_scenes.py are not vacuous — by the references alone, no GPU.

Conditions, per scene, pooled over its sets, wherever query_scenes.SCENES says the condition holds for the scene:
  ray shares         at least a quarter of the rays hit and at least a tenth miss (the oracle's brute force)
  all found          at max_radius = +inf every searchable point finds a triangle
  radius shares      at the sets' finite radii at least a fifth of the points find one and at least a tenth find none
  distinct winners   at least eight different triangles win
  zero-area winners  at least 20 points whose winner is a triangle without area
  ao partial         at least a tenth of the AO points see 0 < visible < K
and on every scene: no set's fp32 statement is dead (d2 NaN or infinite) on more than a twentieth of its pairs of a point and a
triangle with an area, and the fp32 reference's distance agrees with the float64 brute force, relative to the scene's S, to four times the deviation measured here
and recorded in DESIGN.md section 24 (query_scenes.F64_DEVIATION).  Run with -s to see the shares, the deviations and the magnitude
at which the fp32 statement overflows."""
import numpy as np
import pytest

import nearest_ref as nr
import query_scenes as qs

F = np.float32
NAMES = list(qs.SCENES)


def test_the_table_covers_what_the_matrix_needs():
    assert {c[0] for c in qs.CASES} | {"empty", "scaled"} == set(NAMES)
    assert len(qs.sphere()[1]) == 20492 and len(qs.copies()[1]) == 20000 and len(qs.empty()[1]) == 0
    assert qs.SCENES["sphere"].n_queries == 257 and qs.SCENES["copies"].n_queries == 257 and qs.SCENES["box"].n_queries == 1000
    v, idx = qs.zero_area()[:2]
    assert qs.zero_area_mask(v, idx).mean() >= 0.5 and not qs.zero_area_mask(*qs.box()[:2]).any()
    assert np.ptp(qs.flat()[0][:, 1]) == 0 and (qs.point()[0][:, :3] == np.float32(qs.POINT)).all()
    # (2^-7, 4096): a scene 4.4 across at 4096, where an ulp is 2^-11: every coordinate keeps some 13 bits below the offset
    vm = qs.magnitude(*qs.MAGNITUDES["x2^-7plus4096"])[0][:, :3]
    assert vm.min() == 4096.0 and 4.3 < np.ptp(vm) < 4.4 and np.array_equal(vm * F(2048.0), np.round(vm * F(2048.0)))
    for name in ("one_triangle", "two_triangles"):                # points on a vertex, an edge and the face (to fp32's rounding), and far away
        v, idx = qs.SCENES[name].arrays()[:2]
        pts, r, ref_inf, _ = qs.nearest_reference(name)["around"]
        on = ref_inf.view(np.float32)[:, 0] <= 1e-4
        w = ref_inf.view(np.float32)[on][:, 2:4]
        vertex = ((w == 0) | (w == 1)).all(axis=1)
        face = (w > 0).all(axis=1) & (w.sum(axis=1) < 1)
        assert vertex.sum() >= 10 and face.sum() >= 10 and (~vertex & ~face).sum() >= 10
        assert (ref_inf.view(np.float32)[:, 0] == 0).sum() >= 10
        assert (ref_inf.view(np.float32)[:, 0] > 10 * np.ptp(v[:, :3], axis=0).max()).sum() >= 100


@pytest.mark.parametrize("name", NAMES)
def test_rays_hit_and_miss(oracle, name):
    ref = qs.ray_reference(oracle, name)
    hit = np.concatenate([rec[:, 1] != qs.MISS for _, rec, _ in ref.values()])
    occ = np.concatenate([o for _, _, o in ref.values()])
    print("\n%s: %d rays, %.3f hit, %.3f occluded" % (name, hit.size, hit.mean(), occ.mean()))
    assert hit.size == 6 * qs.SCENES[name].n_queries and set(ref) == set(qs.ray_set_names(name))
    if qs.RAY_SHARES in qs.SCENES[name].conditions:
        assert hit.mean() >= 0.25 and (~hit).mean() >= 0.10
        assert occ.mean() >= 0.25 and (~occ).mean() >= 0.10
    else:
        assert not hit.any() and not occ.any()                   # no triangles, or a point


@pytest.mark.parametrize("name", NAMES)
def test_points_find_and_miss(name):
    s = qs.SCENES[name]
    ref = qs.nearest_reference(name)
    v, idx = s.arrays()[:2]
    found_inf = np.concatenate([r[2][:, 1] != qs.MISS for r in ref.values()])
    found_r = np.concatenate([r[3][:, 1] != qs.MISS for r in ref.values()])
    winners = np.unique(np.concatenate([r[2][:, 1] for r in ref.values()] + [r[3][:, 1] for r in ref.values()]))
    winners = winners[winners != qs.MISS]
    print("\n%s: %d points, found %.3f at +inf, %.3f at the radii, %d winners" % (name, found_inf.size, found_inf.mean(), found_r.mean(), winners.size))
    if qs.ALL_FOUND in s.conditions:
        assert found_inf.all()
    if qs.RADIUS_SHARES in s.conditions:
        assert found_r.mean() >= 0.2 and (~found_r).mean() >= 0.1
    if qs.DISTINCT in s.conditions:
        assert winners.size >= 8
    if name in ("copies", "point"):
        assert (winners == 0).all()                              # exact ties: the lowest index
    if name == "empty":
        assert not found_inf.any() and not found_r.any()
    if qs.ZERO_AREA_WINNERS in s.conditions:
        zero = qs.zero_area_mask(v, idx)
        n = 0
        for pts, r, at_inf, at_r in ref.values():
            for rec in (at_inf, at_r):
                f = rec[:, 1] != qs.MISS
                n += int(zero[rec[f, 1]].sum())
        print("    %d answers name a zero-area triangle" % n)
        assert n >= 20
        pts, r, at_inf, at_r = ref["zero_area_features"]
        f = at_r[:, 1] != qs.MISS                  # their own vertices (a midpoint may round off its edge): found at radius 0, on the spot
        assert r == 0 and f.mean() >= 0.5 and (at_r[f, 0] == 0).all() and zero[at_r[f, 1]].sum() >= 20


@pytest.mark.parametrize("name", [n for n in NAMES if n != "empty"])
def test_no_set_is_dead_and_fp32_agrees_with_float64(name):
    s = qs.SCENES[name]
    S = qs.scene_magnitude(name)
    worst = 0.0
    for k, (pts, r, at_inf, at_r) in qs.nearest_reference(name).items():
        dead = qs.dead_share(name, pts)
        assert dead <= 0.05, (name, k, dead)
        d32 = at_inf.view(np.float32)[:, 0].astype(np.float64)
        ok = (at_inf[:, 1] != qs.MISS) & np.isfinite(d32)
        assert ok.all()
        dev = float((np.abs(d32 - qs.f64_distance(name, pts)) / S).max())
        print("\n%s / %s: dead pairs %.4f, fp32 against float64 %.3e of S (S = %.4g)" % (name, k, dead, dev, S))
        worst = max(worst, dev)
    print("%s: largest deviation %.3e of S" % (name, worst))
    assert worst <= 4.0 * qs.F64_DEVIATION[name], (worst, qs.F64_DEVIATION[name])


def test_where_the_fp32_statement_overflows():
    """The box scaled by s with the "shell" set ten diagonals out: the first s at which a pair's d2 is NaN or infinite.  At 1e6 — |q| near
    1e10, va, vb, vc near 1e37 — none is yet, so query_scenes keeps that set where it is; the limit is a product of an edge and a
    distance near sqrt(FLT_MAX) = 1.8e19."""
    v, idx, ids, _ = qs.box()
    v0, e1, e2 = nr.records_of_scene(v, idx)
    pts = nr.point_set("shell", v, idx, qs.camera(qs.SCENES["box"]))[:200]
    first = None
    for e in np.arange(5.0, 8.01, 0.125):
        s = F(10.0 ** e)
        d2 = nr.closest_on_triangle((pts * s)[:, None, :], (v0 * s)[None], (e1 * s)[None], (e2 * s)[None])[0]
        share = float((~np.isfinite(d2)).mean())
        if share > 0 and first is None:
            first = (float(s), share, float(np.abs(pts * s).max()), float(np.abs(v[:, :3] * s).max()))
        if abs(e - 6.0) < 1e-9:
            at_1e6 = share
    print("\nfirst dead pairs at scale %.3g (share %.4f): |q| up to %.3g, S = %.3g; at 1e6 with the shell at ten diagonals: %.4f" % (first + (at_1e6,)))
    assert first is not None and 1e6 < first[0] < 1e7 and at_1e6 == 0
    assert 1e19 < first[2] * first[3] < 1e20


@pytest.mark.parametrize("name", NAMES)
def test_ao_points_see_some_and_not_all(oracle, name):
    P, N, p, vis, ao = qs.ao_reference(oracle, name)
    partial = float(((vis > 0) & (vis < qs.K_AO)).mean())
    print("\n%s: %d AO points, radius %.4g bias %.4g, partly open %.3f, fully open %.3f, closed %.3f" % (name, len(P), p["radius"], p["bias"], partial, (vis == qs.K_AO).mean(), (vis == 0).mean()))
    assert vis[5] == qs.K_AO and vis[17] == qs.K_AO and vis[40] == qs.K_AO           # the no-surface points
    if qs.AO_PARTIAL in qs.SCENES[name].conditions:
        assert partial >= 0.10
    if name in ("empty", "point"):
        assert (vis == qs.K_AO).all()
