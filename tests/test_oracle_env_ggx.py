"""The CPU oracle's environment map and microfacet model (oracle/oracle_pt.cpp) against their float64 statements (tests/env_ref.py,
tests/microfacet_ref.py), function by function, and its light-mode-1 estimator with a map and GGX materials on its own: furnace tests,
MIS consistency, a black map against no map, both builds and any thread count.  These pin the oracle that
tests/test_gpu_env_ggx_parity.py holds the ENV and GGX render kernels to, so that a mistake copied from the device code into the oracle
does not go unseen."""
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import microfacet_ref as M
import oracle_lib
from env_ref import EnvRef, sphere_directions
from scene_utils import copy_params, make_params
from test_gpu_environment import _icosphere, _sky, _sun_sky, _sphere_params
from test_gpu_microfacet import _facets

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
DIFFUSE_BOX = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_scene(orc, path=BOX, roughness=None):
    """the OBJ's scene in the oracle; roughness: {bsdfType: value} written into the materials' Pr"""
    obj = pt.TinyObjWrapper(path)
    mats = obj.getMaterials()
    if roughness:
        mats = (_native.Material * len(mats))(*[_native.Material.from_buffer_copy(m) for m in mats])
        for m in mats:
            if m.bsdfType in roughness:
                m.roughness = roughness[m.bsdfType]
    return orc.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), mats)


def sphere_scene(orc, kd=0.5, bsdf=0, roughness=0.0):
    v, f = _icosphere()
    m = _native.Material()
    m.diffuse = _native.Float3(kd, kd, kd); m.ior = 1.5; m.bsdfType = bsdf; m.roughness = roughness
    mats = (_native.Material * 1)(m)
    return orc.scene(v, f.ravel(), np.zeros(len(f), np.uint32), mats), v, f


def env_maps():
    """the maps the CDF test covers: (name, rgb [h, w, 3], scale)"""
    r = np.random.default_rng(3)
    rows = _sky(16, 40, seed=9)
    rows[[0, 5, 6, 15]] = 0.0                                   # black rows, the poles among them
    rows[8, ::3] = 0.0                                          # zero-weight texels inside a row
    return [("1x1", np.array([[[0.3, 2.0, 0.7]]], np.float32), (1.0, 1.0, 1.0)),
            ("700 wide", r.uniform(0.0, 4.0, (3, 700, 3)).astype(np.float32), (1.0, 1.0, 1.0)),
            ("513 wide", r.uniform(0.0, 1.0, (5, 513, 3)).astype(np.float32) ** 4, (1.0, 1.0, 1.0)),
            ("black rows", rows, (1.0, 1.0, 1.0)),
            ("black", np.zeros((8, 16, 3), np.float32), (1.0, 1.0, 1.0)),
            ("scaled", _sky(), (2.0, 0.75, 0.3)),
            ("1 row", _sky(1, 64, seed=4), (1.0, 1.0, 1.0))]


@pytest.fixture(scope="module")
def sphere(oracle):
    sc, _, _ = sphere_scene(oracle)
    return sc


# ---- 1. the map's tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,img,scale", env_maps(), ids=[m[0] for m in env_maps()])
def test_cdfs_match_env_ref(sphere, name, img, scale):
    sphere.set_environment(img, scale)
    t = sphere.environment_tables()
    ref = EnvRef(img, scale)
    assert np.array_equal(_u32(t["texels"][..., :3]), _u32(ref.rgb))
    assert np.array_equal(_u32(t["texels"][..., 3]), _u32(ref.weight))
    assert np.array_equal(_u32(t["conditional"]), _u32(ref.cond))
    assert np.array_equal(_u32(t["marginal"]), _u32(ref.marg))
    assert _u32(t["total"]) == _u32(ref.total) and _u32(t["pdf_scale"]) == _u32(ref.pdf_scale)
    assert t["p_env"] == (1.0 if ref.total > 0 else 0.0)      # no emissive triangle: every light sample goes to the map
    sphere.set_environment(None)
    assert sphere.environment_tables() is None


def test_p_env_beside_emissive_triangles(oracle):
    sc = box_scene(oracle)
    sc.set_environment(_sky())
    assert sc.environment_tables()["p_env"] == 0.5
    sc.set_environment(np.zeros((4, 8, 3), np.float32))
    assert sc.environment_tables()["p_env"] == 0.0


# ---- 2. lookup, pdf and sample ---------------------------------------------------------------------------------------------------
def test_map_functions_match_env_ref(sphere):
    """test_gpu_environment.py::test_hook_matches_the_reference's checks and tolerances (IEEE), on the oracle's hook"""
    img = _sky()
    img[3, 7] = (300.0, 200.0, 100.0)
    img[20, 30:34] = 0.0
    sphere.set_environment(img, (2.0, 1.0, 0.5))
    try:
        ref = EnvRef(img, (2.0, 1.0, 0.5))
        d = sphere_directions(20000, 1)
        far = ref.edge_distance(d) > 1e-4
        rgb = sphere.env_hook(0, d)
        row, col = ref.texel(d)
        assert np.array_equal(rgb[far, 3].astype(np.int64), (row * ref.w + col)[far])
        assert np.array_equal(rgb[far, :3].view(np.uint32), ref.eval(d)[far].view(np.uint32))
        pdf = sphere.env_hook(1, d)[:, 0]
        assert np.allclose(pdf[far], ref.pdf(d)[far], rtol=1e-5, atol=0)
        u = np.random.default_rng(2).uniform(size=(4000, 2)).astype(np.float32)
        s = sphere.env_hook(2, u)
        checked = 0
        for (u1, u2), got in zip(u, s):
            dr, pr, _, (fv, fu) = ref.sample(float(u1), float(u2))
            if min(fv, 1 - fv, fu, 1 - fu) < 1e-3:
                continue
            assert np.allclose(got[:3], dr, atol=1e-5), (u1, u2, got, dr)
            assert abs(got[3] - pr) <= 1e-4 * pr
            checked += 1
        assert checked > 3500
        # the sample's pdf is the pdf of its direction (away from texel edges)
        far_s = ref.edge_distance(s[:, :3]) > 1e-4
        rel = np.abs(sphere.env_hook(1, s[far_s, :3])[:, 0] / s[far_s, 3] - 1.0)
        assert rel.max() < 1e-4                                # sin(theta) from d.y against sin(pi v): a few ulp apart
    finally:
        sphere.set_environment(None)
    assert np.all(sphere.env_hook(0, d)[:, 3] == -1.0) and np.all(sphere.env_hook(1, d) == 0.0)


# ---- 3. the microfacet BSDF ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grazing", [False, True])
def test_microfacet_functions_match_reference(oracle, grazing):
    """test_gpu_microfacet.py::test_hook_matches_the_reference's checks and IEEE tolerances on the oracle's hook: metal and glass,
    entering and exiting, alpha 0.05 ... 1; grazing: |cos_o| in [0.02, 0.1]"""
    rng = np.random.default_rng(11 + grazing)
    n = 20000
    bsdf = np.where(rng.random(n) < 0.5, M.METALLIC, M.REFRACTION)
    lo = (0.02, 0.1) if grazing else (0.1, 1.0)
    cos_o = rng.uniform(*lo, n) * np.where((bsdf == M.REFRACTION) & (rng.random(n) < 0.4), -1.0, 1.0)
    phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - cos_o ** 2)
    wo = np.stack([s * np.cos(phi), s * np.sin(phi), cos_o], -1).astype(np.float32).astype(np.float64)
    alpha = rng.uniform(0.05, 1.0, n).astype(np.float32).astype(np.float64)
    ior = rng.uniform(1.2, 1.8, n).astype(np.float32).astype(np.float64)
    u = rng.random((n, 3)).astype(np.float32).astype(np.float64)
    out = oracle.microfacet_hook(0, np.column_stack([wo, alpha, ior, bsdf, u]))
    wi, w, pdf, lobe = M.sample(bsdf, wo, alpha, ior, u[:, 0], u[:, 1], u[:, 2])
    F = M.fr_dielectric(np.where(cos_o > 0, 1, -1) * np.sum(wo * M._normalize(wo + np.where(lobe[:, None] == 2, 0, 1) * wi), -1), 1.0, ior)
    edge = (np.abs(wi[:, 2]) < 1e-3) | ((bsdf == M.REFRACTION) & (np.abs(u[:, 2] - F) < 1e-3))
    same_lobe = out[:, 7].astype(int) == lobe
    assert (~same_lobe & ~edge).sum() == 0, np.nonzero(~same_lobe & ~edge)
    k = same_lobe & ~edge & (lobe > 0)
    assert k.sum() > (0.5 if grazing else 0.8) * n
    n_min = 100 if grazing else 500                            # (grazing exits mostly reflect: total internal reflection)
    assert ((lobe[k] == 2) & (cos_o[k] > 0)).sum() > n_min and ((lobe[k] == 2) & (cos_o[k] < 0)).sum() > n_min    # entering, exiting
    np.testing.assert_allclose(out[k, :3], wi[k], atol=2e-5)
    np.testing.assert_allclose(out[k, 3:6], w[k], rtol=1.5e-4, atol=2e-6)
    assert np.mean(np.all(np.abs(out[k, 3:6] - w[k]) <= 2e-5 * np.abs(w[k]) + 2e-6, axis=1)) > 0.999
    rel = np.abs(out[k, 6] / pdf[k] - 1.0)
    assert np.all(rel < 3e-4 + 1e-6 / alpha[k] ** 2), rel.max()
    assert np.mean(rel < 3e-5 + 1e-6 / alpha[k] ** 2) > 0.999
    ev = oracle.microfacet_hook(1, np.column_stack([wo[k], out[k, :3], alpha[k], ior[k], bsdf[k]]))
    ev64 = M.evaluate(bsdf[k], wo[k], out[k, :3].astype(np.float64), alpha[k], ior[k])
    np.testing.assert_allclose(ev[:, :3], ev64[0], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(ev[:, 3], ev64[1], rtol=1e-3, atol=1e-6)
    ratio = ev[:, :3] * np.abs(out[k, 2:3]) / ev[:, 3:4]
    np.testing.assert_allclose(ratio, out[k, 3:6], rtol=2e-3, atol=1e-5)
    # where mf_sample cannot draw wi, mf_eval is zero: reflection for a wi below the plane of a metal
    k &= cos_o > 0
    below = np.column_stack([wo[k], out[k, 0], out[k, 1], -np.abs(out[k, 2]), alpha[k], ior[k], np.full(k.sum(), M.METALLIC)])
    assert np.all(oracle.microfacet_hook(1, below) == 0.0)


# ---- 4. the estimator on its own -------------------------------------------------------------------------------------------------
def _render(sc, p, frames=1, threads=0, **kw):
    acc = None
    for f in range(frames):
        q = copy_params(p)
        q.currentFrameIdx = f
        acc, _, st, _ = sc.render(q, accumulation=acc, threads=threads, **kw)
    return acc, st


def _sphere_mask(orc, p, frames):
    """pixels the sphere covers, and pixels it does not touch: black and white under a white map with kd = 0"""
    sc, _, _ = sphere_scene(orc, kd=0.0)
    sc.set_environment(np.ones((16, 32, 3), np.float32))
    img, _ = _render(sc, p, frames=frames)
    return np.all(img[..., :3] == 0.0, axis=-1), np.all(img[..., :3] == 1.0, axis=-1)


@pytest.mark.parametrize("light,dl,is_", [(0, False, True), (0, False, False), (0, True, True), (1, True, True), (1, False, True), (1, True, False), (1, False, False)])
def test_furnace(oracle, light, dl, is_):
    """a kd = 0.5 convex sphere in a white map is 0.5 wherever it is seen, in both light modes and under every toggle"""
    p = _sphere_params(spp=64, depth=8, dl=dl, is_=is_)
    mask, bg = _sphere_mask(oracle, p, 2)
    assert mask.sum() > 800 and bg.sum() > 200
    sc, _, _ = sphere_scene(oracle)
    sc.set_light_mode(light)
    sc.set_environment(np.ones((16, 32, 3), np.float32))
    img, _ = _render(sc, p, frames=2)
    v = img[..., 1][mask]
    sigma = v.std() / np.sqrt(v.size)
    assert abs(v.mean() - 0.5) < 3 * sigma + 1e-4, (v.mean(), sigma)
    assert np.all(img[..., :3][bg] == 1.0)                     # the map itself, exactly


def _tame_sun_sky():
    """a sky of 0.2 with a 4 x 4-texel sun of 20 ... 30: bright enough that light sampling of the map matters, tame enough that the
    DL-off estimator (the sun found by BSDF sampling alone) resolves a bias of a few percent at this sample count"""
    img = np.full((32, 64, 3), 0.2, np.float32)
    img[6:10, 20:24] = (30.0, 25.0, 20.0)
    return img


def test_light_mode_1_toggles_agree_with_a_map_beside_the_quad(oracle):
    """the box's emissive quad and a sun-and-sky map: DL on / off and IS on / off converge to the same image.  Paired per pixel: the
    toggles share their camera rays, and pixels are independent, so the mean of the per-pixel difference against DL on / IS on and its
    standard error over the pixels say whether the two estimators agree.  Measured: |difference| <= 1.5 standard errors, with
    standard errors of 2.3e-4 (DL on, IS off) and 1.1e-3 ... 1.2e-3 (DL off) on an image mean of 0.242.  A triangle light sample
    without its 1 / (1 - p_env) (the quad's light-sampled share halved) moves the DL-on image by -0.019: 15 standard errors."""
    sc = box_scene(oracle, DIFFUSE_BOX)
    assert sc.set_light_mode(1) == 2
    sc.set_environment(_tame_sun_sky())
    assert sc.environment_tables()["p_env"] == 0.5
    lum = {}
    for dl, is_ in ((True, True), (False, True), (True, False), (False, False)):
        img, _ = _render(sc, make_params(48, 36, 256, 10, dl, is_), frames=4)
        lum[(dl, is_)] = img[..., :3].astype(np.float64).mean(-1)
    ref = lum[(True, True)]
    assert ref.mean() > 0.2
    for k in ((False, True), (True, False), (False, False)):
        d = lum[k] - ref
        se = d.std() / np.sqrt(d.size)
        print("light mode 1 with a map, DL %d IS %d against DL 1 IS 1: %+.2e (standard error %.1e)" % (k[0], k[1], d.mean(), se))
        assert abs(d.mean()) < 4 * se, (k, d.mean(), se)
        assert se < 0.01 * ref.mean(), (k, se)       # the test resolves a bias of a few percent


@pytest.mark.parametrize("dl", [True, False])
def test_furnace_rough_metal(oracle, dl):
    """test_gpu_microfacet.py::test_furnace_rough_metal on the oracle: a white alpha = 0.3 metal sphere in a white map shows
    microfacet_ref.albedo(cos_o)"""
    sc, v, f = sphere_scene(oracle, kd=1.0, bsdf=1, roughness=0.3)
    sc.set_light_mode(1)
    sc.set_material_model(1)
    sc.set_environment(np.ones((16, 32, 3), np.float32))
    p = _sphere_params(spp=64, depth=4, dl=dl, is_=True)
    _, cos_o, inside = _facets(p, v, f.ravel())
    img, _ = _render(sc, p, frames=2)
    grid = np.linspace(0.05, 1.0, 20)
    alb = np.array([M.albedo(M.METALLIC, cg, 0.3, n=100000, seed=i)[0] for i, cg in enumerate(grid)])
    for lo_c, hi_c in ((0.2, 0.7), (0.7, 0.85), (0.85, 1.0)):
        m = inside & (cos_o >= lo_c) & (cos_o < hi_c)
        assert m.sum() > 20, (lo_c, m.sum())
        exp = np.stack([np.interp(cos_o[m], grid, alb[:, ch]) for ch in range(3)], -1)
        got = img[..., :3][m].astype(np.float64)
        diff = (got - exp).mean(0)
        sigma = got.std(0) / np.sqrt(m.sum())
        assert np.all(np.abs(diff) < 3 * sigma + 3e-3), (lo_c, diff, sigma)


@pytest.mark.parametrize("light", [0, 1])
def test_black_map_and_no_map_give_the_same_bits(oracle, light):
    sc = box_scene(oracle, roughness={1: 0.3, 2: 0.05})
    sc.set_light_mode(light)
    sc.set_material_model(light)
    p = make_params(64, 48, 4, 6, True, True)
    a, sa = _render(sc, p)
    sc.set_environment(np.zeros((8, 16, 3), np.float32))
    b, sb = _render(sc, p)
    sc.set_environment(None)
    c, sc_ = _render(sc, p)
    assert np.array_equal(_u32(a), _u32(b)) and np.array_equal(_u32(a), _u32(c))
    assert sa == sb == sc_


def test_builds_and_threads_agree_with_a_map_and_ggx(built):
    p = make_params(48, 32, 4, 6, True, False)
    res = []
    for name in ("liboracle_pt.so", "liboracle_pt_fma.so"):
        if name.endswith("_fma.so") and not oracle_lib._cpu_has_fma():
            continue
        o = oracle_lib.load_variant(name)
        sc = box_scene(o, roughness={1: 0.3, 2: 0.3})
        sc.set_light_mode(1)
        sc.set_material_model(1)
        sc.set_environment(_sun_sky(), (1.0, 0.5, 2.0))
        for threads in (1, 3, 8):
            acc, st = _render(sc, p, frames=2, threads=threads)
            res.append((name, threads, _u32(acc), st))
        mode0 = box_scene(o)
        mode0.set_environment(_sky())
        acc, st = _render(mode0, p, threads=2)
        res.append((name, "mode 0", _u32(acc), st))
    for r in res:
        ref = next(x for x in res if x[1] == r[1]) if r[1] == "mode 0" else res[0]
        assert np.array_equal(r[2], ref[2]) and r[3] == ref[3], r[:2]
    assert res[0][3]["shadow_rays"] > 0 and np.isfinite(res[0][2].view(np.float32)).all()
