"""The microfacet material model on the GPU (pt_set_material_model, include/acgpt.h): the device BSDF against its NumPy statement
(tests/microfacet_ref.py), the same bits as light mode 1 where the model changes nothing, furnace tests, MIS consistency, updates and
groups, refusals and the Python / command-line entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import microfacet_ref as M
from scene_utils import make_params
from test_gpu_environment import Ctx, _icosphere, _sky, _sun_sky, _sphere_params

pytestmark = pytest.mark.gpu

IEEE, FAST = _native.MATH_IEEE, _native.MATH_FAST
REF, MICRO = _native.MATERIALS_REFERENCE, _native.MATERIALS_MICROFACET
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "acgpathtracing_amd", "acgpt_main")


def _mats_of(c):
    return [_native.Material.from_buffer_copy(m) for m in c.mats]


def _set_mats(c, mats):
    t = (_native.Material * len(mats))(*mats)
    info = _native.UpdateInfo()
    assert c.L.pt_update_materials(c.ctx, C.addressof(t), len(mats), None, 0, C.byref(info)) == 0, c.err()
    c.mats = t


def _mf_hook(c, op, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], 8 if op == 0 else 4), np.float32)
    assert c.L.pt_debug_microfacet(c.ctx, op, x.ctypes.data, x.shape[0], out.ctypes.data) == 0, c.err()
    return out


# ---- 1. the device functions against the NumPy statement ------------------------------------------------------------------------
@pytest.mark.parametrize("math", [IEEE, FAST])
def test_hook_matches_the_reference(math):
    rng = np.random.default_rng(11)
    n = 20000
    bsdf = np.where(rng.random(n) < 0.5, M.METALLIC, M.REFRACTION)
    cos_o = rng.uniform(0.1, 1.0, n) * np.where((bsdf == M.REFRACTION) & (rng.random(n) < 0.4), -1.0, 1.0)
    phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - cos_o ** 2)
    wo = np.stack([s * np.cos(phi), s * np.sin(phi), cos_o], -1).astype(np.float32).astype(np.float64)
    alpha = rng.uniform(0.05, 1.0, n).astype(np.float32).astype(np.float64)
    ior = rng.uniform(1.2, 1.8, n).astype(np.float32).astype(np.float64)
    u = rng.random((n, 3)).astype(np.float32).astype(np.float64)
    c = Ctx.sphere(math=math)
    try:
        out = _mf_hook(c, 0, np.column_stack([wo, alpha, ior, bsdf, u]))
        wi, w, pdf, lobe = M.sample(bsdf, wo, alpha, ior, u[:, 0], u[:, 1], u[:, 2])
        # the lobe choice and the wrong-side test are decisions on float32 values: compare where they are not on a knife's edge
        F = M.fr_dielectric(np.where(cos_o > 0, 1, -1) * np.sum(wo * M._normalize(wo + np.where(lobe[:, None] == 2, 0, 1) * wi), -1), 1.0, ior)
        edge = (np.abs(wi[:, 2]) < 1e-3) | ((bsdf == M.REFRACTION) & (np.abs(u[:, 2] - F) < 1e-3))
        same_lobe = out[:, 7].astype(int) == lobe
        assert (~same_lobe & ~edge).sum() == 0, np.nonzero(~same_lobe & ~edge)
        k = same_lobe & ~edge & (lobe > 0)
        assert k.sum() > 0.8 * n
        # IEEE: float32 against float64 operations in the same order; D (hence pdf) is ill-conditioned near h = N for small alpha:
        # its denominator 1 - cos^2(h) (1 - alpha^2) >= alpha^2 loses ~1e-7 / alpha^2 relative.  Fast math: v_rcp / v_sqrt / v_rsq are
        # 1 ulp, v_sin / v_cos of 2 pi u about 2e-6 absolute: ~100 times the IEEE level.  The weight's Lambda(wi) divides by cos_i^2:
        # a few grazing directions in 1e4 (measured: 9 of 52 551) lose up to 8e-5 relative at IEEE, 2e-5 everywhere else
        tol = 1.0 if math == IEEE else 100.0
        np.testing.assert_allclose(out[k, :3], wi[k], atol=2e-5 * tol)
        np.testing.assert_allclose(out[k, 3:6], w[k], rtol=1.5e-4 * tol, atol=2e-6 * tol)
        assert np.mean(np.all(np.abs(out[k, 3:6] - w[k]) <= 2e-5 * tol * np.abs(w[k]) + 2e-6 * tol, axis=1)) > 0.999
        rel = np.abs(out[k, 6] / pdf[k] - 1.0)
        # (the refraction Jacobian's (wo.h + eta wi.h)^2 cancels near grazing refraction: the same few in 1e4 lose up to 1.4e-4)
        assert np.all(rel < tol * (3e-4 + 1e-6 / alpha[k] ** 2)), rel.max()
        assert np.mean(rel < tol * (3e-5 + 1e-6 / alpha[k] ** 2)) > 0.999
        # eval at the sampled direction: the same pdf and f |cos_i| / pdf = weight
        ev = _mf_hook(c, 1, np.column_stack([wo[k], out[k, :3], alpha[k], ior[k], bsdf[k]]))
        ev64 = M.evaluate(bsdf[k], wo[k], out[k, :3].astype(np.float64), alpha[k], ior[k])
        np.testing.assert_allclose(ev[:, :3], ev64[0], rtol=1e-3 * tol, atol=1e-6)
        np.testing.assert_allclose(ev[:, 3], ev64[1], rtol=1e-3 * tol, atol=1e-6)
        ratio = ev[:, :3] * np.abs(out[k, 2:3]) / ev[:, 3:4]
        np.testing.assert_allclose(ratio, out[k, 3:6], rtol=2e-3 * tol, atol=1e-5)
    finally:
        c.close()


# ---- 2. the same bits where nothing should differ --------------------------------------------------------------------------------
def _box_without_rough(c):
    mats = _mats_of(c)
    for m in mats:
        if m.bsdfType == 1:
            m.bsdfType = 0            # the metal becomes diffuse
        if m.bsdfType == 2:
            m.roughness = 0.0         # smooth glass
    _set_mats(c, mats)


@pytest.mark.parametrize("math", [IEEE, FAST])
@pytest.mark.parametrize("with_map", [False, True])
def test_diffuse_and_smooth_glass_keep_light_mode_1_bits(math, with_map):
    c = Ctx.box(math=math, light=1)
    try:
        _box_without_rough(c)
        if with_map:
            assert c.env(_sky()) == 0
        p = make_params(96, 64, 8, 6, True, True)
        for batch in (False, True):
            assert c.L.pt_set_material_model(c.ctx, REF) == 0
            a, sa = c.render(p, frames=3, batch=batch)
            assert c.L.pt_set_material_model(c.ctx, MICRO) == 0
            b, sb = c.render(p, frames=3, batch=batch)
            name = c.L.pt_variant_name(int(sb.variant)).decode()
            assert name.startswith("LIGHTS GGX ENV" if with_map else "LIGHTS GGX") and ("ENV" in name) == with_map, name
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert (sa.radiance_rays, sa.shadow_rays, sa.paths) == (sb.radiance_rays, sb.shadow_rays, sb.paths)
        parts = np.zeros_like(b)
        whole, _ = c.render(p, frames=1)
        for rank in range(2):
            assert c.L.pt_set_partition(c.ctx, rank, 2) == 0
            img, _ = c.render(p, frames=1)
            parts += img
        assert c.L.pt_set_partition(c.ctx, 0, 1) == 0
        assert np.array_equal(parts[..., :3].view(np.uint32), whole[..., :3].view(np.uint32))
    finally:
        c.close()


# ---- 3. furnace: a Kd = 1 sphere of metal in a white map ---------------------------------------------------------------------------
def _facets(p, verts, idx):
    """per pixel: cos_o of the pixel centre's camera ray against the facet it hits, and whether the pixel's four corners hit that facet"""
    w, h = p.width, p.height
    eye = np.array([p.cameraEye.x, p.cameraEye.y, p.cameraEye.z])
    U, V, W = (np.array([v.x, v.y, v.z]) for v in (p.cameraU, p.cameraV, p.cameraW))
    tri = verts[idx.reshape(-1, 3), :3].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)

    def hit(fx, fy):
        d = (2 * fx / w - 1)[..., None] * U + (2 * fy / h - 1)[..., None] * V + W
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        d = d.reshape(-1, 3)
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        pv = np.cross(d[:, None], e2[None])
        det = np.sum(e1[None] * pv, -1)
        tv = eye - tri[:, 0]
        uu = np.sum(tv[None] * pv, -1) / det
        qv = np.cross(tv[None], e1[None])
        vv = np.sum(d[:, None] * qv, -1) / det
        t = np.sum(e2[None] * qv, -1) / det
        ok = (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t > 0)
        t = np.where(ok, t, np.inf)
        f = np.argmin(t, axis=1)
        f[~np.isfinite(t.min(axis=1))] = -1
        return f.reshape(h, w), d.reshape(h, w, 3)

    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    f0, d0 = hit(xs + 0.5, ys + 0.5)
    same = f0 >= 0
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        same &= hit(xs + dx, ys + dy)[0] == f0
    cos_o = np.abs(np.sum(n[np.maximum(f0, 0)] * d0, -1))
    return f0, cos_o, same


def _metal_sphere(alpha, **kw):
    v, f = _icosphere()
    m = _native.Material()
    m.diffuse = _native.Float3(1.0, 1.0, 1.0); m.ior = 1.5; m.bsdfType = 1; m.roughness = alpha
    c = Ctx(v, f.ravel(), [m], np.zeros(len(f), np.uint32), **kw)
    return c, v, f


@pytest.mark.parametrize("dl", [True, False])
def test_furnace_rough_metal(dl):
    c, v, f = _metal_sphere(0.3, light=1)
    try:
        assert c.L.pt_set_material_model(c.ctx, MICRO) == 0
        assert c.env(np.ones((16, 32, 3), np.float32)) == 0
        p = _sphere_params(spp=64, depth=4, dl=dl, is_=True)
        face, cos_o, inside = _facets(p, v, f.ravel())
        img, _ = c.render(p, frames=4)
        grid = np.linspace(0.05, 1.0, 20)
        alb = np.array([M.albedo(M.METALLIC, cg, 0.3, n=100000, seed=i)[0] for i, cg in enumerate(grid)])
        for lo_c, hi_c in ((0.2, 0.7), (0.7, 0.85), (0.85, 1.0)):
            m = inside & (cos_o >= lo_c) & (cos_o < hi_c)
            assert m.sum() > 20, (lo_c, m.sum())
            exp = np.stack([np.interp(cos_o[m], grid, alb[:, ch]) for ch in range(3)], -1)
            got = img[..., :3][m].astype(np.float64)
            diff = (got - exp).mean(0)
            sigma = got.std(0) / np.sqrt(m.sum())
            # 3 sigma plus the NumPy albedo's own Monte-Carlo error and its linear interpolation (< 2e-3)
            assert np.all(np.abs(diff) < 3 * sigma + 3e-3), (lo_c, diff, sigma)
    finally:
        c.close()


def test_furnace_smooth_metal_is_fresnel():
    c, v, f = _metal_sphere(0.0, light=1, math=IEEE)
    try:
        assert c.L.pt_set_material_model(c.ctx, MICRO) == 0
        assert c.env(np.ones((16, 32, 3), np.float32)) == 0
        p = _sphere_params(spp=8, depth=4, dl=True, is_=True)
        face, cos_o, inside = _facets(p, v, f.ravel())
        img, _ = c.render(p, frames=1)
        m = inside & (cos_o > 0.2)
        assert m.sum() > 200
        F = M.fresnel_conductor(cos_o[m])
        # one path per sample: the mirror sends it to the map (L = 1) with throughput F(cos_o), and the roulette after the hit keeps it
        # with p = min(1, lum(F)) and divides by p.  So a pixel is (k / spp) F / p for the k of its spp samples that survived: per
        # channel F's own ratios, times an integer over spp.  Across a pixel the view direction turns by < 0.01 rad (the camera's 0.35
        # half-width over 48 pixels), so cos_o moves by < 0.01 and F, whose slope is below 0.5, by < 5e-3 (under 1 % of F)
        p = np.minimum(1.0, F @ np.array([0.30, 0.59, 0.11]))
        k = img[..., :3][m] * p[:, None] / F * 8
        kr = np.round(k[:, 1:2])
        off = np.abs(k - kr) >= 0.08 * np.maximum(1.0, kr)
        assert not off.any(), k[off.any(axis=1)][:5]
        assert kr.mean() > 4
    finally:
        c.close()


# ---- 4. MIS: light and BSDF sampling converge to the same image --------------------------------------------------------------------
def _box_micro(alpha_metal=None, alpha_glass=None, **kw):
    c = Ctx.box(light=1, **kw)
    mats = _mats_of(c)
    for m in mats:
        if m.bsdfType == 1 and alpha_metal is not None:
            m.roughness = alpha_metal
        if m.bsdfType == 2 and alpha_glass is not None:
            m.roughness = alpha_glass
    _set_mats(c, mats)
    assert c.L.pt_set_material_model(c.ctx, MICRO) == 0
    return c


def _mis_runs(make, p_of, env=None):
    runs = {}
    for key, dl, spp, frames, frame0 in (("ref", True, 128, 8, 0), ("dl", True, 32, 1, 0), ("dl2", True, 32, 1, 1000),
                                         ("nodl", False, 32, 1, 0), ("nodl2", False, 32, 1, 1000), ("nois", True, 32, 1, 0), ("nois2", True, 32, 1, 1000)):
        c = make()
        try:
            if env is not None:
                assert c.env(env) == 0
            p = p_of(spp, dl, key.startswith("nois") is False)
            img, _ = c.render(p, frames=frames, frame0=frame0)
            if frame0:
                img = img * np.float32(frame0 + 1)
            runs[key] = img[..., :3].astype(np.float64)
        finally:
            c.close()
    ref = runs["ref"]
    mse = {k: float(((runs[k] - ref) ** 2).mean()) for k in ("dl", "nodl", "nois")}
    noise = {k: float(((runs[k] - runs[k + "2"]) ** 2).mean()) / 2 for k in ("dl", "nodl", "nois")}
    for k in mse:       # bias-free: the error against the converged image is the estimator's own noise plus the reference's
        assert mse[k] < 1.5 * noise[k] + 0.5 * mse["dl"], (k, mse, noise)
    return mse


@pytest.mark.parametrize("alpha", [0.05, 0.3])
def test_mis_rough_metal_under_the_area_light(alpha):
    mse = _mis_runs(lambda: _box_micro(alpha_metal=alpha), lambda spp, dl, is_: make_params(96, 64, spp, 6, dl, is_))
    print("rough metal alpha %.2f: MSE at 32 spp against 1024 spp" % alpha, mse, "DL off / DL on = %.2f" % (mse["nodl"] / mse["dl"]))
    if alpha == 0.3:
        assert mse["nodl"] > 2 * mse["dl"], mse


@pytest.mark.parametrize("alpha", [0.05, 0.3])
def test_mis_rough_metal_under_the_sun(alpha):
    def make():
        c, _, _ = _metal_sphere(alpha, light=1)
        m = _mats_of(c)
        m[0].diffuse = _native.Float3(0.8, 0.8, 0.8)
        _set_mats(c, m)
        assert c.L.pt_set_material_model(c.ctx, MICRO) == 0
        return c
    mse = _mis_runs(make, lambda spp, dl, is_: _sphere_params(spp=spp, depth=6, dl=dl, is_=is_), env=_sun_sky())
    print("rough metal alpha %.2f under the sun: DL off / DL on = %.2f" % (alpha, mse["nodl"] / mse["dl"]), mse)


def test_mis_rough_glass():
    mse = _mis_runs(lambda: _box_micro(alpha_glass=0.2), lambda spp, dl, is_: make_params(96, 64, spp, 6, dl, is_))
    print("rough glass alpha 0.2:", mse)


# ---- 5. continuity: small alpha approaches the smooth image ----------------------------------------------------------------------
def test_small_alpha_is_close_to_smooth():
    def render(am, ag, spp):
        c = _box_micro(alpha_metal=am, alpha_glass=ag)
        try:
            img, _ = c.render(make_params(96, 64, spp, 6, True, True), frames=2)
            return img[..., :3].astype(np.float64)
        finally:
            c.close()
    smooth = render(0.0, 0.0, 256)
    near = render(0.01, 0.01, 64)
    far = render(0.3, 0.3, 64)
    e_near, e_far = ((near - smooth) ** 2).mean(), ((far - smooth) ** 2).mean()
    print("continuity: MSE to smooth at alpha 0.01 %.3e, at 0.3 %.3e" % (e_near, e_far))
    assert e_near < 0.5 * e_far, (e_near, e_far)


# ---- 6. updates and groups --------------------------------------------------------------------------------------------------------
def test_updates_equal_a_fresh_scene():
    p = make_params(64, 48, 8, 6, True, True)
    a = _box_micro(alpha_metal=0.25, alpha_glass=0.15)          # roughness set by pt_update_materials
    try:
        got_upd, _ = a.render(p, frames=2)
        verts = np.ascontiguousarray(a.verts)
        info = _native.UpdateInfo()
        assert a.L.pt_update_vertices(a.ctx, verts.ctypes.data, verts.size // 4, 0, C.byref(info)) == 0, a.err()    # refit
        got_refit, _ = a.render(p, frames=2)
        assert a.L.pt_update_vertices(a.ctx, verts.ctypes.data, verts.size // 4, 1, C.byref(info)) == 0, a.err()    # rebuild
        got_rebuild, _ = a.render(p, frames=2)
        assert a.L.pt_set_sample_chunks(a.ctx, 1) == 0
        got_one, _ = a.render(p, frames=1)
        mats = _mats_of(a)
    finally:
        a.close()
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj"))
    b = Ctx(obj.getVerticesFloat(), obj.getIndexBuffer(), mats, obj.getMaterialIndices(), light=1)
    try:
        assert b.L.pt_set_material_model(b.ctx, MICRO) == 0
        fresh, _ = b.render(p, frames=2)
        assert b.L.pt_set_sample_chunks(b.ctx, 1) == 0
        fresh_one, _ = b.render(p, frames=1)
    finally:
        b.close()
    for g in (got_upd, got_refit, got_rebuild):
        assert np.array_equal(g.view(np.uint32), fresh.view(np.uint32))
    assert np.array_equal(got_one.view(np.uint32), fresh_one.view(np.uint32))


def test_group_rehearsal_equals_one_device(monkeypatch):
    monkeypatch.setenv("ACGPT_REHEARSE_SAME_GPU", "1")
    p = make_params(64, 48, 8, 6, True, True)
    one = _box_micro(alpha_metal=0.3, alpha_glass=0.2)
    try:
        a, _ = one.render(p, frames=2)
        mats = _mats_of(one)
    finally:
        one.close()
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj"))
    g = Ctx(obj.getVerticesFloat(), obj.getIndexBuffer(), mats, obj.getMaterialIndices(), light=1, device_ids=[0, 0])
    try:
        assert g.L.pt_set_material_model(g.ctx, MICRO) == 0
        b, st = g.render(p, frames=2)
        assert g.L.pt_variant_name(int(st.variant)).decode().startswith("LIGHTS GGX")
    finally:
        g.close()
    np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6)


# ---- 7. refusals and entry points --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_and_the_context_usable():
    c = Ctx.box(light=0)
    try:
        L = c.L
        assert L.pt_set_material_model(c.ctx, 2) != 0 and L.pt_set_material_model(c.ctx, -1) != 0
        assert L.pt_set_material_model(c.ctx, MICRO) == 0
        p = make_params(32, 32, 4, 4, True, True)
        n = 32 * 32 * 16
        buf = C.c_void_p()
        assert L.pt_device_malloc(c.ctx, C.byref(buf), n) == 0
        try:
            mark = np.full((32, 32, 4), 7.25, np.float32)
            assert L.pt_copy_to_device(c.ctx, buf, mark.ctypes.data, n) == 0
            p.accumulationBuffer = buf.value
            p.handle = L.pt_scene_handle(c.ctx)
            assert L.pt_launch(c.ctx, C.byref(p)) != 0
            msg = L.pt_last_error(c.ctx).decode()
            assert "pt_set_light_mode" in msg and "pt_set_material_model" in msg, msg
            assert L.pt_launch_frames(c.ctx, C.byref(p), 2) != 0
            back = np.zeros_like(mark)
            assert L.pt_copy_to_host(c.ctx, back.ctypes.data, buf, n) == 0
            assert np.array_equal(back, mark)
        finally:
            L.pt_device_free(c.ctx, buf)
        assert L.pt_set_light_mode(c.ctx, 1) == 0
        img, st = c.render(p, frames=1)
        assert st.paths == 32 * 32 * 4 and np.isfinite(img).all()
    finally:
        c.close()


def test_python_api_and_cli(tmp_path):
    state, obj = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=48, height=32, max_depth=4,
                          direct_lighting=True, importance_sampling=True, spp=4)
    try:
        pt.setLightMode(state, 1)
        h = pt.TemporalHistory()
        key0 = h._settings_of(state)
        pt.setMaterialModel(state, "microfacet")
        key1 = h._settings_of(state)
        assert key0 != key1 and key0[5] == 1 and key1[5] == 1 | (1 << 8)
        ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 48, 32, state)
        pt.updateState(ob, state)
        state.params.currentFrameIdx = 0
        pt.LaunchCurrentFrame(ob, state)
        assert pt.getStats(state).paths == 48 * 32 * 4
        with pytest.raises(Exception):
            pt.setMaterialModel(state, 5)
    finally:
        pt.CleanAllTheThings(state)
    out = str(tmp_path / "micro.ppm")
    r = subprocess.run([MAIN, "--obj", os.path.join(pt.SCENES, "cornell_box.obj"), "--width", "64", "--height", "48", "--frames", "1",
                        "--spp-per-launch", "4", "--light-mode", "1", "--materials", "microfacet", "--out", out,
                        "--history-out", str(tmp_path / "m.hist")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(out) > 64 * 48 * 3
    r2 = subprocess.run([MAIN, "--obj", os.path.join(pt.SCENES, "cornell_box.obj"), "--width", "64", "--height", "48", "--frames", "1",
                         "--spp-per-launch", "4", "--light-mode", "1", "--out", str(tmp_path / "ref.ppm"),
                         "--history-in", str(tmp_path / "m.hist")], capture_output=True, text=True, timeout=120)
    assert r2.returncode != 0 and "light mode" in (r2.stdout + r2.stderr)
    r3 = subprocess.run([MAIN, "--obj", os.path.join(pt.SCENES, "cornell_box.obj"), "--materials", "microfacet", "--out", str(tmp_path / "x.ppm"),
                         "--width", "16", "--height", "16", "--frames", "1", "--spp-per-launch", "1"], capture_output=True, text=True, timeout=120)
    assert r3.returncode != 0
