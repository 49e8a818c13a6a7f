"""Environment lighting on the GPU (pt_set_environment): the device lookup, pdf and sample against tests/env_ref.py; a black map
changes no bit and no ray count; a constant map is seen exactly; the furnace test in both light modes and every toggle; light
sampling of the map agrees with BSDF sampling and beats it; frame batches and rank partitions; refusals keep the previous map."""
import ctypes as C
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
from env_ref import EnvRef, sphere_directions
from scene_utils import make_params

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
IEEE, FAST = _native.MATH_IEEE, _native.MATH_FAST
ENV, ENV_DEEP, LIGHTS_ENV, DEFAULT, LIGHTS, DEEP = 10, 11, 12, 7, 8, 9


def _icosphere(radius=100.0, subdiv=2):
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        cache, nf = {}, []
        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m)); cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.zeros((len(v), 4), np.float32)
    verts[:, :3] = np.array(v) * radius
    return verts, np.array(f, np.uint32)


class Ctx:
    def __init__(self, verts, idx, mats, mat_ids, math=FAST, light=0, device_ids=None):
        self.L = L = _native.hip()
        self.ctx = C.c_void_p()
        if device_ids:
            dev = (C.c_int * len(device_ids))(*device_ids)
            assert L.pt_create_multi(C.byref(self.ctx), dev, len(device_ids)) == 0
        else:
            assert L.pt_create(C.byref(self.ctx), 0) == 0
        assert L.pt_set_math_mode(self.ctx, math) == 0 and L.pt_set_light_mode(self.ctx, light) == 0
        self.verts, self.idx = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(idx, np.uint32)
        self.mid = np.ascontiguousarray(mat_ids, np.uint32)
        self.mats = (_native.Material * len(mats))(*mats)
        assert L.pt_set_scene(self.ctx, self.verts.ctypes.data, self.verts.size // 4, self.idx.ctypes.data, self.idx.size // 3,
                              self.mid.ctypes.data, C.addressof(self.mats), len(self.mats)) == 0, self.err()

    @classmethod
    def box(cls, **kw):
        obj = pt.TinyObjWrapper(BOX)
        mats = [_native.Material.from_buffer_copy(m) for m in obj.getMaterials()]
        return cls(obj.getVerticesFloat(), obj.getIndexBuffer(), mats, obj.getMaterialIndices(), **kw)

    @classmethod
    def sphere(cls, kd=0.5, **kw):
        v, f = _icosphere()
        m = _native.Material()
        m.diffuse = _native.Float3(kd, kd, kd); m.ior = 1.5; m.bsdfType = 0
        return cls(v, f.ravel(), [m], np.zeros(len(f), np.uint32), **kw)

    def err(self):
        return self.L.pt_last_error(self.ctx)

    def env(self, img, scale=(1.0, 1.0, 1.0)):
        if img is None:
            return self.L.pt_set_environment(self.ctx, None, 0, 0, _native.Float3(*scale))
        img = np.ascontiguousarray(img, np.float32)
        return self.L.pt_set_environment(self.ctx, img.ctypes.data, img.shape[1], img.shape[0], _native.Float3(*scale))

    def hook(self, op, x):
        x = np.ascontiguousarray(x, np.float32)
        n = x.shape[0]
        out = np.zeros((n, 1 if op == 1 else 4), np.float32)
        assert self.L.pt_debug_environment(self.ctx, op, x.ctypes.data, n, out.ctypes.data) == 0, self.err()
        return out

    def render(self, p, frames=1, batch=False, frame0=0):
        """accumulation (float32 [h, w, 4]) and stats of `frames` frames from frame0 (one pt_launch_frames when batch), into a zeroed buffer"""
        L, n = self.L, p.width * p.height * 16
        buf = C.c_void_p()
        assert L.pt_device_malloc(self.ctx, C.byref(buf), n) == 0
        assert L.pt_device_memset(self.ctx, buf, 0, n) == 0
        try:
            p.accumulationBuffer = buf.value
            p.frameBuffer = None
            p.handle = L.pt_scene_handle(self.ctx)
            if batch:
                p.currentFrameIdx = frame0
                assert L.pt_launch_frames(self.ctx, C.byref(p), frames) == 0, self.err()
            else:
                for f in range(frames):
                    p.currentFrameIdx = frame0 + f
                    assert L.pt_launch(self.ctx, C.byref(p)) == 0, self.err()
            st = _native.Stats()
            assert L.pt_get_stats(self.ctx, C.byref(st)) == 0
            out = np.zeros((p.height, p.width, 4), np.float32)
            assert L.pt_copy_to_host(self.ctx, out.ctypes.data, buf, n) == 0
            return out, st
        finally:
            L.pt_device_free(self.ctx, buf)

    def close(self):
        self.L.pt_destroy(self.ctx)


def _sky(h=32, w=64, seed=5):
    r = np.random.default_rng(seed)
    return r.uniform(0.05, 1.0, size=(h, w, 3)).astype(np.float32)


def _sun_sky(h=64, w=128):
    img = np.full((h, w, 3), 0.2, np.float32)
    img[10:13, 40:43] = (900.0, 800.0, 700.0)
    return img


def _sphere_params(w=48, h=48, spp=16, depth=6, dl=True, is_=True):
    p = make_params(w, h, spp, depth, dl, is_)
    p.cameraEye = _native.Float3(0.0, 0.0, -400.0)
    p.cameraU, p.cameraV, p.cameraW = _native.Float3(0.35, 0, 0), _native.Float3(0, 0.35, 0), _native.Float3(0, 0, 1.0)
    p.areaLight.emission = _native.Float3(0.0, 0.0, 0.0)
    return p


# ---- 1. the device functions against the numpy reference ------------------------------------------------------------------------
@pytest.mark.parametrize("math", [IEEE, FAST])
def test_hook_matches_the_reference(math):
    c = Ctx.box(math=math)
    try:
        img = _sky()
        img[3, 7] = (300.0, 200.0, 100.0)
        img[20, 30:34] = 0.0
        assert c.env(img, (2.0, 1.0, 0.5)) == 0, c.err()
        ref = EnvRef(img, (2.0, 1.0, 0.5))
        d = sphere_directions(20000, 1)
        far = ref.edge_distance(d) > 1e-4
        rgb = c.hook(0, d)
        row, col = ref.texel(d)
        assert np.array_equal(rgb[far, 3].astype(np.int64), (row * ref.w + col)[far])
        assert np.array_equal(rgb[far, :3].view(np.uint32), ref.eval(d)[far].view(np.uint32))
        pdf = c.hook(1, d)[:, 0]
        rp = ref.pdf(d)
        assert np.allclose(pdf[far], rp[far], rtol=1e-5, atol=0)
        u = np.random.default_rng(2).uniform(size=(4000, 2)).astype(np.float32)
        s = c.hook(2, u)
        checked = 0
        for (u1, u2), got in zip(u, s):
            dr, pr, _, (fv, fu) = ref.sample(float(u1), float(u2))
            if min(fv, 1 - fv, fu, 1 - fu) < 1e-3:
                continue
            assert np.allclose(got[:3], dr, atol=1e-5), (u1, u2, got, dr)
            assert abs(got[3] - pr) <= 1e-4 * pr
            checked += 1
        assert checked > 3500
        assert c.env(img, (2.0, 1.0, 0.5)) == 0                  # a second upload: the same bits
        assert np.array_equal(c.hook(1, d).view(np.uint32), pdf[:, None].view(np.uint32))
    finally:
        c.close()


# ---- 2. a black map changes nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [IEEE, FAST])
def test_black_map_changes_no_bit(math):
    c = Ctx.box(math=math)
    L = c.L
    try:
        p = make_params(160, 96, 8, 8, True, True)
        ref, st0 = c.render(p)
        assert st0.variant == DEFAULT
        for v in (ENV, ENV_DEEP):
            assert L.pt_set_tuning(c.ctx, 0, v) == 0
            img, st = c.render(p)                                # no map: an ENV row sees a black one
            assert st.variant == v
            assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), v
            assert (st.radiance_rays, st.shadow_rays, st.paths) == (st0.radiance_rays, st0.shadow_rays, st0.paths)
        assert L.pt_set_tuning(c.ctx, 0, -1) == 0
        assert c.env(np.zeros((8, 16, 3), np.float32)) == 0
        img, st = c.render(p)
        assert st.variant == ENV and np.array_equal(img.view(np.uint32), ref.view(np.uint32))
        assert (st.radiance_rays, st.shadow_rays, st.paths) == (st0.radiance_rays, st0.shadow_rays, st0.paths)
        assert L.pt_set_light_mode(c.ctx, 1) == 0
        lit, stl = c.render(p)
        assert stl.variant == LIGHTS_ENV
        assert c.env(None) == 0
        lit0, stl0 = c.render(p)
        assert stl0.variant == LIGHTS
        assert np.array_equal(lit.view(np.uint32), lit0.view(np.uint32))
        assert (stl.radiance_rays, stl.shadow_rays) == (stl0.radiance_rays, stl0.shadow_rays)
        assert L.pt_set_light_mode(c.ctx, 0) == 0
        img, st = c.render(p)                                    # cleared: today's kernel and bits
        assert st.variant == DEFAULT and np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    finally:
        c.close()


# ---- 3. a constant map is what a camera facing away sees --------------------------------------------------------------------------
def constant_map_is_seen_exactly(classes, light, shape=(4, 8)):
    """the test below for a map of `shape` (h, w); tests/test_gpu_env_wide.py runs it with a map wider than the scan's workgroup"""
    c = Ctx.box(light=light)
    try:
        assert c.L.pt_debug_pixel_classes(c.ctx, classes) == 0
        col = np.array([0.25, 1.5, 3.0], np.float32)
        assert c.env(np.broadcast_to(col, shape + (3,))) == 0
        p = make_params(96, 64, 8, 6, True, True)
        W = p.cameraW
        p.cameraW = _native.Float3(-W.x, -W.y, -W.z)             # looking away from the box
        img, st = c.render(p, frames=2)
        assert st.variant == (LIGHTS_ENV if light else ENV)
        got = img[..., :3].reshape(-1, 3)
        ulp = np.spacing(col)
        assert np.all(np.abs(got - col) <= ulp), np.abs(got - col).max(axis=0)
        assert st.culled_rays == 96 * 64 * 8
    finally:
        c.close()


@pytest.mark.parametrize("classes", [1, 0])
@pytest.mark.parametrize("light", [0, 1])
def test_constant_map_is_seen_exactly(classes, light):
    constant_map_is_seen_exactly(classes, light)


# ---- 4. furnace ------------------------------------------------------------------------------------------------------------------
def _sphere_mask(c, p):
    """pixels the sphere covers entirely: black under a white map with kd = 0"""
    m = _native.Material()
    m.diffuse = _native.Float3(0.0, 0.0, 0.0); m.ior = 1.5
    t = (_native.Material * 1)(m)
    info = _native.UpdateInfo()
    assert c.L.pt_update_materials(c.ctx, C.addressof(t), 1, None, 0, C.byref(info)) == 0, c.err()
    img, _ = c.render(p)
    assert c.L.pt_update_materials(c.ctx, C.addressof(c.mats), 1, None, 0, C.byref(info)) == 0, c.err()
    return np.all(img[..., :3] == 0.0, axis=-1)


def furnace(light, dl, is_, shape=(16, 32)):
    """the test below under a white map of `shape` (h, w)"""
    c = Ctx.sphere(light=light)
    try:
        assert c.env(np.ones(shape + (3,), np.float32)) == 0
        p = _sphere_params(spp=64, depth=8, dl=dl, is_=is_)
        mask = _sphere_mask(c, p)
        assert mask.sum() > 800
        img, _ = c.render(p, frames=4)
        v = img[..., 1][mask]
        sigma = v.std() / np.sqrt(v.size)
        assert abs(v.mean() - 0.5) < 3 * sigma + 1e-4, (v.mean(), sigma)
        bg = img[..., :3][~mask & np.all(img[..., :3] == 1.0, axis=-1)]
        assert bg.size > 0
    finally:
        c.close()


@pytest.mark.parametrize("light,dl,is_", [(0, False, True), (0, False, False), (0, True, True), (1, True, True), (1, False, True), (1, True, False), (1, False, False)])
def test_furnace(light, dl, is_):
    furnace(light, dl, is_)


# ---- 5. MIS: light sampling of the map and BSDF sampling converge to the same image -------------------------------------------------
def test_map_light_sampling_agrees_with_bsdf_sampling_and_wins():
    runs = {}
    for key, light, dl, spp, frames in (("ref", 1, True, 256, 8), ("dl", 1, True, 64, 1), ("dl2", 1, True, 64, 1), ("nodl", 1, False, 64, 1),
                                        ("nodl2", 1, False, 64, 1), ("mode0", 0, False, 64, 1), ("mode0_2", 0, False, 64, 1)):
        c = Ctx.sphere(light=light)
        try:
            assert c.env(_sun_sky()) == 0
            p = _sphere_params(spp=spp, depth=6, dl=dl, is_=True)
            if key.endswith("2"):
                img, _ = c.render(p, frames=1, frame0=1000)     # other seeds: an independent render of the same configuration (frame 1000's blend weight is 1 / 1001)
                img = img * np.float32(1001.0)
            else:
                img, _ = c.render(p, frames=frames)
            runs[key] = img[..., :3].astype(np.float64)
        finally:
            c.close()
    ref = runs["ref"]
    mse = {k: float(((runs[k] - ref) ** 2).mean()) for k in ("dl", "nodl", "mode0")}
    noise = {k: float(((runs[k] - runs[k + ("2" if k != "mode0" else "_2")]) ** 2).mean()) / 2 for k in ("dl", "nodl", "mode0")}
    for k in mse:        # bias-free: the error against the converged image is the estimator's own noise (plus the reference's)
        assert mse[k] < 1.5 * noise[k] + mse["dl"] * 0.5, (k, mse, noise)
    print("env MIS: MSE at 64 spp against 2048 spp:", mse, "DL off / DL on = %.1f" % (mse["nodl"] / mse["dl"]))
    assert mse["nodl"] > 4 * mse["dl"], mse


# ---- 6. frame batches and partitions -------------------------------------------------------------------------------------------
def batches_and_partitions_with_a_map(light, img):
    """the test below with the map img"""
    c = Ctx.box(light=light)
    try:
        assert c.env(img) == 0
        p = make_params(96, 64, 8, 6, True, True)
        single, _ = c.render(p, frames=3)
        batch, _ = c.render(p, frames=3, batch=True)
        assert np.array_equal(single.view(np.uint32), batch.view(np.uint32))
        whole, _ = c.render(p, frames=1)
        parts = np.zeros_like(whole)
        for rank in range(3):
            assert c.L.pt_set_partition(c.ctx, rank, 3) == 0
            img, _ = c.render(p, frames=1)
            parts += img
        assert c.L.pt_set_partition(c.ctx, 0, 1) == 0
        assert np.array_equal(parts[..., :3].view(np.uint32), whole[..., :3].view(np.uint32))
    finally:
        c.close()


@pytest.mark.parametrize("light", [0, 1])
def test_batches_and_partitions_with_a_map(light):
    batches_and_partitions_with_a_map(light, _sky())


# ---- 7. refusals keep the previous map; the map outlives a scene change -------------------------------------------------------------
def test_refusals_keep_the_previous_map():
    c = Ctx.box()
    try:
        img = _sky()
        assert c.env(img) == 0
        d = sphere_directions(500, 3)
        before = c.hook(0, d)
        bad = []
        nan = img.copy(); nan[1, 2, 0] = np.nan; bad.append((nan, (1, 1, 1)))
        inf = img.copy(); inf[0, 0, 2] = np.inf; bad.append((inf, (1, 1, 1)))
        neg = img.copy(); neg[5, 5, 1] = -1e-3; bad.append((neg, (1, 1, 1)))
        bad.append((img, (1.0, -1.0, 1.0)))
        big = img.copy(); big[7, 9] = 10.0; bad.append((big, (1e38, 1e38, 1e38)))     # overflows to infinity after the scale
        for im, sc in bad:
            assert c.env(im, sc) != 0 and b"pt_set_environment" in c.err()
        f = np.ones((1, 16385, 3), np.float32)
        assert c.env(f) != 0
        assert c.L.pt_set_environment(c.ctx, img.ctypes.data, 8192, 8192, _native.Float3(1, 1, 1)) != 0     # 2^26 texels
        assert np.array_equal(c.hook(0, d).view(np.uint32), before.view(np.uint32))
        assert c.L.pt_set_scene(c.ctx, c.verts.ctypes.data, c.verts.size // 4, c.idx.ctypes.data, c.idx.size // 3,
                                c.mid.ctypes.data, C.addressof(c.mats), len(c.mats)) == 0
        assert np.array_equal(c.hook(0, d).view(np.uint32), before.view(np.uint32))
        p = make_params(32, 32, 4, 4, True, True)
        _, st = c.render(p)
        assert st.variant == ENV
    finally:
        c.close()


def test_python_api_and_cli_take_a_file(tmp_path):
    fix = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env", "rle.hdr")
    state, _ = pt.setup(BOX, width=64, height=48, max_depth=4, direct_lighting=True, importance_sampling=True, spp=4)
    try:
        pt.setEnvironment(state, fix, scale=2.0)
        pt.LaunchCurrentFrame(None, state)
        assert pt.getStats(state).variant == ENV
        pt.setEnvironment(state, None)
        pt.LaunchCurrentFrame(None, state)
        assert pt.getStats(state).variant == DEFAULT
    finally:
        pt.CleanAllTheThings(state)
    import subprocess
    exe = os.path.join(os.path.dirname(pt.__file__), "acgpt_main")
    out = tmp_path / "f.ppm"
    r = subprocess.run([exe, "--obj", BOX, "--width", "64", "--height", "48", "--frames", "1", "--spp-per-launch", "4", "--env", fix,
                        "--env-scale", "2", "--no-area-light", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Environment map" in r.stdout and out.exists()
