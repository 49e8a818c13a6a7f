"""Temporal reprojection without a GPU: the library exports and binds pt_temporal_blend and refuses a null context, the blend as
include/acgpt.h defines it (tests/temporal_ref.py) has the properties the definition promises, and it is calibrated on the CPU oracle.

Calibration (test_reference_blend_on_the_oracle): the oracle's Cornell box at 128 x 128, maxDepth 8, direct lighting and importance
sampling.  History: one 256-spp launch at the reference's camera.  Current: one 8-spp launch at the camera of acgpt_main --orbit 20,0
(10 degrees about the look-at point).  Features from the oracle's own closest hits through the pixel centres.  Truth:
tests/golden/temporal_cornell_128.npz (8192 spp at the orbited camera, tests/golden/make_temporal_golden.py).  Measured with the
default cap (256) and 5 denoising iterations:
    MSE(8 spp, ref)             = 1.92e-2
    MSE(blend, ref)             = 3.75e-3     -> F_BLEND = 5.1 (the factor the blend cuts the MSE by)
    MSE(denoise(blend), ref)    = 1.54e-3     -> 12.4   (denoise(8 spp) alone: 2.69e-3, 7.1)
    reprojection bias: MSE(blend of the two 8192-spp goldens, ref) = 4.7e-7 = 2.5e-5 of MSE(8 spp)
    pixels that take history    = 76.6 % of the image (13.2 % miss the scene, 6.1 % are metal or glass, the rest are disoccluded
                                  or leave the previous image)
Cap sweep, same inputs: 16 -> 2.5x, 32 -> 3.6x, 64 -> 4.6x, 128 -> 5.0x, 256 and above -> 5.1x (the history holds 256 samples).
With a converged history (the 8192-spp golden of the unmoved camera) instead: 96 -> 6.05x, 128 -> 6.19x, 192 -> 6.22x, 256 -> 6.17x,
512 -> 6.03x, 4096 -> 5.86x: past ~200 samples the blur of the bilinear resampling costs more than the extra weight gains.  256 is
best or within 1 % of it in both.  tests/test_gpu_temporal.py sets its thresholds from these numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import denoise_ref as dr
import temporal_ref as tr
from scene_utils import copy_params, image_mse, make_params

HERE = os.path.dirname(os.path.abspath(__file__))
BOX = os.path.join(pt.SCENES, "cornell_box.obj")
F_BLEND = 5.1               # MSE(8 spp, ref) / MSE(blend, ref), docstring above
F_BLEND_DENOISED = 12.4     # MSE(8 spp, ref) / MSE(denoise(blend), ref)
TOOK_MEASURED = 0.766       # share of the pixels that take history
BIAS_MEASURED = 2.5e-5      # MSE(blend of the two goldens, ref) / MSE(8 spp, ref)


@pytest.fixture(scope="module")
def lib():
    _build.build_hip()
    return _native.hip()


def test_library_exports_and_binds_the_blend(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.hip_library_path()], capture_output=True, text=True, check=True).stdout
    assert "pt_temporal_blend" in set(re.findall(r" T (pt_[a-z_]+)", out))
    assert "pt_temporal_blend" in _native.ABI_SYMBOLS
    assert lib.pt_temporal_blend.restype is C.c_int and len(lib.pt_temporal_blend.argtypes) == 11
    assert callable(pt.TemporalHistory) and pt.TEMPORAL_HISTORY_CAP == 256.0


def test_default_cap_is_the_header_constant():
    with open(os.path.join(os.path.dirname(HERE), "include", "acgpt.h")) as fh:
        m = re.search(r"#define PT_TEMPORAL_HISTORY_CAP ([0-9.]+)f", fh.read())
    assert m and float(m.group(1)) == pt.TEMPORAL_HISTORY_CAP


def test_null_context_is_refused_with_a_message(lib):
    assert lib.pt_temporal_blend(None, None, 8, None, None, None, None, None, None, 256.0, None) != 0
    assert b"pt_temporal_blend" in lib.pt_last_error(None)


# ---- the reference's properties ------------------------------------------------------------------------------------------------
class _Views:
    """Features of the reference camera and of --orbit 20,0 from the oracle's closest hits."""

    def __init__(self, oracle, size=(128, 96), orbit=(20, 0), prev_size=None):
        self.obj = pt.TinyObjWrapper(BOX)
        obj = self.obj
        self.sc = oracle.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
        self.diffuse = np.array([[m.diffuse.x, m.diffuse.y, m.diffuse.z] for m in obj.getMaterials()], np.float32)
        self.bsdf = tr.tri_bsdf(obj)
        self.size, self.prev_size = size, prev_size or size
        self.cam_prev = tr.orbit_camera(*self.prev_size, 0, 0)
        self.cam = tr.orbit_camera(*size, *orbit)
        self.alb_prev, self.nd_prev = self.features(self.prev_size, self.cam_prev)
        self.alb, self.nd = self.features(size, self.cam)

    def features(self, size, cam):
        w, h = size
        rays = dr.pixel_rays(w, h, *cam)
        t, prim = self.sc.trace_closest(rays, use_bvh=True)
        a, n = dr.features_from_hits(rays, t, prim, self.obj.getVerticesFloat(), self.obj.getIndexBuffer(), self.obj.getMaterialIndices(),
                                     self.diffuse)
        return a.reshape(h, w, 4), n.reshape(h, w, 4)

    def prev(self, hist):
        return (self.cam_prev, hist, self.alb_prev, self.nd_prev)


@pytest.fixture(scope="module")
def views(oracle):
    return _Views(oracle)


def _noise(shape, seed, w):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 2.0, size=shape[:2] + (4,)).astype(np.float32)
    a[..., 3] = w
    return a


def test_reference_pass_through_without_history_or_with_cap_zero(views):
    acc = _noise(views.nd.shape, 1, 1.0)
    hist = _noise(views.nd_prev.shape, 2, 512.0)
    for cap, prev in ((256.0, None), (0.0, views.prev(hist))):
        out, took = tr.blend(acc, views.alb, views.nd, views.cam, 24, views.bsdf, cap, prev)
        assert not took.any()
        assert np.array_equal(out[..., :3].view(np.uint32), acc[..., :3].view(np.uint32)) and np.all(out[..., 3] == 24)
    out, took = tr.blend(acc, views.alb, views.nd, views.cam, 24, views.bsdf, 256.0, views.prev(hist))
    assert 0.5 < took.mean() < 0.9


def test_reference_unmoved_camera_gives_the_sample_weighted_mean(views):
    """History and accumulation constant over each triangle, the camera unmoved: every pixel that takes history gets
    (n h + N c) / (n + N) with h and c its triangle's two colours, and nearly all hits take the whole footprint (n = cap)."""
    rng = np.random.default_rng(3)
    n_tris = views.bsdf.size
    col_h, col_c = rng.uniform(0.1, 1.0, (n_tris, 3)).astype(np.float32), rng.uniform(0.1, 1.0, (n_tris, 3)).astype(np.float32)
    hit = views.nd_prev[..., 3] >= 0
    prim = views.alb_prev[..., 3].view(np.uint32)
    hist = np.zeros(views.nd_prev.shape, np.float32)
    hist[hit, :3] = col_h[prim[hit]]
    hist[..., 3] = 100.0
    acc = np.zeros(views.nd_prev.shape, np.float32)
    acc[hit, :3] = col_c[prim[hit]]
    N, cap = 8, 64.0
    out, took = tr.blend(acc, views.alb_prev, views.nd_prev, views.cam_prev, N, views.bsdf, cap, views.prev(hist))
    diffuse = np.zeros(hit.shape, bool)
    diffuse[hit] = views.bsdf[prim[hit]] == 0
    assert np.array_equal(took, diffuse)             # unmoved: every diffuse hit finds itself
    n = out[took, 3] - N
    assert np.all(n > 0) and np.all(n <= cap) and (n == cap).mean() > 0.97
    want = (n[:, None] * col_h[prim[took]] + N * col_c[prim[took]]) / (n + N)[:, None]
    assert np.allclose(out[took, :3], want, rtol=1e-6, atol=0)


def test_reference_keeps_disoccluded_pixels_and_metal_and_glass_fresh(views):
    acc = _noise(views.nd.shape, 4, 1.0)
    hist = _noise(views.nd_prev.shape, 5, 256.0)
    N = 8
    out, took = tr.blend(acc, views.alb, views.nd, views.cam, N, views.bsdf, 256.0, views.prev(hist))
    h, w = views.nd.shape[:2]
    hit = views.nd[..., 3] >= 0
    prim = views.alb[..., 3].view(np.uint32)
    # metal and glass: never
    shiny = np.zeros(hit.shape, bool)
    shiny[hit] = views.bsdf[prim[hit]] != 0
    assert shiny.sum() > 100 and np.all(out[shiny, 3] == N)
    # hidden from the previous camera: the oracle's ray from eye' towards the hit point stops at another triangle first
    eye_p = np.asarray(views.cam_prev[0], np.float32)
    d = dr.pixel_rays(w, h, *views.cam)[:, 3:6].reshape(h, w, 3)
    P = np.asarray(views.cam[0], np.float32) + views.nd[..., 3:4] * d
    to = (P - eye_p).reshape(-1, 3)
    dist = np.linalg.norm(to, axis=1).astype(np.float32)
    rays = np.zeros((h * w, 8), np.float32)
    rays[:, 0:3] = eye_p
    rays[:, 3:6] = to / np.maximum(dist, 1e-6)[:, None]
    rays[:, 6], rays[:, 7] = 0.01, 1e16
    t, p2 = views.sc.trace_closest(rays, use_bvh=True)
    hidden = (hit & ~shiny).reshape(-1) & (p2 != prim.reshape(-1)) & (t >= 0) & (t < 0.99 * dist)
    hidden = hidden.reshape(h, w)
    assert hidden.sum() > 50
    # a hidden point takes history only where its triangle is visible at a tap of the footprint: at the rim of the occluder
    rim = np.zeros(hit.shape, bool)
    prim_p = views.alb_prev[..., 3].view(np.uint32)
    hp, wp = prim_p.shape
    ys, xs = np.nonzero(hidden & took)
    for y, x in zip(ys, xs):
        v = P[y, x] - eye_p
        U, V, W = (np.asarray(a, np.float64) for a in views.cam_prev[1:])
        s = v @ W / (W @ W)
        fx = (v @ U / (s * (U @ U)) + 1) * 0.5 * wp - 0.5
        fy = (v @ V / (s * (V @ V)) + 1) * 0.5 * hp - 0.5
        x0, y0 = int(np.floor(fx)), int(np.floor(fy))
        rim[y, x] = (prim_p[max(y0, 0):y0 + 2, max(x0, 0):x0 + 2] == prim[y, x]).any()
    assert np.all(rim[hidden & took])
    assert np.all(out[hidden & ~took, 3] == N) and (hidden & ~took).sum() >= 0.8 * hidden.sum()


def test_reference_history_of_another_size(oracle):
    """The previous view may have another size: an unmoved camera at 3/4 of the resolution still reprojects nearly every
    diffuse hit, and a history in one colour comes back in that colour."""
    v = _Views(oracle, size=(128, 96), orbit=(0, 0), prev_size=(96, 72))
    hist = np.zeros(v.nd_prev.shape, np.float32)
    hist[..., :3] = (0.25, 0.5, 0.75)
    hist[..., 3] = 64.0
    acc = np.zeros(v.nd.shape, np.float32)
    acc[..., 3] = 1.0
    out, took = tr.blend(acc, v.alb, v.nd, v.cam, 64, v.bsdf, 256.0, v.prev(hist))
    hit = v.nd[..., 3] >= 0
    prim = v.alb[..., 3].view(np.uint32)
    diffuse = np.zeros(hit.shape, bool)
    diffuse[hit] = v.bsdf[prim[hit]] == 0
    assert took.sum() > 0.95 * diffuse.sum() and not (took & ~diffuse).any()
    n = out[took, 3] - 64
    want = n[:, None] * np.float32([0.25, 0.5, 0.75]) / (n + 64)[:, None]
    assert np.allclose(out[took, :3], want, rtol=1e-6, atol=0)


# ---- calibration ---------------------------------------------------------------------------------------------------------------
def test_reference_blend_on_the_oracle(oracle):
    obj = pt.TinyObjWrapper(BOX)
    sc = oracle.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    gold = np.load(os.path.join(HERE, "golden", "temporal_cornell_128.npz"))
    gold0 = np.load(os.path.join(HERE, "golden", "denoise_cornell_128.npz"))
    size, _, depth, _, _, ox, oy = (int(v) for v in gold["meta"])
    assert (ox, oy) == (20, 0)
    one = np.ones((size, size, 1), np.float32)
    ref = np.concatenate([gold["ref"], one], axis=-1)
    ref0 = np.concatenate([gold0["ref"], one], axis=-1)
    diffuse = np.array([[m.diffuse.x, m.diffuse.y, m.diffuse.z] for m in obj.getMaterials()], np.float32)

    def features(p):
        rays = dr.pixel_rays(size, size, *tr.camera_of(p))
        t, prim = sc.trace_closest(rays, use_bvh=True)
        a, n = dr.features_from_hits(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), diffuse)
        return a.reshape(size, size, 4), n.reshape(size, size, 4)

    p0 = make_params(size, size, 256, depth, True, True)
    p1 = tr.set_camera(make_params(size, size, 8, depth, True, True), *tr.orbit_camera(size, size, ox, oy))
    hist, _, _, _ = sc.render(copy_params(p0))
    hist[..., 3] = 256.0
    noisy, _, _, _ = sc.render(copy_params(p1))
    a0, n0 = features(p0)
    a1, n1 = features(p1)
    bsdf = tr.tri_bsdf(obj)
    cam0, cam1 = tr.camera_of(p0), tr.camera_of(p1)
    cap = pt.TEMPORAL_HISTORY_CAP

    blended, took = tr.blend(noisy, a1, n1, cam1, 8, bsdf, cap, (cam0, hist, a0, n0))
    mse_noisy, mse_blend = image_mse(noisy, ref), image_mse(blended, ref)
    mse_dn = image_mse(dr.denoise(blended, a1, n1, 5), ref)
    mse_dn_noisy = image_mse(dr.denoise(noisy, a1, n1, 5), ref)
    g0 = ref0.copy()
    g0[..., 3] = 8192.0
    both, _ = tr.blend(ref, a1, n1, cam1, 8192, bsdf, cap, (cam0, g0, a0, n0))
    bias = image_mse(both, ref) / mse_noisy
    print("MSE 8 spp %.3e blend %.3e (F %.2f) denoise(blend) %.3e (%.2f) denoise(8 spp) %.3e; bias %.2e of 8 spp; %.3f take history"
          % (mse_noisy, mse_blend, mse_noisy / mse_blend, mse_dn, mse_noisy / mse_dn, mse_dn_noisy, bias, took.mean()))
    assert mse_noisy / mse_blend >= 0.9 * F_BLEND
    assert mse_noisy / mse_dn >= 0.9 * F_BLEND_DENOISED and mse_dn < mse_dn_noisy
    assert took.mean() >= 0.9 * TOOK_MEASURED
    assert bias <= 10 * BIAS_MEASURED
    # the cap is what decides the weight: a smaller one gives less
    small, _ = tr.blend(noisy, a1, n1, cam1, 8, bsdf, 32.0, (cam0, hist, a0, n0))
    assert image_mse(small, ref) > mse_blend
