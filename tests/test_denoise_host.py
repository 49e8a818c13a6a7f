"""The denoised preview without a GPU: the library exports and binds pt_render_features / pt_denoise and refuses a null context, and
the filter as include/acgpt.h defines it (tests/denoise_ref.py) is calibrated on the CPU oracle.

Calibration (test_reference_filter_on_the_oracle): the oracle's Cornell box at 128 x 128, maxDepth 8, direct lighting and importance
sampling, one 8-spp launch; features from the oracle's own closest hits through the pixel centres; the converged image is
tests/golden/denoise_cornell_128.npz (8192 spp, tests/golden/make_denoise_golden.py).  Measured with the constants of acgpt.h
(sigma_z 0.01, sigma_n 128, sigma_l 5) and 5 iterations:
    MSE(noisy, ref)        = 2.03e-2
    MSE(denoised, ref)     = 2.89e-3      -> F = 7.0 (the factor the filter cuts the MSE by)
    MSE(denoise(ref), ref) = 8.5e-4       =  0.042 * MSE(noisy, ref)   (what the filter costs a converged image)
tests/test_gpu_denoise.py sets its thresholds from these two numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import denoise_ref as dr
from scene_utils import copy_params, image_mse, make_params

HERE = os.path.dirname(os.path.abspath(__file__))
F_MEASURED = 7.0            # MSE(noisy, ref) / MSE(denoised, ref), docstring above
EDGE_MEASURED = 0.042       # MSE(denoise(ref), ref) / MSE(noisy, ref)


@pytest.fixture(scope="module")
def lib():
    _build.build_hip()
    return _native.hip()


def test_library_exports_and_binds_the_denoiser(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.hip_library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pt_[a-z_]+)", out))
    for name in ("pt_render_features", "pt_denoise"):
        assert name in exported
        assert name in _native.ABI_SYMBOLS
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes is not None
    assert callable(pt.renderFeatures) and callable(pt.denoise)


def test_null_context_is_refused_with_a_message(lib):
    assert lib.pt_denoise(None, None, None, None, None, 5) != 0
    assert b"pt_denoise" in lib.pt_last_error(None)
    assert lib.pt_render_features(None, None, None, None) != 0
    assert b"pt_render_features" in lib.pt_last_error(None)


def test_reference_filter_keeps_a_flat_image(built):
    """A constant colour on one plane at one depth passes through unchanged (every weight is positive, the mean is the colour)."""
    h, w = 24, 40
    acc = np.zeros((h, w, 4), np.float32); acc[..., :3] = (0.25, 0.5, 0.125); acc[..., 3] = 1
    alb = np.zeros((h, w, 4), np.float32); alb[..., :3] = 0.5
    nd = np.zeros((h, w, 4), np.float32); nd[..., 2] = 1.0; nd[..., 3] = 100.0
    out = dr.denoise(acc, alb, nd, 5)
    assert np.allclose(out[..., :3], acc[..., :3], rtol=1e-6, atol=0) and np.all(out[..., 3] == 1)


def test_reference_filter_on_the_oracle(oracle):
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj"))
    sc = oracle.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    gold = np.load(os.path.join(HERE, "golden", "denoise_cornell_128.npz"))
    size, _, depth, _, _ = (int(v) for v in gold["meta"])
    ref = np.concatenate([gold["ref"], np.ones((size, size, 1), np.float32)], axis=-1)
    p = make_params(size, size, 8, depth, True, True)
    noisy, _, _, _ = sc.render(copy_params(p))
    rays = dr.pixel_rays(size, size, p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple())
    t, prim = sc.trace_closest(rays, use_bvh=True)
    diffuse = np.array([[m.diffuse.x, m.diffuse.y, m.diffuse.z] for m in obj.getMaterials()], np.float32)
    alb, nd = dr.features_from_hits(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), diffuse)
    alb, nd = alb.reshape(size, size, 4), nd.reshape(size, size, 4)
    assert 0.9 < (prim != 0xFFFFFFFF).mean() < 1.0

    mse_noisy = image_mse(noisy, ref)
    mse_dn = image_mse(dr.denoise(noisy, alb, nd, 5), ref)
    mse_edge = image_mse(dr.denoise(ref, alb, nd, 5), ref)
    print("MSE noisy %.3e denoised %.3e (F %.2f) denoise(ref) %.3e (%.3f of noisy)" % (mse_noisy, mse_dn, mse_noisy / mse_dn, mse_edge, mse_edge / mse_noisy))
    assert mse_noisy / mse_dn >= 0.9 * F_MEASURED
    assert mse_edge <= 1.2 * EDGE_MEASURED * mse_noisy
    # more iterations reach further: each of the first three lowers the error
    errs = [image_mse(dr.denoise(noisy, alb, nd, i), ref) for i in (1, 2, 3)]
    assert errs[0] < mse_noisy and errs[1] < errs[0] and errs[2] < errs[1]
