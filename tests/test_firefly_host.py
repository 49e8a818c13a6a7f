"""The firefly filter without a GPU: the arithmetic of pt_firefly_filter as include/acgpt.h states it (tests/firefly_ref.py) is pinned
by its properties and calibrated on the CPU oracle; the library exports and binds the call.

Calibration (test_calibration_on_the_oracle; tools/firefly_sweep.py prints the whole table, DESIGN.md section 20 holds it): the
oracle's Cornell box at 128 x 128, maxDepth 8, direct lighting and importance sampling; the input is one 8-spp launch, repeated with
the frame indices 0 .. 7; the truth is tests/golden/denoise_cornell_128.npz (8192 spp); denoise_ref with 5 iterations as in
test_denoise_host.py.  With G = MSE(denoised) / MSE(filtered then denoised), over the 8 inputs:
    MSE(noisy) 2.039e-2 +- 3.4e-4    MSE(denoised) 3.193e-3 +- 2.7e-4 (8.4 %)
    ratio 16, rank 1, radius 1 (the defaults):  G = 1.000 1.006 1.004 1.037 1.033 1.008 1.010 1.020   mean 1.0146, spread 0.0140
No setting of the grid beats the denoiser alone by more than the spread of the denoised MSE over the 8 inputs (8.4 %): the best
is 1.5 %, and every ratio below 8 makes the result worse (ratio 2, rank 2, radius 1: G = 0.67), because the clamp takes energy the
denoiser would have spread, and the metric clamps to [0, 1] anyway.  The light-mode-1 microfacet twin says the same (best G = 1.053
+- 0.034 against a denoised MSE that spreads by 10 %; the defaults give 1.015 +- 0.018 there).  So the tests assert what the issue
asks for in that case: the filter with its defaults does not make the denoised result worse beyond the band,
    G >= 1 - CAL_BAND,   CAL_BAND = max(4 * spread, 0.1) = 0.1    (set as test_convergence_host.CAL_BAND was)
and the host test also holds G of frame index 0 to CAL_GAIN +- CAL_BAND.  The defaults cost the converged image nothing (no pixel of
the 8192-spp truth is clamped), against the denoiser's own 4.2 % of the noisy MSE."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import denoise_ref as dr
import firefly_ref as fr
from scene_utils import copy_params, image_mse, make_params

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CAL_GAIN, CAL_SPREAD = 1.0146, 0.0140               # measured, docstring above
CAL_BAND = max(4.0 * CAL_SPREAD, 0.1)
CAL_EDGE_LIMIT = 0.042                              # what the denoiser costs a converged image (test_denoise_host.EDGE_MEASURED)


@pytest.fixture(scope="module")
def lib():
    _build.build_hip()
    return _native.hip()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def flat(h, w, rgb=(0.25, 0.5, 0.125), alpha=1.0):
    img = np.zeros((h, w, 4), F)
    img[..., :3] = rgb
    img[..., 3] = alpha
    return img


# ---- symbol and ABI -----------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_call(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.hip_library_path()], capture_output=True, text=True, check=True).stdout
    assert "pt_firefly_filter" in set(re.findall(r" T (pt_[a-z_]+)", out))
    assert "pt_firefly_filter" in _native.ABI_SYMBOLS
    assert lib.pt_firefly_filter.restype is C.c_int and len(lib.pt_firefly_filter.argtypes) == 7
    assert lib.pt_abi_version() == 4 == _native.ABI_VERSION
    assert C.sizeof(_native.FireflyParams) == 16 and C.sizeof(_native.FireflyInfo) == 40
    assert _native.FireflyInfo.total_luma_q16.offset == 16 and _native.FireflyInfo.max_ratio.offset == 32
    assert callable(pt.fireflyFilter)
    assert {k: float(v) for k, v in pt.FIREFLY_DEFAULTS.items()} == {k: float(v) for k, v in fr.DEFAULTS.items()}


def test_null_context_is_refused_with_a_message(lib):
    assert lib.pt_firefly_filter(None, None, 1, 1, None, None, None) != 0
    assert b"pt_firefly_filter" in lib.pt_last_error(None)


def test_kernel_sources_do_not_include_the_filter():
    """the render kernels' source hash, the committed profiles and bench.py do not see this post-pass"""
    assert "firefly.hip" in _build.HIP_SOURCES and "firefly.hip" not in _build.KERNEL_SOURCES and "firefly.h" not in _build.KERNEL_SOURCES


# ---- the statement's properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", (1, 2))
@pytest.mark.parametrize("rank", (1, 2, 3, 4))
def test_a_constant_image_comes_back_as_bits(rank, radius):
    src = flat(9, 13)
    src[..., 3] = np.arange(9 * 13, dtype=F).reshape(9, 13)
    out, info = fr.filter(src, ratio=1.0, rank=rank, radius=radius)
    assert np.array_equal(bits(out), bits(src))
    assert (info["clamped_pixels"], info["replaced_pixels"], info["passed_pixels"]) == (0, 0, 9 * 13)
    assert info["removed_luma_q16"] == 0 and info["max_ratio"] == 0.0


def test_an_image_within_the_ratio_comes_back_as_bits():
    """a background over less than one octave: no pixel exceeds 2 x its brightest neighbour (nor, with radius 2, 4 x its fourth)"""
    rng = np.random.default_rng(1)
    src = np.exp2(rng.uniform(0.0, 0.99, (33, 47, 4))).astype(F)
    for kw in (dict(ratio=2.0, rank=1, radius=1), dict(ratio=2.0, rank=4, radius=2), dict(ratio=2.0, rank=4, radius=1)):
        out, info = fr.filter(src, **kw)
        assert np.array_equal(bits(out), bits(src)), kw
        assert info["passed_pixels"] == 33 * 47 and info["clamped_pixels"] == 0


@pytest.mark.parametrize("radius", (1, 2))
def test_a_single_spike_is_clamped_to_ratio_times_the_background(radius):
    src = flat(11, 11, rgb=(0.5, 0.5, 0.5))
    src[5, 6, :3] = (4096.0, 2048.0, 1024.0)
    out, info = fr.filter(src, ratio=4.0, rank=1, radius=radius)
    want = src.copy()
    lb, ls = fr.lum(src[0, 0]), fr.lum(src[5, 6])
    t = F(4.0) * lb
    want[5, 6, :3] = src[5, 6, :3] * (t / ls)
    assert np.array_equal(bits(out), bits(want))
    assert abs(float(fr.lum(out[5, 6])) - 4.0 * float(lb)) <= 4.0 * float(lb) * 2.0 ** -22       # three roundings from the limit
    assert info["clamped_pixels"] == 1 and info["passed_pixels"] == 120 and info["replaced_pixels"] == 0
    assert F(info["max_ratio"]).view(np.uint32) == (ls / t).view(np.uint32)
    assert info["removed_luma_q16"] == int(float(ls - t) * 65536.0)
    # the floor: a black background limits the spike to ratio * floor
    src[..., :3] = 0
    src[5, 6, :3] = 1.0
    out, info = fr.filter(src, ratio=4.0, rank=1, radius=radius, floor=0.01)
    assert info["clamped_pixels"] == 1
    assert abs(float(fr.lum(out[5, 6])) - 0.04) < 1e-7


def test_two_adjacent_spikes_survive_rank_one_and_fall_to_rank_two():
    src = flat(9, 9, rgb=(0.5, 0.5, 0.5))
    src[4, 4, :3] = 100.0
    src[4, 5, :3] = 100.0
    out, info = fr.filter(src, ratio=4.0, rank=1, radius=1)
    assert np.array_equal(bits(out), bits(src)) and info["clamped_pixels"] == 0
    out, info = fr.filter(src, ratio=4.0, rank=2, radius=1)
    assert info["clamped_pixels"] == 2
    assert np.allclose(fr.lum(out[4, 4:6]), 2.0, rtol=1e-6)
    mask = np.ones((9, 9), bool); mask[4, 4:6] = False
    assert np.array_equal(bits(out)[mask], bits(src)[mask])
    # multiplicity: two equal brightest neighbours are ranks 1 and 2
    src[3, 4, :3] = 100.0
    out, info = fr.filter(src, ratio=4.0, rank=2, radius=1)
    assert info["clamped_pixels"] == 0 and np.array_equal(bits(out), bits(src))


def synthetic(h, w, seed, spikes=0.01, specials=0.03):
    """a log-uniform background over three octaves, about 1 % spikes of 2^4 .. 2^12 times it (every fourth with a spiked right-hand
    neighbour), about 3 % special pixels (0, NaN, +-inf, negatives, values near FLT_MAX), and a NaN with a payload in .w"""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-2.0, 1.0, (h, w, 4))).astype(F)
    n = h * w
    px = img.reshape(n, 4)
    spike = np.flatnonzero(rng.random(n) < spikes)
    if n >= 9 and spike.size == 0:
        spike = np.array([n // 2])
    pair = spike[::4] + 1
    spike = np.unique(np.concatenate([spike, pair[pair < n]]))
    px[spike, :3] *= np.exp2(rng.uniform(4.0, 12.0, (spike.size, 1))).astype(F)
    special = np.array([0.0, 0.0, np.nan, np.inf, -np.inf, -1.0, -300.0, 3.0e38, 3.4e38, -3.4e38], F)
    pick = np.flatnonzero(rng.random(n) < specials)
    if n <= 64:
        pick = np.union1d(pick, np.arange(0, n, 3))
    vals = special[rng.integers(0, len(special), pick.size)]
    grey = rng.random(pick.size) < 0.5
    px[pick[grey], :3] = vals[grey, None]
    px[pick[~grey], rng.integers(0, 3, int((~grey).sum()))] = vals[~grey]
    w_bits = (np.uint32(0x7FC00000) | (np.arange(n, dtype=np.uint32) & np.uint32(0x3FFFFF)))
    w_bits[::7] |= np.uint32(0x80000000)
    px.view(np.uint32)[:, 3] = w_bits
    return img


@pytest.mark.parametrize("radius", (1, 2))
@pytest.mark.parametrize("rank", (1, 2, 4))
def test_properties_on_a_spiked_image(rank, radius):
    src = synthetic(37, 53, 11 + rank)
    out, info = fr.filter(src, ratio=3.0, rank=rank, radius=radius)
    n = 37 * 53
    l, lo = fr.lum(src), fr.lum(out)
    ok = fr.valid(l)
    assert info["clamped_pixels"] > 0 and info["replaced_pixels"] > 0 and info["passed_pixels"] > 0
    assert info["clamped_pixels"] + info["replaced_pixels"] + info["passed_pixels"] == n
    assert info["replaced_pixels"] == int((~ok).sum())
    # a valid pixel never gains luminance, and one that changed was scaled down as a whole
    assert np.all(lo[ok] <= l[ok] * F(1.0 + 2.0 ** -22))
    changed = ok & np.any(bits(out)[..., :3] != bits(src)[..., :3], axis=-1)
    assert int(changed.sum()) <= info["clamped_pixels"]
    # .w passes as bits, NaN payloads and signs included
    assert np.array_equal(bits(out)[..., 3], bits(src)[..., 3])
    # every output colour is finite or comes from an overflowing sum of finite neighbours; no NaN is left
    assert not np.isnan(out[..., :3]).any()
    # the q16 sums against Python integers
    t = ok & ~changed
    total = sum(int(min(float(v), 2.0 ** 24) * 65536.0) for v in l[ok].ravel())
    assert info["total_luma_q16"] == total
    removed = 0
    worst = 0.0
    for y, x in zip(*np.nonzero(ok)):
        nb = []
        for dx, dy in fr.taps(radius):
            qy, qx = y + dy, x + dx
            if 0 <= qy < 37 and 0 <= qx < 53 and ok[qy, qx]:
                nb.append(l[qy, qx])
        if len(nb) < rank:
            continue
        with np.errstate(over="ignore"):
            lim = F(3.0) * max(sorted(nb, reverse=True)[rank - 1], F(0.01))
        if l[y, x] > lim:
            removed += int(min(float(l[y, x] - lim), 2.0 ** 24) * 65536.0)
            worst = max(worst, float(l[y, x] / lim))
    assert info["removed_luma_q16"] == removed
    assert info["max_ratio"] == worst
    assert 0.0 < fr.removed_share(info) < 1.0


def test_small_images_pass_where_the_rank_is_out_of_reach():
    for (h, w), radius in (((1, 1), 1), ((1, 1), 2), ((2, 1), 1), ((1, 2), 2), ((2, 2), 1), ((2, 2), 2)):
        src = np.exp2(np.arange(h * w * 4, dtype=F).reshape(h, w, 4) * F(3.0))      # each pixel far above the one before
        for rank in (1, 2, 3, 4):
            out, info = fr.filter(src, ratio=1.0, rank=rank, radius=radius)
            if h * w - 1 < rank:
                assert np.array_equal(bits(out), bits(src)), (h, w, rank)
                assert info["passed_pixels"] == h * w == info["passed_undefined"]
            else:
                assert info["clamped_pixels"] >= 1, (h, w, rank)


def test_invalid_pixels_are_replaced_by_the_mean_of_their_valid_neighbours():
    src = flat(5, 5, rgb=(1.0, 2.0, 3.0))
    src[..., 0] += np.arange(25, dtype=F).reshape(5, 5)
    bad = {(2, 2): (np.nan, 1, 1), (0, 0): (np.inf, 0, 0), (4, 4): (-np.inf, 0, 0), (2, 3): (-1.0, -1.0, -1.0), (0, 4): (-3.4e38, -3.4e38, 3.4e38)}
    for (y, x), v in bad.items():
        src[y, x, :3] = v
    src[1, 1, :3] = (0.0, 0.0, 0.0)           # zero is valid
    out, info = fr.filter(src, ratio=1e6, rank=1, radius=1)
    assert info["replaced_pixels"] == len(bad) and info["clamped_pixels"] == 0
    for (y, x) in bad:
        acc, n = np.zeros(3, F), 0
        for dx, dy in fr.taps(1):
            qy, qx = y + dy, x + dx
            if 0 <= qy < 5 and 0 <= qx < 5 and (qy, qx) not in bad:
                acc = acc + src[qy, qx, :3]
                n += 1
        assert n > 0 and np.array_equal(bits(out[y, x, :3]), bits(acc / F(n))), (y, x)
    good = np.ones((5, 5), bool)
    for k in bad:
        good[k] = False
    assert np.array_equal(bits(out)[good], bits(src)[good])
    # no valid neighbour: zero; .w stays
    src = np.full((2, 2, 4), np.nan, F)
    src[..., 3] = 7.0
    out, info = fr.filter(src, ratio=2.0, rank=1, radius=2)
    assert info["replaced_pixels"] == 4 and np.all(bits(out)[..., :3] == 0) and np.all(out[..., 3] == 7.0)
    # overflow: the weights of l sum to one, so finite channels near FLT_MAX still give a finite, valid luminance, and the pixel passes;
    # the sum over such neighbours overflows, and the replacement is the infinity the stated arithmetic gives
    src = flat(3, 3, rgb=(3.0e38, 3.0e38, 3.0e38))
    src[1, 1, :3] = np.nan
    out, info = fr.filter(src, ratio=2.0, rank=1, radius=1)
    assert info["replaced_pixels"] == 1 and info["passed_pixels"] == 8 and np.all(np.isposinf(out[1, 1, :3]))
    mx = np.finfo(F).max
    src = flat(3, 3, rgb=(mx, mx, mx))
    l = fr.lum(src[0, 0])
    out, info = fr.filter(src, ratio=2.0, rank=1, radius=1)
    assert info["replaced_pixels"] == (0 if np.isfinite(l) else 9)


def test_the_record_as_words():
    src = synthetic(20, 20, 5)
    _, info = fr.filter(src, ratio=2.0, rank=1, radius=1)
    rec = fr.info_bits(info)
    assert rec.dtype == np.uint32 and rec.size == 10
    assert int(rec[4]) | (int(rec[5]) << 32) == info["total_luma_q16"] and int(rec[6]) | (int(rec[7]) << 32) == info["removed_luma_q16"]


# ---- calibration on real noise ------------------------------------------------------------------------------------------------
def test_calibration_on_the_oracle(oracle):
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj"))
    sc = oracle.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    gold = np.load(os.path.join(HERE, "golden", "denoise_cornell_128.npz"))
    size, _, depth, _, _ = (int(v) for v in gold["meta"])
    ref = np.concatenate([gold["ref"], np.ones((size, size, 1), F)], axis=-1)
    p = make_params(size, size, 8, depth, True, True)
    noisy, _, _, _ = sc.render(copy_params(p))
    noisy = noisy.reshape(size, size, 4)
    rays = dr.pixel_rays(size, size, p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple())
    t, prim = sc.trace_closest(rays, use_bvh=True)
    diffuse = np.array([[m.diffuse.x, m.diffuse.y, m.diffuse.z] for m in obj.getMaterials()], F)
    alb, nd = dr.features_from_hits(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), diffuse)
    alb, nd = alb.reshape(size, size, 4), nd.reshape(size, size, 4)

    filtered, info = fr.filter(noisy)                           # the defaults
    mse_noisy, mse_f = image_mse(noisy, ref), image_mse(filtered, ref)
    mse_dn = image_mse(dr.denoise(noisy, alb, nd, 5), ref)
    mse_fdn = image_mse(dr.denoise(filtered, alb, nd, 5), ref)
    gain = mse_dn / mse_fdn
    edge, edge_info = fr.filter(ref)
    cost = image_mse(edge, ref) / mse_noisy
    print("MSE noisy %.3e filtered %.3e denoised %.3e filtered+denoised %.3e: G %.4f; clamped %d, removed share %.4f; on the truth: cost %.5f of noisy, removed %.5f"
          % (mse_noisy, mse_f, mse_dn, mse_fdn, gain, info["clamped_pixels"], fr.removed_share(info), cost, fr.removed_share(edge_info)))
    assert info["clamped_pixels"] > 0 and mse_f < mse_noisy
    assert gain >= 1.0 - CAL_BAND
    assert abs(gain - CAL_GAIN) <= CAL_BAND
    assert cost < CAL_EDGE_LIMIT and fr.removed_share(edge_info) < 0.01
