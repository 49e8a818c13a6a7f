"""The convergence estimate without a GPU: the arithmetic of pt_convergence_update as include/acgpt.h states it
(tests/convergence_ref.py) is unbiased on synthetic data, handles restarts and invalid pixels, reduces to the right quantile, and is
calibrated on the CPU oracle's noise; the library exports and binds the call.

Calibration (test_calibration_on_the_oracle): the oracle's Cornell box at 48 x 48, maxDepth 4, direct lighting and importance
sampling, 16 spp per frame.  256 frames with the frame indices 0 .. 255 (256 seed sets) are rendered one by one; their float64 mean
is the reference image A_ref (K_ref = 256).  Run r = 0 .. 7 accumulates the frames 16 r .. 16 r + 15 as fp32 running means, the
statement is fed after each of them, and
    R = sum (l(A_16) - l(A_ref))^2 / sum v      over the measured pixels with l(A_16) > lum_floor
is the ratio of the error the image really has to the error the estimate claims.  A_16 is part of A_ref, so the expected value is
1 - 16 / 256 = 0.9375.  Measured over the 8 runs (printed by the test):
    R = 1.033 0.751 0.756 0.739 0.722 0.871 0.882 0.792      mean 0.8181, spread (sample standard deviation) 0.1055
so the band is mean +- max(4 * spread, 0.1) = 0.818 +- 0.422.  Both sums are dominated by the few pixels that caught a bright path,
which makes R heavy-tailed: the mean of 8 runs is itself only good to 0.1055 / sqrt(8) = 0.037.  Over more seed sets it moves to
the expected value (16 runs inside the same 256 frames: 0.866 +- 0.034; 32 runs inside 512 frames: 0.947 +- 0.037 against
0.969), so the 13 % these 8 runs lie below 0.9375 is their sampling error, not a bias of the estimate (which the synthetic test
bounds to 0.3 %).  tests/test_gpu_convergence.py moves the band to its own K_ref."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import convergence_ref as cr
from scene_utils import copy_params, make_params

F = np.float32
CAL_FRAMES, CAL_KREF, CAL_RUNS = 16, 256, 8
CAL_EXPECTED = 1.0 - CAL_FRAMES / CAL_KREF
CAL_MEAN, CAL_SPREAD = 0.8181, 0.1055              # measured, docstring above
CAL_BAND = max(4.0 * CAL_SPREAD, 0.1)


@pytest.fixture(scope="module")
def lib():
    _build.build_hip()
    return _native.hip()


# ---- symbol and ABI -----------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_call(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.hip_library_path()], capture_output=True, text=True, check=True).stdout
    assert "pt_convergence_update" in set(re.findall(r" T (pt_[a-z_]+)", out))
    assert "pt_convergence_update" in _native.ABI_SYMBOLS
    assert lib.pt_convergence_update.restype is C.c_int and len(lib.pt_convergence_update.argtypes) == 8
    assert lib.pt_abi_version() == 4 == _native.ABI_VERSION
    assert C.sizeof(_native.ConvergenceParams) == 16 and C.sizeof(_native.ConvergenceInfo) == 32 + 4 * 256
    assert (_native.CONVERGENCE_BINS, _native.CONVERGENCE_TILE) == (cr.BINS, cr.TILE) == (256, 16)
    assert callable(pt.renderUntil) and callable(pt.Convergence)


def test_null_context_is_refused_with_a_message(lib):
    assert lib.pt_convergence_update(None, None, 1, None, None, None, None, None) != 0
    assert b"pt_convergence_update" in lib.pt_last_error(None)


# ---- unbiasedness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batches", [[1, 1, 2, 4, 8, 3, 5], [3] * 8], ids=["unequal", "equal"])
def test_the_variance_is_unbiased(batches):
    """v * k1 estimates the per-frame variance sigma^2 with B - 1 degrees of freedom per pixel: its pixel mean has the standard
    deviation sigma^2 sqrt(2 / ((B - 1) N)).  A B written for B - 1 is off by 1 / B, a dropped k1 by the factor k1."""
    n, mu, sigma = 1 << 20, 1.0, 0.25
    rng = np.random.default_rng(20240607)
    state = np.zeros((n, 4), F)
    total, k = np.zeros(n, np.float64), 0
    for size in batches:
        for _ in range(size):
            total += rng.normal(mu, sigma, n)
        k += size
        state, err, measured, invalid = cr.update_pixels((total / k).astype(F), state, k, 0.01)
        assert not invalid.any() and measured.all() == (k > batches[0])
    b = len(batches)
    assert np.all(state[:, 3] == b) and np.all(state[:, 2] == k)
    v = state[:, 1].astype(np.float64) / ((b - 1) * k)
    est = float(np.mean(v * k))
    tol = 5.0 * sigma ** 2 * np.sqrt(2.0 / ((b - 1) * n))
    print("sigma^2 %.6f estimated %.6f (tolerance %.2e)" % (sigma ** 2, est, tol))
    assert abs(est - sigma ** 2) <= tol
    # err is sqrt(v) / max(l, floor) of the same numbers
    l = state[:, 0]
    assert np.array_equal(err, (np.sqrt((state[:, 1] / (F(b - 1) * F(k))).astype(F)) / np.maximum(l, F(0.01))).astype(F))


# ---- restart and invalid pixels -----------------------------------------------------------------------------------------------
def _acc(lums):
    a = np.zeros((len(lums), 4), F)
    a[:, :3] = np.asarray(lums, F)[:, None]
    return a


def test_a_restart_and_a_zero_state_start_over():
    acc = _acc([0.5, 0.25, 2.0])
    l = cr.lum(acc)
    zero = np.zeros((3, 4), F)
    s1, e1, t1, i1 = cr.update(acc, zero, 3, 1, 4)
    assert np.array_equal(s1, np.stack([l, np.zeros(3, F), np.full(3, 4, F), np.ones(3, F)], axis=-1))
    assert np.all(e1 == -1) and np.all(t1 == -1)
    assert (i1["measured_pixels"], i1["unmeasured_pixels"], i1["invalid_pixels"], i1["converged_pixels"]) == (0, 3, 0, 0)
    assert i1["max_error"] == 0 and i1["quantile_error"] == 0 and i1["frames"] == 4 and not i1["histogram"].any()
    s2, e2, _, i2 = cr.update(_acc([0.75, 0.25, 1.0]), s1, 3, 1, 6)
    assert i2["measured_pixels"] == 3 and np.all(s2[:, 3] == 2) and e2[1] == 0 and e2[0] > 0
    for k1 in (6, 5, 1):                       # k1 <= k0: the accumulation was restarted
        s3, e3, t3, i3 = cr.update(acc, s2, 3, 1, k1)
        assert np.array_equal(s3, np.stack([l, np.zeros(3, F), np.full(3, k1, F), np.ones(3, F)], axis=-1))
        assert np.all(e3 == -1) and np.all(t3 == -1) and i3["unmeasured_pixels"] == 3 and i3["measured_pixels"] == 0
    weird = s2.copy()
    weird[:, 2] = [-1.0, np.nan, 0.0]          # !(k0 > 0): a first observation whatever else the state holds
    s4, e4, _, _ = cr.update(acc, weird, 3, 1, 7)
    assert np.array_equal(s4[:, 1:], np.tile(np.array([0, 7, 1], F), (3, 1))) and np.all(e4 == -1)


def test_an_invalid_pixel_clears_its_state_and_counts_once():
    acc = _acc([0.5, 0.5, 0.5, 0.5, 0.5])
    s1, _, _, _ = cr.update(acc, np.zeros((5, 4), F), 5, 1, 2)
    bad = acc.copy()
    bad[1, 0] = np.nan
    bad[2, 1] = np.inf
    bad[3, 2] = -np.inf
    bad[4, 0], bad[4, 1] = np.inf, -np.inf                           # infinite channels, NaN luminance
    s2, e2, t2, i2 = cr.update(bad, s1, 5, 1, 4)
    assert np.all(s2[1:] == 0) and np.all(e2[1:] == -1) and s2[0, 3] == 2 and e2[0] == 0
    assert (i2["measured_pixels"], i2["unmeasured_pixels"], i2["invalid_pixels"]) == (1, 0, 4)
    assert t2[0] == 0
    s3, _, _, i3 = cr.update(acc, s2, 5, 1, 6)                        # afterwards they start over
    assert (i3["measured_pixels"], i3["unmeasured_pixels"], i3["invalid_pixels"]) == (1, 4, 0) and np.all(s3[1:, 3] == 1)


# ---- reductions ---------------------------------------------------------------------------------------------------------------
def _reduce(errs, **kw):
    errs = np.asarray(errs, F)
    return cr.reduce_errors(errs, np.ones(errs.size, bool), 0, 0, 3, cr.params(**kw))


def _check_against_sort(errs, info, permille, threshold):
    e = np.sort(np.asarray(errs, F))
    n = e.size
    r = max(1, -(-n * permille // 1000))                              # ceil(n * permille / 1000), at least 1
    j = int(cr.bin_index(e[r - 1:r])[0])
    assert info["quantile_error"] == cr.bin_upper_edge(j)
    if 0 < j < cr.BINS - 1:
        assert cr.bin_upper_edge(j - 1) <= e[r - 1] < info["quantile_error"]
    assert info["max_error"] == e[-1] and info["converged_pixels"] == int((e <= F(threshold)).sum()) and info["measured_pixels"] == n
    assert int(info["histogram"].sum()) == n


def test_quantile_max_and_converged_count_against_a_sort():
    rng = np.random.default_rng(7)
    errs = np.exp2(rng.uniform(-20, 2, 1001)).astype(F)
    for permille in (1, 500, 949, 950, 999, 1000):
        for threshold in (0.02, 1e-3):
            _check_against_sort(errs, _reduce(errs, quantile_permille=permille, threshold=threshold), permille, threshold)
    # r rounds up: of 3 pixels, 334 permille is the second, 333 the first; of 1001, 999 permille is the 1000th (999.999 rounds up)
    three = np.array([0.001, 0.01, 0.1], F)
    assert [cr.quantile_bin(_reduce(three)["histogram"], q)[0] for q in (1, 333, 334, 666, 667, 1000)] == [1, 1, 2, 2, 3, 3]
    assert cr.quantile_bin(_reduce(errs)["histogram"], 999)[0] == 1000
    for q in (333, 334, 667):
        _check_against_sort(three, _reduce(three, quantile_permille=q), q, 0.02)
    # every pixel in one bin
    flat = np.full(500, 0.03, F)
    info = _reduce(flat, quantile_permille=1)
    assert np.count_nonzero(info["histogram"]) == 1 and info["quantile_error"] == _reduce(flat, quantile_permille=1000)["quantile_error"]
    assert info["quantile_error"] == F(0.03125) and info["max_error"] == F(0.03)           # 0.03 lies in [0.029296875, 0.03125)
    # both open bins: zero and everything below 2^-24 in bin 0, everything from 2^7.875 up, infinity and NaN in bin 255
    assert list(cr.bin_index(np.array([0.0, 1e-40, 2.0 ** -25, 2.0 ** -24, np.nextafter(F(2.0 ** -23), F(0)), 2.0 ** -23], F))) == [0, 0, 0, 0, 7, 8]
    assert list(cr.bin_index(np.array([np.nextafter(F(2.0 ** 7.875), F(0)) * F(0.99), 240.0, 256.0, 1e30, np.inf, np.nan], F))) == [254, 255, 255, 255, 255, 255]
    lo = _reduce([0.0, 0.0, 1e-30], quantile_permille=1000)
    assert lo["histogram"][0] == 3 and lo["quantile_error"] == F(2.0 ** -24 * 1.125) and lo["converged_pixels"] == 3
    hi = _reduce([300.0, np.inf, 0.5], quantile_permille=1000)
    assert hi["histogram"][255] == 2 and hi["quantile_error"] == F(256.0) and hi["max_error"] == np.inf
    # err == threshold exactly counts as converged, the next float up does not
    t = F(0.02)
    edge = _reduce([t, np.nextafter(t, F(1)), np.nextafter(t, F(0))], threshold=0.02)
    assert edge["converged_pixels"] == 2
    assert cr.is_converged(dict(edge, converged_pixels=3), 1000) and not cr.is_converged(edge, 950) and cr.is_converged(edge, 666)


def test_tiles_are_row_major_from_the_bottom():
    w, h = 33, 17
    err = np.full(w * h, -1.0, F)
    measured = np.zeros(w * h, bool)
    for (x, y, e) in ((0, 0, 0.5), (15, 15, 0.75), (16, 0, 0.25), (32, 16, 2.0), (31, 16, 0.0)):
        err[y * w + x], measured[y * w + x] = e, True
    assert list(cr.tile_max(err, measured, w, h)) == [0.75, 0.25, -1, -1, 0.0, 2.0]


# ---- calibration on real noise ------------------------------------------------------------------------------------------------
def test_calibration_on_the_oracle(oracle):
    size, spp, depth, floor = 48, 16, 4, 0.01
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj"))
    sc = oracle.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    frames = np.zeros((CAL_KREF, size * size, 3), F)
    for f in range(CAL_KREF):
        # a launch with frame index f onto a zero accumulation leaves frame / (f + 1): the frame's own mean is that times f + 1
        acc, _, _, _ = sc.render(copy_params(make_params(size, size, spp, depth, True, True, frame=f)))
        frames[f] = acc.reshape(-1, 4)[:, :3] * F(f + 1)
    l_ref = cr.lum(frames.astype(np.float64).mean(axis=0).astype(F)).astype(np.float64)
    ratios = []
    for r in range(CAL_RUNS):
        state = np.zeros((size * size, 4), F)
        a = np.zeros((size * size, 3), F)
        for k in range(CAL_FRAMES):
            c = frames[r * CAL_FRAMES + k]
            a = c if k == 0 else a + F(1.0 / (k + 1)) * (c - a)         # the reference's running mean, fp32
            state, err, tiles, info = cr.update(a, state, size, size, k + 1, cr.params(lum_floor=floor))
        assert info["measured_pixels"] == size * size and info["frames"] == CAL_FRAMES
        l = state[:, 0].astype(np.float64)
        v = state[:, 1].astype(np.float64) / ((state[:, 3].astype(np.float64) - 1.0) * CAL_FRAMES)
        keep = l > floor
        assert keep.mean() > 0.75
        ratios.append(float(((l - l_ref) ** 2)[keep].sum() / v[keep].sum()))
    mean, spread = float(np.mean(ratios)), float(np.std(ratios, ddof=1))
    print("R = %s  mean %.4f spread %.4f (expected %.4f)" % (" ".join("%.3f" % x for x in ratios), mean, spread, CAL_EXPECTED))
    for x in ratios:
        assert abs(x - CAL_MEAN) <= CAL_BAND, ratios
    assert abs(CAL_MEAN - CAL_EXPECTED) <= CAL_BAND
