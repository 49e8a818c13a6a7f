"""The bloom without a GPU: the arithmetic of pt_bloom as include/acgpt.h states it (tests/bloom_ref.py) is pinned by its properties;
the library exports and binds the call; pathtracer.bloom refuses bad settings on the host and displayTransform(bloom=None) takes the
path it took before there was a bloom.

The float32 statement against its float64 twin (test_energy_and_the_float64_twin): an impulse of (120, 80, 40) in the middle of a
black 257 x 257 image, farther from every edge than the pyramid reaches, under the four parameter sets of ENERGY_SETS.  The largest
|out32 - out64| over the image, relative to the impulse's largest channel, measured on the reference:
    3.1e-8, 1.7e-8, 5.4e-8, 2.2e-9   ->   TWIN_MEASURED = 5.5e-8 (2^-24 is 6.0e-8), and the test allows TWIN_FACTOR = 4 times that."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import bloom_ref as br

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN_MEASURED, TWIN_FACTOR = 5.5e-8, 4.0             # docstring above
ENERGY_SETS = [dict(threshold=0.0, knee=0.0, clamp=0.0, spread=1.0, levels=5, intensity=0.5),
               dict(threshold=1.0, knee=0.5, clamp=50.0, spread=0.7, levels=5, intensity=0.25),
               dict(threshold=2.0, knee=0.0, clamp=0.0, spread=0.0, levels=1, intensity=1.0),
               dict(levels=4)]                      # the defaults, cut to a reach that fits the image


@pytest.fixture(scope="module")
def lib():
    _build.build_hip()
    return _native.hip()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def positive(h, w, seed, lo=-3.0, hi=3.0):
    """strictly positive float32 [h, w, 4], log-uniform over 2^lo .. 2^hi"""
    return np.exp2(np.random.default_rng(seed).uniform(lo, hi, (h, w, 4))).astype(F)


def reach(n):
    """how far (in source pixels, Chebyshev) a pixel's light gets through n levels: a level-k texel's footprint spans 1.5 * 2^k to
    either side of its centre, and the n up steps add a texel of every level, 2^n + ... + 2 < 2^(n+1)"""
    return int(3.5 * 2 ** n) + 1


# ---- symbol and ABI -----------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_call(lib, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.hip_library_path()], capture_output=True, text=True, check=True).stdout
    assert "pt_bloom" in set(re.findall(r" T (pt_[a-z_]+)", out))
    assert "pt_bloom" in _native.ABI_SYMBOLS
    assert lib.pt_bloom.restype is C.c_int and len(lib.pt_bloom.argtypes) == 7
    assert lib.pt_abi_version() == 4 == _native.ABI_VERSION
    assert callable(pt.bloom)
    assert {k: float(v) for k, v in pt.BLOOM_DEFAULTS.items()} == {k: float(v) for k, v in br.DEFAULTS.items()}
    assert br.MAX_LEVELS == _native.BLOOM_MAX_LEVELS
    # the C compiler's layout of the two structures against the ctypes mirrors
    fields_p = [n for n, _ in _native.BloomParams._fields_]
    fields_i = [n for n, _ in _native.BloomInfo._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "acgpt.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(pt_bloom_params), sizeof(pt_bloom_info));\n'
                   + "".join('  printf(" %%zu", offsetof(pt_bloom_params, %s));\n' % f for f in fields_p)
                   + "".join('  printf(" %%zu", offsetof(pt_bloom_info, %s));\n' % f for f in fields_i)
                   + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_native.BloomParams), C.sizeof(_native.BloomInfo)] + [getattr(_native.BloomParams, f).offset for f in fields_p] + \
           [getattr(_native.BloomInfo, f).offset for f in fields_i]
    assert got == want and got[:2] == [24, 40]
    assert sorted(br.DEFAULTS) == sorted(fields_p)


def test_null_context_is_refused_with_a_message(lib):
    assert lib.pt_bloom(None, None, 1, 1, None, None, None) != 0
    assert b"pt_bloom" in lib.pt_last_error(None)


def test_kernel_sources_do_not_include_the_bloom():
    """the render kernels' source hash, the committed profiles and bench.py do not see this post-pass"""
    assert "bloom.hip" in _build.HIP_SOURCES and "bloom.h" in _build.HIP_HEADERS
    assert not {"bloom.hip", "bloom.h", "image_common.h"} & set(_build.KERNEL_SOURCES)


# ---- levels -------------------------------------------------------------------------------------------------------------------
def test_levels_of():
    assert br.levels_of(1, 1, 8) == [(1, 1)]                               # a 1 x 1 source builds one 1 x 1 level
    assert br.levels_of(2, 2, 8) == [(1, 1)] and br.levels_of(2, 1, 8) == [(1, 1)] and br.levels_of(1, 2, 8) == [(1, 1)]
    assert br.levels_of(1, 9, 8) == [(1, 5), (1, 3), (1, 2), (1, 1)]      # 1 x N: the width stays 1
    assert br.levels_of(1, 1048577, 3) == [(1, 524289), (1, 262145), (1, 131073)]
    for k in range(1, 9):
        n = 2 ** k
        full = br.levels_of(n, n, 8)
        assert full == [(n >> j, n >> j) for j in range(1, k + 1)][:8] and full[-1] == ((1, 1) if k <= 8 else full[-1])
        assert len(br.levels_of(n + 1, n + 1, 8)) == min(k + 1, 8)         # 2^k + 1 halves to 2^(k-1) + 1, ..., 2, 1: one level more
        assert br.levels_of(n + 1, n + 1, 8)[0] == (n // 2 + 1, n // 2 + 1)
        if k >= 2:
            assert br.levels_of(n - 1, n - 1, 8) == full                  # 2^k - 1 rounds up to the sizes of 2^k
    assert br.levels_of(1920, 1080, 6) == [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]
    assert br.levels_of(1920, 1080, 1) == [(960, 540)] and len(br.levels_of(40, 24, 4)) == 4
    assert br.levels_of(4099, 3, 8)[:3] == [(2050, 2), (1025, 1), (513, 1)] and br.levels_of(4099, 3, 8)[-1] == (17, 1)


# ---- the statement's properties -------------------------------------------------------------------------------------------------
def test_a_constant_image_is_exact():
    """every weight is dyadic and so is 0.5: level k = 0.5, E_3 = 1, E_2 = 1.5, E_1 = 2, gain = 0.5 / 4, out = 0.5 + 0.125 * 2"""
    h, w = 24, 40
    src = np.full((h, w, 4), 0.5, F)
    src.view(np.uint32)[..., 3] = (np.uint32(0x7FC00000) | np.arange(h * w, dtype=np.uint32).reshape(h, w))
    out, info, pyr = br.bloom(src, dict(threshold=0.0, knee=0.0, clamp=0.0, spread=1.0, intensity=0.5, levels=4))
    assert info["levels"] == 4 and len(pyr["down"]) == 4
    assert np.all(out[..., :3] == F(0.75))
    assert np.array_equal(bits(out)[..., 3], bits(src)[..., 3])
    assert info["bright_pixels"] == h * w and info["invalid_pixels"] == 0
    assert info["total_luma_q16"] == info["bright_luma_q16"] == h * w * int(float(br.lum(src[0, 0, :3])) * 65536.0)
    assert F(info["max_luma"]) == br.lum(src[0, 0, :3])


def test_threshold_zero_feeds_the_raw_source():
    src = positive(37, 53, 1)
    _, info, pyr = br.bloom(src, dict(threshold=0.0, knee=0.0, clamp=0.0, levels=3))
    assert np.array_equal(bits(pyr["P"]), bits(src[..., :3]))             # c = l / l = 1: the pixel's own bits
    assert np.array_equal(bits(pyr["down"][0]), bits(br.down(src[..., :3])))
    assert info["bright_pixels"] == 37 * 53 and info["bright_luma_q16"] == info["total_luma_q16"]


def test_a_nan_and_an_infinity_stay_where_they_are():
    src = positive(45, 61, 2)
    clean = src.copy()
    src[20, 30, 1] = np.nan
    src[7, 50, :3] = np.inf
    clean[20, 30, :3] = 0
    clean[7, 50, :3] = 0
    p = dict(threshold=0.5, knee=0.25, levels=4, intensity=0.3)
    out, info, _ = br.bloom(src, p)
    ref, rinfo, _ = br.bloom(clean, p)
    assert info["invalid_pixels"] == 2 and rinfo["invalid_pixels"] == 0
    assert np.isnan(out[20, 30, 1]) and np.all(np.isposinf(out[7, 50, :3]))
    # the NaN pixel's finite channels get the glare the zeroed pixel gets (0 + x = x)
    assert out[20, 30, 0] == src[20, 30, 0] + ref[20, 30, 0] and out[20, 30, 2] == src[20, 30, 2] + ref[20, 30, 2]
    mask = np.ones((45, 61), bool)
    mask[20, 30] = mask[7, 50] = False
    assert np.array_equal(bits(out)[mask], bits(ref)[mask])
    assert np.array_equal(bits(out)[..., 3], bits(src)[..., 3])


def test_a_dark_pixel_out_of_reach_keeps_its_bits():
    n = 3
    src = positive(128, 128, 3, lo=-6.0, hi=-2.0)                          # everything below threshold - knee = 0.5
    src[8:12, 8:12, :3] = 40.0
    out, info, _ = br.bloom(src, dict(threshold=1.0, knee=0.5, levels=n, intensity=0.5))
    assert info["bright_pixels"] == 16
    yy, xx = np.mgrid[0:128, 0:128]
    far = (np.maximum(np.abs(yy - 9.5), np.abs(xx - 9.5)) > 1.5 + reach(n))
    assert far.sum() > 128 * 128 // 2
    assert np.array_equal(bits(out)[far], bits(src)[far])
    near = ~far & (np.maximum(np.abs(yy - 9.5), np.abs(xx - 9.5)) < 6)
    assert np.all(out[near][:, :3] > src[near][:, :3])


def test_the_knee_is_continuous_and_monotone():
    T, K = 1.0, 0.5
    l = np.linspace(T - K - 0.25, T + K + 0.25, 20001).astype(F)
    e = br.excess(l, T, K, 0.0)
    assert e.dtype == F
    assert np.all(e[l <= F(T - K)] == 0) and e.min() == 0
    assert np.all(np.diff(e.astype(np.float64)) >= 0)
    step = float(np.max(np.diff(l.astype(np.float64))))
    assert np.max(np.diff(e.astype(np.float64))) <= step * 1.001 + 2.0 ** -23      # slope at most 1: no jump at either end of the knee
    assert br.excess(F(T + K), T, K, 0.0) == F(K)                          # q = (2K)^2 / 4K = K = d: the two branches meet
    above = l >= F(T + K)
    assert np.array_equal(e[above], (l - F(T))[above])
    inside = (l > F(T - K)) & (l < F(T + K))
    assert np.all(e[inside] > 0) and np.all(e[inside] >= (l - F(T))[inside])
    hard = br.excess(l, T, 0.0, 0.0)
    assert np.array_equal(hard, np.maximum(l - F(T), F(0)))
    assert np.all(e >= hard)


def test_the_clamp_caps_what_a_pixel_feeds():
    l = np.exp2(np.linspace(-2, 14, 2000)).astype(F)
    for T, K in ((1.0, 0.5), (0.0, 0.0), (2.0, 0.0)):
        free, capped = br.excess(l, T, K, 0.0), br.excess(l, T, K, 50.0)
        assert np.array_equal(capped, np.minimum(free, F(50.0))) and capped.max() == F(50.0) and free.max() > 1e4
    src = np.zeros((33, 33, 4), F)
    src[16, 16, :3] = (3000.0, 2000.0, 1000.0)
    _, info, pyr = br.bloom(src, dict(threshold=1.0, knee=0.5, clamp=50.0, levels=2))
    assert info["bright_pixels"] == 1 and info["bright_luma_q16"] == 50 * 65536
    assert abs(float(br.lum(pyr["P"][16, 16])) - 50.0) < 50.0 * 2.0 ** -21


@pytest.mark.parametrize("index", range(len(ENERGY_SETS)))
def test_energy_and_the_float64_twin(index):
    """every filter has unit gain away from the edges: the glare of an impulse sums to intensity * P(impulse)"""
    p = br.params(**ENERGY_SETS[index])
    size, c = 257, 128
    n = len(br.levels_of(size, size, p["levels"]))
    assert reach(n) < c
    src = np.zeros((size, size, 4), F)
    src[c, c, :3] = (120.0, 80.0, 40.0)
    out64, info64, pyr64 = br.bloom(src, p, dtype=np.float64)
    glare = (out64[..., :3] - src[..., :3].astype(np.float64)).sum(axis=(0, 1))
    want = p["intensity"] * pyr64["P"][c, c]
    assert np.all(want > 0)
    assert np.max(np.abs(glare / want - 1.0)) <= 1e-12
    out32, info32, _ = br.bloom(src, p)
    assert out32.dtype == F and info32["bright_pixels"] == info64["bright_pixels"] == 1
    err = float(np.max(np.abs(out32[..., :3].astype(np.float64) - out64[..., :3]))) / 120.0
    print("set %d: fp32 against float64 %.3e (allowed %.3e)" % (index, err, TWIN_FACTOR * TWIN_MEASURED))
    assert err <= TWIN_FACTOR * TWIN_MEASURED


def test_the_default_intensity_is_the_sweep_s_pick():
    """tools/bloom_sweep.py on the oracle's converged Cornell box: the largest intensity of its list that raises the image's mean
    luminance by less than 2 % (DESIGN.md section 21 holds the table)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bloom_sweep
    import display_ref as dr
    gold = np.load(os.path.join(ROOT, "tests", "golden", "denoise_cornell_128.npz"))
    ref = np.asarray(gold["ref"], F)
    img = np.concatenate([ref, np.ones(ref.shape[:2] + (1,), F)], axis=-1)
    rows = bloom_sweep.table(img, dr.transform(img.reshape(-1, 4), dr.params())[1]["exposure"])
    assert [r["intensity"] for r in rows] == [0.02, 0.05, 0.1, 0.2, 0.5]
    assert bloom_sweep.pick(rows) == br.DEFAULTS["intensity"] == pt.BLOOM_DEFAULTS["intensity"]
    assert all(0.0 < r["bright_share"] < 1.0 for r in rows) and np.all(np.diff([r["increase"] for r in rows]) > 0)


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
class _Poison:
    """Stands in for the library: any call is an error."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


@pytest.mark.parametrize("bad", [dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(knee=-0.1), dict(knee=1.5),
                                 dict(knee=float("nan")), dict(clamp=-1.0), dict(clamp=float("inf")), dict(intensity=-0.1), dict(intensity=float("nan")),
                                 dict(spread=-0.5), dict(spread=4.5), dict(spread=float("nan")), dict(levels=0), dict(levels=9), dict(levels=2.5)])
def test_bad_settings_are_refused_before_the_library(monkeypatch, bad):
    monkeypatch.setattr(_native, "hip", lambda: _Poison())
    state = pt.PathTracerState()
    with pytest.raises(ValueError):
        pt.bloom(state, **bad)
    with pytest.raises(ValueError):
        pt.displayTransform(state, bloom=bad)


def test_unknown_settings_are_refused_before_the_library(monkeypatch):
    monkeypatch.setattr(_native, "hip", lambda: _Poison())
    state = pt.PathTracerState()
    with pytest.raises(ValueError):
        pt.displayTransform(state, bloom=dict(treshold=1.0))
    with pytest.raises(TypeError):
        pt.bloom(state, treshold=1.0)


class _Lib:
    """Records the calls and answers as a library that metered an exposure of 2 would."""

    def __init__(self):
        self.calls = []
        self.next_ptr = 0x1000

    def pt_device_malloc(self, ctx, out, nbytes):
        self.calls.append(("malloc", nbytes))
        self.next_ptr += 0x100000
        out._obj.value = self.next_ptr
        return 0

    def pt_device_free(self, ctx, ptr):
        self.calls.append(("free",))
        return 0

    def pt_copy_to_host(self, ctx, dst, src, nbytes):
        self.calls.append(("to_host", nbytes))
        return 0

    def pt_display_transform(self, ctx, src, n, dp, out, fb, info):
        d = dp._obj
        self.calls.append(("display", src, n, d.exposure, d.prev_exposure, d.adapt, out, fb, info is not None))
        if info is not None:
            info._obj.exposure = d.exposure if d.exposure > 0 else 2.0
            info._obj.metered_pixels = 0 if d.exposure > 0 else n
        return 0

    def pt_bloom(self, ctx, src, w, h, bp, out, info):
        b = bp._obj
        self.calls.append(("bloom", src, w, h, b.threshold, b.knee, b.clamp, b.intensity, b.spread, b.levels, out))
        info._obj.levels = 3
        return 0


def _state(w, h):
    state = pt.PathTracerState()
    state.params.width, state.params.height = w, h
    state.params.accumulationBuffer = 0xABC000
    return state


def test_display_transform_without_bloom_takes_the_path_it_took(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(_native, "hip", lambda: lib)
    state = _state(8, 4)
    rgba, info = pt.displayTransform(state, prev_exposure=1.5, adapt=0.25)
    kinds = [c[0] for c in lib.calls]
    assert kinds == ["malloc", "display", "to_host", "free"]                   # one frame buffer, one call, no pt_bloom
    assert lib.calls[0] == ("malloc", 8 * 4 * 4)
    assert lib.calls[1] == ("display", 0xABC000, 32, 0.0, 1.5, 0.25, None, lib.next_ptr, True)
    assert rgba.shape == (4, 8, 4) and info["exposure"] == 2.0 and "bloom" not in info
    assert sorted(info) == ["exposure", "histogram", "metered_luminance", "metered_pixels", "unmetered_pixels"]
    lib.calls.clear()
    pt.displayTransform(state, bloom=None, exposure=3.0)
    assert [c[0] for c in lib.calls] == ["malloc", "display", "to_host", "free"] and lib.calls[1][3] == 3.0


def test_display_transform_with_bloom_meters_first(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(_native, "hip", lambda: lib)
    state = _state(8, 4)
    rgba, info = pt.displayTransform(state, prev_exposure=1.5, adapt=0.25, bloom=dict(threshold=3.0, knee=1.0, clamp=10.0, levels=4))
    kinds = [c[0] for c in lib.calls]
    assert kinds == ["malloc", "malloc", "display", "bloom", "display", "to_host", "free", "free"]
    meter, glare, shown = lib.calls[2], lib.calls[3], lib.calls[4]
    fb, tmp = lib.next_ptr - 0x100000, lib.next_ptr
    assert meter == ("display", 0xABC000, 32, 0.0, 1.5, 0.25, None, fb, True)            # metered on the image without its glare
    # display units over the exposure of 2, in fp32
    assert glare == ("bloom", 0xABC000, 8, 4, 1.5, 0.5, 5.0, float(F(pt.BLOOM_DEFAULTS["intensity"])), 1.0, 4, tmp)
    assert shown == ("display", tmp, 32, 2.0, 1.5, 0.25, None, fb, False)                # the metered exposure as a manual one
    assert info["exposure"] == 2.0 and info["metered_pixels"] == 32 and info["bloom"]["levels"] == 3 and info["bloom"]["bright_share"] == 0.0
    lib.calls.clear()
    rgba, info = pt.displayTransform(state, exposure=4.0, bloom={})                       # a manual exposure: no metering call
    assert [c[0] for c in lib.calls] == ["malloc", "malloc", "bloom", "display", "to_host", "free", "free"]
    assert lib.calls[2][4:7] == (0.25, 0.125, 0.0) and lib.calls[3][3] == 4.0
    assert info["exposure"] == 4.0 and info["metered_pixels"] == 0
    ae = pt.AutoExposure(speed=1.0, bloom={})
    lib.calls.clear()
    ae.frame(state, 0.1)
    assert [c[0] for c in lib.calls].count("bloom") == 1 and ae.exposure == 2.0
