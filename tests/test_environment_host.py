"""Environment map on the host (no GPU): the numpy reference of tests/env_ref.py is a normalised, self-consistent distribution; the
.hdr / .pfm readers of host/ImageIO.cpp and of pathtracer.py decode the committed fixtures (tests/golden/make_env_fixtures.py) to the
same floats; the new entry points are declared and bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from env_ref import EnvRef, sphere_directions  # noqa: E402

FIX = os.path.join(ROOT, "tests", "golden", "env")


def _map(h=12, w=24, seed=3, sun=True):
    r = np.random.default_rng(seed)
    img = r.uniform(0.0, 1.0, size=(h, w, 3)).astype(np.float32)
    img[2, 5:7] = 0.0                      # black texels: bins of zero width
    if sun:
        img[3, 17] = (400.0, 380.0, 300.0)
    return img


def test_pdf_integrates_to_one_over_the_sphere():
    e = EnvRef(_map())
    # the pdf is w * scale / sin(theta) per texel: integrate over a grid 8x finer than the map, in (theta, phi) with the sin(theta) Jacobian
    nv, nu = e.h * 8, e.w * 8
    th = (np.arange(nv) + 0.5) / nv * np.pi
    ph = (np.arange(nu) + 0.5) / nu * 2 * np.pi - np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.sin(P), np.cos(T), -np.sin(T) * np.cos(P)], axis=-1)
    integral = float((e.pdf(d) * np.sin(T)).sum() * (np.pi / nv) * (2 * np.pi / nu))
    assert abs(integral - 1.0) < 1e-5, integral
    # and a Monte-Carlo check with uniform directions (a map without the sun: its variance is small)
    u = sphere_directions(200000, 7)
    assert abs(float(EnvRef(_map(sun=False)).pdf(u).mean()) * 4 * np.pi - 1.0) < 0.01


def test_pdf_of_the_sample_is_the_sampled_pdf_and_follows_the_weights():
    e = EnvRef(_map())
    r = np.random.default_rng(11)
    counts = np.zeros((e.h, e.w))
    n_checked = 0
    for u1, u2 in r.uniform(size=(4000, 2)):
        d, pdf, (row, col), (fv, fu) = e.sample(u1, u2)
        counts[row, col] += 1
        assert pdf > 0 and e.weight[row, col] > 0           # a black texel is never drawn
        assert abs(np.linalg.norm(d) - 1.0) < 1e-9
        if min(fv, 1 - fv, fu, 1 - fu) < 1e-3:              # the direction lies on a texel edge: the lookup may pick the neighbour
            continue
        assert tuple(int(x) for x in e.texel(d.astype(np.float32))) == (row, col)
        # the direction's fp32 y carries a rounding of 2^-24 relative to 1 - |y| into sin(theta) near the poles
        assert abs(float(e.pdf(d)) - pdf) <= (1e-5 + 1.2e-7 / (1.0 - abs(d[1]))) * pdf
        n_checked += 1
    assert n_checked > 3500
    p = e.weight / e.weight.sum()
    assert abs(counts[3, 17] / counts.sum() - p[3, 17]) < 0.03   # the sun gets its share


def test_black_map_has_nothing_to_sample():
    e = EnvRef(np.zeros((4, 8, 3), np.float32))
    assert e.total == 0 and e.pdf_scale == 0
    assert np.all(e.pdf(sphere_directions(100)) == 0)


def _host_load(path):
    from acgpathtracing_amd import _native
    H = _native.host()
    w, h = C.c_int(0), C.c_int(0)
    err = C.create_string_buffer(256)
    assert H.pth_load_environment(path.encode(), None, C.byref(w), C.byref(h), err, 256) == 0, err.value
    out = np.zeros((h.value, w.value, 3), np.float32)
    assert H.pth_load_environment(path.encode(), out.ctypes.data, C.byref(w), C.byref(h), err, 256) == 0, err.value
    return out


@pytest.mark.parametrize("name", ["flat.hdr", "rle.hdr", "grey.pfm", "colour.pfm"])
def test_cpp_and_numpy_readers_decode_the_fixtures_alike(name):
    import acgpathtracing_amd as pt
    exp = np.load(os.path.join(FIX, "expected.npz"))[name.replace(".", "_")]
    a = _host_load(os.path.join(FIX, name))
    b = pt.loadEnvironment(os.path.join(FIX, name))
    assert a.shape == b.shape == exp.shape
    assert np.array_equal(a.view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(b.view(np.uint32), exp.view(np.uint32))


def test_readers_refuse_what_they_cannot_read(tmp_path):
    from acgpathtracing_amd import _native
    import acgpathtracing_amd as pt
    H = _native.host()
    bad = tmp_path / "bad.hdr"
    bad.write_bytes(b"#?RADIANCE\n\n+Y 4 +X 4\n" + bytes(64))          # bottom-up orientation: not supported
    w, h = C.c_int(0), C.c_int(0)
    err = C.create_string_buffer(256)
    assert H.pth_load_environment(str(bad).encode(), None, C.byref(w), C.byref(h), err, 256) == 1 and b"resolution" in err.value
    with pytest.raises(ValueError):
        pt.loadEnvironment(str(bad))
    with pytest.raises(ValueError):
        pt.loadEnvironment(str(tmp_path / "x.exr"))


def test_new_symbols_are_declared_and_bound():
    from acgpathtracing_amd import _native
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    thdr = open(os.path.join(ROOT, "include", "acgpt_test.h")).read()
    assert "int pt_set_environment(pt_ctx* ctx, const float* rgb, uint32_t width, uint32_t height, pt_float3 scale);" in hdr
    assert "int pt_debug_environment(pt_ctx* ctx, int op, const float* in, size_t n, float* out);" in thdr
    assert "pt_set_environment" in _native.ABI_SYMBOLS and "pt_debug_environment" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4
    lib = C.CDLL(_native.hip_library_path())
    assert hasattr(lib, "pt_set_environment") and hasattr(lib, "pt_debug_environment")


def test_env_kernels_keep_the_budget_of_their_parents():
    """Read from the code object: ENV and ENV deep are five-wave kernels (<= 96 registers) and LIGHTS ENV a four-wave one (<= 128),
    none with spills or scratch; each in both math modes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from acgpathtracing_amd import _native
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_render_env<" in k["name"]]
    assert len(rows) == 6, [k["name"] for k in rows]
    for k in rows:
        five = k["name"].split("<")[1].split(",")[4].strip() == "5"
        assert k["vgpr_count"] <= (96 if five else 128), k
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert sum(k["name"].split("<")[1].split(",")[4].strip() == "5" for k in rows) == 4
