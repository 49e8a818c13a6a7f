"""Environment maps wider and taller than one workgroup of the device's CDF scan (csrc/environment.hip: 256 threads, each owning a run
of ceil(n / 256) values).  Every other GPU test uploads maps of at most 64 x 128, where a run is one value.  Here: the tables the
device built, read back (pt_debug_environment_tables), bit for bit against tests/env_ref.py at the shapes of tests/env_cases.py and
against the CPU oracle at 1024 x 2048; the device's lookup, pdf and sample on those tables, among them tables that step down across
run boundaries; renders through a 260 x 300 map; and the largest sizes pt_set_environment accepts."""
import numpy as np
import pytest

import env_cases as K
from env_cases import assert_tables_equal, check_one_texel, check_pdf_of_samples, check_samples, sample_inputs
from env_ref import EnvRef, sphere_directions
from test_gpu_environment import Ctx, FAST, IEEE, batches_and_partitions_with_a_map, constant_map_is_seen_exactly, furnace
from test_oracle_env_ggx import sphere_scene

pytestmark = pytest.mark.gpu


def device_tables(c, texels=True, conditional=True):
    """the map's tables as the device holds them; None without a map"""
    dims = np.zeros(2, np.uint32)
    info = np.zeros(2, np.float32)
    rc = c.L.pt_debug_environment_tables(c.ctx, None, None, None, None, dims.ctypes.data)
    assert rc in (0, 1), c.err()
    if rc == 0:
        assert dims[0] == 0 and dims[1] == 0
        return None
    w, h = int(dims[0]), int(dims[1])
    tex = np.zeros((h, w, 4), np.float32) if texels else None
    cond = np.zeros((h, w), np.float32) if conditional else None
    marg = np.zeros(h, np.float32)
    assert c.L.pt_debug_environment_tables(c.ctx, tex.ctypes.data if texels else None, marg.ctypes.data,
                                           cond.ctypes.data if conditional else None, info.ctypes.data, None) == 1, c.err()
    return {"texels": tex, "marginal": marg, "conditional": cond, "total": info[0], "pdf_scale": info[1]}


# ---- 1. the tables ---------------------------------------------------------------------------------------------------------------
def test_tables_match_env_ref_bit_for_bit():
    """one context, the cases in turn, twice: every upload replaces a map of another shape, and the second upload of a map gives the
    bits of its first"""
    c = Ctx.box()
    try:
        assert device_tables(c) is None
        first = {}
        for name, _, _ in K.CASES:
            assert c.env(K.case(name)) == 0, c.err()
            first[name] = device_tables(c)
            assert_tables_equal(first[name], K.reference(name), name)
        for name, _, _ in K.CASES:
            assert c.env(K.case(name)) == 0, c.err()
            assert_tables_equal(device_tables(c), first[name], name + ", second upload")
        assert c.env(None) == 0 and device_tables(c) is None
    finally:
        c.close()


def test_real_size_map_matches_the_oracle(oracle):
    """1024 x 2048, runs of 8 texels and 4 rows: the tables against the oracle's bit for bit (tests/test_env_wide_host.py pins those to
    env_ref.py), then lookup, pdf and sample against the oracle's at IEEE with test_hook_matches_the_reference's tolerances"""
    img = K.real_size_map()
    sc, _, _ = sphere_scene(oracle)
    sc.set_environment(img)
    t = sc.environment_tables()
    c = Ctx.box(math=IEEE)
    try:
        assert c.env(img) == 0, c.err()
        assert_tables_equal(device_tables(c), t, "1024x2048")
        geo = EnvRef(img)                                    # for the mapping alone: texel() and edge_distance()
        d = sphere_directions(20000, 1)
        far = geo.edge_distance(d) > 1e-4
        assert far.sum() > 0.75 * len(d)
        got, exp = c.hook(0, d), sc.env_hook(0, d)
        row, col = geo.texel(d)
        assert np.array_equal(got[far, 3].astype(np.int64), (row * geo.w + col)[far])
        assert np.array_equal(got[far].view(np.uint32), exp[far].view(np.uint32))
        assert np.allclose(c.hook(1, d)[far, 0], sc.env_hook(1, d)[far, 0], rtol=1e-5, atol=0)
        u = sample_inputs()
        got, exp = c.hook(2, u), sc.env_hook(2, u)
        checked = 0
        for (u1, u2), g, e in zip(u, got, exp):
            r, fv = EnvRef._pick(t["marginal"], float(u1))
            _, fu = EnvRef._pick(t["conditional"][r], float(u2))
            if min(fv, 1 - fv, fu, 1 - fu) < 1e-3:
                continue
            assert np.allclose(g[:3], e[:3], atol=1e-5), (u1, u2, g, e)
            assert abs(g[3] - e[3]) <= 1e-4 * e[3], (u1, u2, g, e)
            checked += 1
        assert checked > 3500, checked
    finally:
        c.close()
        sc.close()


# ---- 2. the sample on tables that step down -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [IEEE, FAST])
def test_sample_matches_env_ref(math):
    """the device's bisection, offset and pdf against EnvRef.sample (which walks the tables as the device does) on the sun, faint-sky
    sun, sparse and one-texel maps; the faint-sky sun and the sparse map hold steps down (tests/test_env_wide_host.py)"""
    c = Ctx.box(math=math)
    try:
        u = sample_inputs()
        for name in K.SAMPLED:
            ref = K.reference(name)
            assert c.env(K.case(name)) == 0, c.err()
            s = c.hook(2, u)
            check_samples(name, ref, u, s)
            assert np.all(s[:, 3] > 0), name
            if name == "300x260 one texel":
                check_one_texel(ref, s)
            check_pdf_of_samples(name, ref, lambda x: c.hook(1, x), s)
    finally:
        c.close()


# ---- 3. renders through a wide map ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", [0, 1])
def test_constant_wide_map_is_seen_exactly(light):
    constant_map_is_seen_exactly(1, light, shape=(260, 300))


@pytest.mark.parametrize("light,dl,is_", [(1, True, True), (1, True, False)])
def test_furnace_under_a_wide_map(light, dl, is_):
    furnace(light, dl, is_, shape=(260, 300))


def test_batches_and_partitions_with_a_wide_map():
    batches_and_partitions_with_a_map(1, K.case("260x300 sun"))


# ---- 4. the largest sizes that are accepted ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 16384), (16384, 1)])
def test_longest_row_and_column(shape):
    """runs of 64: the row scan and the marginal scan at the largest width and height"""
    img = K.longest_map(shape)
    c = Ctx.box()
    try:
        assert c.env(img) == 0, c.err()
        assert_tables_equal(device_tables(c), EnvRef(img), "%dx%d" % shape)
    finally:
        c.close()


def test_most_texels():
    """4096 x 8192 = 2^25 texels of 1: the total and pdf_scale against the closed form W sum(sin), and the ends of three tables, each
    run + 9 roundings from 1 (runs of 32 texels, of 16 rows).  Not scanned in Python."""
    h, w = 4096, 8192
    try:
        img = np.ones((h, w, 3), np.float32)
    except MemoryError:
        pytest.skip("no 400 MB of host memory for a 4096 x 8192 map")
    c = Ctx.box()
    try:
        assert c.env(img) == 0, c.err()
        del img
        t = device_tables(c, texels=False)
        lum = float(np.float32(0.2126) + np.float32(0.7152) + np.float32(0.0722))
        total = w * lum * np.sin(np.pi * (np.arange(h) + 0.5) / h).sum()
        assert abs(float(t["total"]) - total) <= 1e-5 * total, (t["total"], total)
        scale = w * h / (2.0 * np.pi ** 2 * total)
        assert abs(float(t["pdf_scale"]) - scale) <= 1e-5 * scale, (t["pdf_scale"], scale)
        assert abs(float(t["marginal"][-1]) - 1.0) <= (K.run_length(h) + 9) * K.U, t["marginal"][-1]
        for r in (0, h - 1):
            assert abs(float(t["conditional"][r, -1]) - 1.0) <= (K.run_length(w) + 9) * K.U, (r, t["conditional"][r, -1])
    finally:
        c.close()

