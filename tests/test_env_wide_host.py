"""Environment maps wider and taller than one workgroup of the CDF scan, on the host (no GPU): the CPU oracle's tables against
tests/env_ref.py bit for bit at every shape of tests/env_cases.py (runs of 2 and 3 values, threads that own nothing, a marginal over
more than 256 rows, black rows) and at one map of real size; which of the maps give tables that step down across run boundaries; the
oracle's sample against the reference's on those tables; and how far the distribution the bisection draws from such tables lies from
the exact one, against bounds derived from the scan's rounding count.  tests/test_gpu_env_wide.py holds the device to the same."""
import numpy as np
import pytest

import env_cases as K
from env_cases import assert_tables_equal, check_one_texel, check_pdf_of_samples, check_samples, sample_inputs
from env_ref import EnvRef, decreasing_steps, search, search_many, selection_measure
from test_oracle_env_ggx import sphere_scene

NAMES = [c[0] for c in K.CASES]


@pytest.fixture(scope="module")
def sphere(oracle):
    sc, _, _ = sphere_scene(oracle)
    return sc


# ---- 1. the tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_tables_match_env_ref(sphere, name):
    sphere.set_environment(K.case(name))
    try:
        assert_tables_equal(sphere.environment_tables(), K.reference(name), name)
    finally:
        sphere.set_environment(None)


def test_oracle_tables_match_env_ref_at_real_size(sphere):
    """1024 x 2048, runs of 8 texels and of 4 rows: this pins the oracle that the GPU test compares the device with at this size"""
    img = K.real_size_map()
    sphere.set_environment(img)
    try:
        assert_tables_equal(sphere.environment_tables(), EnvRef(img), "1024x2048")
    finally:
        sphere.set_environment(None)


@pytest.mark.parametrize("shape", [(1, 16384), (16384, 1)])
def test_oracle_tables_match_env_ref_at_the_longest_row_and_column(sphere, shape):
    """runs of 64, the largest width and height pt_set_environment accepts; the GPU test's maps"""
    img = K.longest_map(shape)
    sphere.set_environment(img)
    try:
        assert_tables_equal(sphere.environment_tables(), EnvRef(img), "%dx%d" % shape)
    finally:
        sphere.set_environment(None)


def test_which_maps_step_down():
    """The last entry of run t is sums[t - 1] + v + v ..., the first of run t + 1 starts from sums[t], a Hillis-Steele sum in another
    association: where a run's values vanish against the running sum, the table can step down there.  The sparse map and the sun over
    a faint sky do (measured: 4488 and 8 such steps in their conditional rows); maps of one scale do not.  The sun over a sky of 0.2
    does not either and cannot: each of its weights is at least 8e-5 of its row's sum, a hundred times the scan's rounding error
    ((run + 9) 2^-24 = 6.6e-7 of the sum), so it is the case of a sun inside a run on sorted tables, and the faint sky carries the
    unsorted ones."""
    assert decreasing_steps(K.reference("260x300 sparse").cond) >= 1
    assert decreasing_steps(K.reference("260x300 faint-sky sun").cond) >= 1
    for name, _, uniform in K.CASES:
        if uniform:
            ref = K.reference(name)
            assert decreasing_steps(ref.cond) == 0 and decreasing_steps(ref.marg) == 0, name
    ref = K.reference("260x300 sun")
    assert decreasing_steps(ref.cond) == 0 and decreasing_steps(ref.marg) == 0


def test_bisection_is_searchsorted_on_sorted_tables_only():
    """search() restates the device's walk.  On a sorted table it is numpy's searchsorted(side="right"); on the sparse map's rows the
    two part for some x, which is why the reference cannot use searchsorted there."""
    x = np.random.default_rng(5).uniform(size=2000)
    ref = K.reference("3x700 uniform")
    for row in ref.cond:
        assert np.array_equal(search_many(row, x), np.minimum(np.searchsorted(row, x, side="right"), len(row) - 1))
    assert [search(ref.cond[0], v) for v in x[:50]] == list(search_many(ref.cond[0], x[:50]))
    ref = K.reference("260x300 sparse")
    parted = 0
    for row in ref.cond:
        steps = np.nonzero(np.diff(row) < 0)[0]
        if len(steps):
            v = row[steps + 1].astype(np.float64)        # x at the lower value of a step down
            parted += int((search_many(row, v) != np.minimum(np.searchsorted(row, v, side="right"), len(row) - 1)).sum())
    assert parted > 0


# ---- 2. the sample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.SAMPLED)
def test_oracle_sample_matches_env_ref(sphere, name):
    """Measured on the reference alone: 3980 ... 3983 of these 4000 lie further than 1e-3 from a bin edge on each of the four maps, the
    one-texel map included (one bin on each axis: the offsets are u1 and u2 themselves), so none needs another cap."""
    ref = K.reference(name)
    u = sample_inputs()
    sphere.set_environment(K.case(name))
    try:
        s = sphere.env_hook(2, u)
        check_pdf_of_samples(name, ref, lambda d: sphere.env_hook(1, d), s)
    finally:
        sphere.set_environment(None)
    check_samples(name, ref, u, s)
    assert np.all(s[:, 3] > 0)
    if name == "300x260 one texel":
        check_one_texel(ref, s)


# ---- 3. what the bisection draws from these tables ------------------------------------------------------------------------------------
def table_quality(cdf, weights):
    """(the measure that falls on bins of zero weight, the total-variation distance to weights / sum(weights)) of search() on cdf"""
    m = selection_measure(cdf)
    assert abs(m.sum() - 1.0) < 1e-12
    w = np.asarray(weights, np.float64)
    return float(m[w == 0].sum()), float(0.5 * np.abs(m - w / w.sum()).sum())


def quality_bounds(n):
    """An entry of a table of n values is `run` additions, 8 scan levels and one division away from the exact partial sum over the
    exact total: at most (run + 9) roundings of 2^-24 each, relative to the total.  A bin's measure lies between two entries: off by at
    most 2 (run + 9) 2^-24.  A zero-weight bin inside a run repeats its predecessor's entry and has no width; only the at most 255 run
    starts can give one a width: (a) <= 255 * 2 (run + 9) 2^-24.  Half the sum of n such differences: (b) <= n (run + 9) 2^-24."""
    run = K.run_length(n)
    return 255 * 2 * (run + 9) * K.U, n * (run + 9) * K.U


@pytest.mark.parametrize("name", NAMES)
def test_table_quality_stays_within_the_derived_bounds(name):
    """Measured on these maps: (a) at most 1.5e-6 (the sparse map's rows; bound 3.3e-4), (b) at most 8.0e-6 (700 wide; bound 5.0e-4);
    the marginals: (a) 1.2e-7 (black rows), (b) at most 5.4e-6.  The row totals the marginal scans are its inputs: the distribution it
    is held to is theirs."""
    ref = K.reference(name)
    za, tv = quality_bounds(ref.w)
    worst = [0.0, 0.0]
    for r in range(ref.h):
        if ref.row_total[r] > 0:
            a, b = table_quality(ref.cond[r], ref.weight[r])
            worst = [max(worst[0], a), max(worst[1], b)]
    print("%s: conditional rows, zero-weight measure %.2e (bound %.2e), total variation %.2e (bound %.2e)" % (name, worst[0], za, worst[1], tv))
    assert worst[0] <= za and worst[1] <= tv
    za, tv = quality_bounds(ref.h)
    a, b = table_quality(ref.marg, ref.row_total)
    print("%s: marginal, zero-weight measure %.2e (bound %.2e), total variation %.2e (bound %.2e)" % (name, a, za, b, tv))
    assert a <= za and b <= tv


def test_table_quality_on_long_rows():
    """rows of 2048 and 4096 texels (runs of 8 and 16): a sun over a faint sky and a sparse row, the shapes of a real map's rows"""
    from env_ref import block_scan
    r = np.random.default_rng(41)
    for n in (2048, 4096):
        sun = (r.uniform(0.05, 1.0, n) * 1e-3).astype(np.float32)
        sun[n // 3] = 5e4
        sparse = r.uniform(0.0, 1.0, n).astype(np.float32)
        sparse[r.uniform(size=n) < 0.7] = 0.0
        za, tv = quality_bounds(n)
        for what, w in (("sun", sun), ("sparse", sparse)):
            cdf, total = block_scan(w)
            a, b = table_quality(cdf, w)
            print("%d-texel %s row: %d steps down, zero-weight measure %.2e (bound %.2e), total variation %.2e (bound %.2e)"
                  % (n, what, decreasing_steps(cdf), a, za, b, tv))
            assert a <= za and b <= tv


# ---- 4. the read-back hook without a context ----------------------------------------------------------------------------------------
def test_hook_refuses_a_null_context():
    from acgpathtracing_amd import _native
    L = _native.hip()                                          # loads the library; no GPU is touched
    assert L.pt_debug_environment_tables(None, None, None, None, None, None) == -1
    assert L.pt_last_error(None).startswith(b"pt_debug_environment_tables:")
