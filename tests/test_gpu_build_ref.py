"""Build modes 1 and 2 of csrc/lbvh_build.hip held to the sequential references of tests/build_ref.py, word for word: the PLOC tree, the
host insertion pass on it, the device's parallel reinsertion on it; the figures the build keeps about itself (pt_debug_build_stats);
and whether building the same scene again gives the same bytes.  tests/test_build_ref_host.py shows, on the CPU, that these scenes
depend on every rule the comparison is meant to prove.

The trees are read with pt_debug_read_tree under pt_set_tuning(ctx, 0, 1), which keeps the build's own fp32 nodes.  The references
start from the device's triangle records (array 5), so the sort is not under test here (tests/tree_ref.py holds it); the order is also
compared with build_ref.morton_order, the order the CPU tests used, so that what they show about the scenes holds for these builds.
Not reached by any scene here: the two fallbacks that keep the PLOC tree when an optimised one is too deep."""
import ctypes as C

import numpy as np
import pytest

import build_ref as br
import build_scenes as bs
import query_scenes as qs
import tree_ref as tr
from acgpathtracing_amd import _native
from test_gpu_tree import _info, _read, _s82k

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture
def ctxs():
    made = []

    def make(name, mode):
        v, idx, ids, mats = _s82k()[:4] if name == "s82k" else bs.scene(name)
        c = qs._Ctx.from_arrays(v, idx, ids, mats, variant=1, build_mode=mode)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def _stats(c):
    s = _native.BuildStats()
    assert c.L.pt_debug_build_stats(c.ctx, C.byref(s)) == 0, c.err()
    return s


def _leaves(c, name):
    """(lo, hi) of the device's records, and whether their order is the one the CPU tests built their references on"""
    tw = _read(c, 5).reshape(-1, 12)
    lo, hi = tr.record_boxes(tw, _info(c).pad_abs)
    cpu_lo, cpu_hi, cpu_prims = bs.leaves(name)
    same = np.array_equal(tw[:, 9], cpu_prims) and np.array_equal(lo.view(np.uint32), cpu_lo.view(np.uint32)) and np.array_equal(hi.view(np.uint32), cpu_hi.view(np.uint32))
    return lo, hi, same


def _first_difference(got, want):
    got, want = got.reshape(-1, 16), want.reshape(-1, 16)
    if got.shape != want.shape:
        return "shapes %s, %s" % (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    if not bad.size:
        return None
    i = int(bad[0])
    return "%d of %d nodes differ, the first is node %d: children %s, reference %s; words %s" % (
        bad.size, len(got), i, got[i, 12:14].view(np.int32).tolist(), want[i, 12:14].view(np.int32).tolist(), np.flatnonzero(got[i] != want[i]).tolist())


# ---- mode 1 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", bs.MODE1)
def test_ploc_tree_is_the_references(ctxs, name):
    c = ctxs(name, 1)
    lo, hi, same = _leaves(c, name)
    assert same, "the device's Morton order is not build_ref.morton_order's"
    nodes, rounds, height, hashed = bs.ploc(name)
    assert _first_difference(_read(c, 1), nodes) is None, _first_difference(_read(c, 1), nodes)
    s, info = _stats(c), _info(c)
    assert (s.mode, info.mode) == (1, 1)
    assert s.build_iterations == rounds
    assert info.max_depth == height
    assert (s.opt_passes, s.opt_area_before, s.opt_area_after) == (0, 0.0, 0.0)
    assert hashed == (name in ("strip", "copies"))
    print("%s: PLOC, %d triangles, %d rounds, height %d, hashed ties %s, area sum %.9g" % (name, len(lo), rounds, height, hashed, br.area_sum(nodes)))


# ---- mode 2, the host pass ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("passes", [1, None], ids=["ACGPT_OPT_PASSES=1", "default"])
@pytest.mark.parametrize("name", bs.HOST_PASS)
def test_host_pass_tree_is_the_references(ctxs, monkeypatch, name, passes):
    if passes is None:
        monkeypatch.delenv("ACGPT_OPT_PASSES", raising=False)
    else:
        monkeypatch.setenv("ACGPT_OPT_PASSES", str(passes))
    monkeypatch.delenv("ACGPT_OPT_STOP", raising=False)
    c = ctxs(name, 2)
    ploc_tree = _read(ctxs(name, 1), 1).reshape(-1, 16)
    assert len(ploc_tree) + 1 <= tr.K_OPTIMIZE_MAX_TRIS
    limit = () if passes is None else (passes,)
    nodes, done, before, after = bs.host_pass(name, *limit) if np.array_equal(ploc_tree, bs.ploc(name)[0]) else br.insertion_pass(ploc_tree, *limit)
    assert _first_difference(_read(c, 1), nodes) is None, _first_difference(_read(c, 1), nodes)
    s, info = _stats(c), _info(c)
    assert (s.mode, info.mode) == (2, 2)
    assert s.opt_passes == done
    assert F(s.opt_area_before) == F(before) and F(s.opt_area_after) == F(after), (s.opt_area_before, before, s.opt_area_after, after)
    assert info.max_depth == br.height_of(nodes)
    assert s.build_iterations == bs.ploc(name)[1]
    assert after <= before              # (holds for the reference alone on these scenes: tests/test_build_ref_host.py)
    print("%s: host pass, %d passes, area sum %.9g -> %.9g, height %d" % (name, done, before, after, info.max_depth))


# ---- mode 2, the reinsertion on the device -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("iters", [1, 2, None], ids=["ACGPT_RI_ITERS=1", "ACGPT_RI_ITERS=2", "default"])
@pytest.mark.parametrize("name", bs.REINSERTED)
def test_reinserted_tree_is_the_references(ctxs, monkeypatch, name, iters):
    if iters is None:
        monkeypatch.delenv("ACGPT_RI_ITERS", raising=False)
    else:
        monkeypatch.setenv("ACGPT_RI_ITERS", str(iters))
    monkeypatch.delenv("ACGPT_RI_STOP", raising=False)
    cap = br.K_REINSERT_ITERATIONS if iters is None else iters
    c = ctxs(name, 2)
    ploc_tree = _read(ctxs(name, 1), 1).reshape(-1, 16)
    assert len(ploc_tree) + 1 > tr.K_OPTIMIZE_MAX_TRIS
    ref = bs.reinserted(name) if np.array_equal(ploc_tree, bs.ploc(name)[0]) else br.reinsert(ploc_tree)
    assert ref.broken == 0
    s, info = _stats(c), _info(c)
    k = int(s.opt_passes)
    assert (s.mode, info.mode) == (2, 2) and 1 <= k <= cap
    assert _first_difference(_read(c, 1), ref.nodes[k - 1]) is None, "after %d rounds: %s" % (k, _first_difference(_read(c, 1), ref.nodes[k - 1]))
    assert info.max_depth == ref.height[k]
    # the stop rule on the reference's exact sums: every round before the last went on, the last one stopped (or was the cap); the
    # device adds its sum with double atomics in no fixed order, so a ratio within 1e-12 of 0.998 may fall either way
    for r in range(k):
        ratio = ref.area[r + 1] / ref.area[r]
        went_on = ref.winners[r] != 0 and ref.area[r + 1] < ref.area[r] * 0.998
        if abs(ratio - 0.998) <= 1e-12 and ref.winners[r] != 0:
            continue
        assert went_on == (r < k - 1) or (r == k - 1 and k == cap), (r, k, cap, ratio, int(ref.winners[r]))
    # the sums themselves: the float of a float64 sum of the same terms in another order, one float step at the most
    for got, want in ((s.opt_area_before, ref.area[0]), (s.opt_area_after, ref.area[k])):
        assert abs(float(got) - float(F(want))) <= float(np.spacing(F(want))), (got, want)
    assert s.build_iterations == bs.ploc(name)[1]
    print("%s: reinsertion, %d rounds (cap %d), moves %s, area sums %s, height %d" % (name, k, cap, ref.winners[:k].tolist(), ["%.9g" % a for a in ref.area[:k + 1]], info.max_depth))


# ---- repeat builds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s82k", "soup16385"])
def test_repeat_builds_give_the_same_bytes(ctxs, name):
    """Three mode-2 builds of one scene in one process, other contexts made and destroyed in between: the fp32 nodes, the triangle records
    and the shade records are equal byte for byte, and so are the build's figures.  The 82 k-triangle tree is also the reference's,
    numbered depth first."""
    builds, stats = [], []
    for k in range(3):
        c = ctxs(name, 2)
        builds.append({w: _read(c, w) for w in (1, 5, 6)})
        s, info = _stats(c), _info(c)
        stats.append((s.opt_passes, s.build_iterations, s.opt_area_before, s.opt_area_after, info.max_depth))
        other = ctxs("box" if k else "soup2049", k)          # another scene's build in between, and its memory released again
        other.close()
        if k == 1:
            c.close()
    print("%s: three builds: (rounds of reinsertion, PLOC rounds, area before, after, depth) %s" % (name, stats))
    for w in (5, 6, 1):
        for k in (1, 2):
            diff = np.flatnonzero(builds[0][w] != builds[k][w])
            assert not diff.size, "array %d of build %d differs from build 0's in %d words, the first at %d" % (w, k, diff.size, diff[0])
    assert stats[0][:2] == stats[1][:2] == stats[2][:2] and stats[0][4] == stats[1][4] == stats[2][4]
    tw = builds[0][5].reshape(-1, 12)
    lo, hi = tr.record_boxes(tw, _info(c).pad_abs)
    ref = br.build(lo, hi, 2)
    want = br.depth_first(ref["nodes"]) if len(lo) > tr.K_DEPTH_FIRST_TRIS else ref["nodes"]
    assert stats[0][1] == ref["rounds"]
    assert stats[0][0] == ref["passes"] and stats[0][4] == ref["height"], (stats[0], ref["passes"], ref["height"], ref["ri"].winners.tolist(), ref["ri"].area.tolist())
    assert _first_difference(builds[0][1], want) is None, _first_difference(builds[0][1], want)


# ---- the hook ----------------------------------------------------------------------------------------------------------------------

def test_the_stats_hook_refuses_and_changes_nothing():
    L = _native.hip()
    s = _native.BuildStats()
    C.memset(C.byref(s), 0xCD, C.sizeof(s))
    before = bytes(s)
    assert L.pt_debug_build_stats(None, C.byref(s)) != 0
    bare = C.c_void_p()
    assert L.pt_create(C.byref(bare), 0) == 0
    try:
        assert L.pt_debug_build_stats(bare, C.byref(s)) != 0 and b"no scene" in L.pt_last_error(bare)
        assert L.pt_debug_build_stats(bare, None) != 0 and b"null" in L.pt_last_error(bare)
        assert bytes(s) == before
        abi = L.pt_abi_version()
        v, idx, ids, mats = bs.scene("soup17")
        c = qs._Ctx.from_arrays(v, idx, ids, mats, build_mode=2)
        try:
            bytes0 = c.info().device_bytes
            assert L.pt_debug_build_stats(c.ctx, None) != 0 and b"null" in c.err()
            assert L.pt_debug_build_stats(c.ctx, C.byref(s)) == 0
            assert s.mode == 2 and s.opt_passes >= 1 and s.build_iterations == bs.ploc("soup17")[1] and s.opt_ms >= 0
            assert c.info().device_bytes == bytes0 and L.pt_abi_version() == abi
        finally:
            c.close()
    finally:
        L.pt_destroy(bare)
