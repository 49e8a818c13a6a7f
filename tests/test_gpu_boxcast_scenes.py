"""pt_query_box_cast / pt_query_box_cast_any on the scenes of tests/query_scenes.py that break walks: flat, collapsed and zero-area
geometry, no triangles, 20 000 copies of one triangle (a tree of ~96 levels), four magnitudes, through the same builders and both node
formats.

Every record is held to boxcast_ref's brute force, as bits, and every byte to the records; pt_debug_box_cast_visits gives the same
records in both modes with visits the tree bounds.  64 bytes of 0xCD behind every output stay.  The sets are boxcast_ref's "aimed" and
"links", regenerated from the scene's own triangles (the box's for the scene without any), 1 000 casts each, 257 on the
20 000-triangle scene: boxes that meet their target with a face, an edge or a corner, and long thin ones, where a child box inflated by
too little, a bound on the best t widened by too little or an extra axis that trusts its own direction loses the winner."""
import numpy as np
import pytest

from acgpathtracing_amd import _native
import boxcast_ref as cr
import query_scenes as qs
import test_gpu_boxcast as gc

pytestmark = pytest.mark.gpu

NAMES = ("flat", "point", "zero_area", "empty", "copies") + tuple(qs.MAGNITUDES)
CASES = [c for c in qs.CASES if c[0] in NAMES] + [("empty", None, None), ("empty", None, 1)]
_cache = {}


@pytest.fixture
def ctxs():
    made = []

    def make(name, build_mode=None, tuning=None):
        v, idx, ids, mats = qs.SCENES[name].arrays()
        c = qs._Ctx.from_arrays(v, idx, ids, mats, build_mode=build_mode, variant=tuning)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def cast_reference(name):
    """set -> (casts, records) of the scene by boxcast_ref's brute force: computed once per scene, shared, never written"""
    if name not in _cache:
        s = qs.SCENES[name]
        v, idx, ids = s.arrays()[:3]
        sv, sidx = (s.set_arrays() if len(idx) == 0 else s.arrays())[:2]          # a scene without triangles borrows the box's
        out = {}
        for k in cr.SCENE_SETS:
            casts = cr.cast_set(k, sv, sidx.reshape(-1), n=s.n_queries)
            assert casts.shape == (s.n_queries, 20) and cr.castable(casts).all(), (name, k)
            ref = cr.box_records(casts, v, idx.reshape(-1), ids)
            casts.setflags(write=False); ref.setflags(write=False)
            out[k] = (casts, ref)
        _cache[name] = out
    return _cache[name]


def _stage(c, name):
    st = qs.state_of(c)
    info = c.info()
    before = info.device_bytes
    ref = cast_reference(name)
    for k, (casts, want) in ref.items():
        d = gc._DeviceCasts(st, casts)
        try:
            rec, blocked = d.cast().copy(), d.blocked().copy()
            twin, visits = d.visits(0)
            twin1, visits1 = d.visits(1)
        finally:
            d.free()
        assert np.array_equal(rec, want), (name, k) + gc._diff(rec, want)
        assert np.array_equal(blocked, cr.blocked_of(want)), (name, k)
        assert np.array_equal(twin, want) and np.array_equal(twin1, want), (name, k)
        assert (visits1[:, 1] <= info.n_tris).all() and (visits1[:, 0] <= info.n_nodes).all(), (name, k, visits1.max(axis=0))
        assert (visits[:, 0] <= visits1[:, 0]).all() and (visits[:, 1] <= visits1[:, 1]).all(), (name, k)
        assert info.n_tris != 0 or not visits1.any()
    assert c.info().device_bytes == before
    return ref


def test_kernel_source_hash_is_the_parents():
    assert _native.hip().pt_kernel_source_hash().decode() == gc.PARENT_KERNEL_HASH


@pytest.mark.parametrize("name,build_mode,tuning", CASES, ids=["%s-mode%s-%s" % (n, m, "default" if t is None else "tuning%d" % t) for n, m, t in CASES])
def test_scene(ctxs, name, build_mode, tuning):
    c = ctxs(name, build_mode, tuning)
    v, idx = qs.SCENES[name].arrays()[:2]
    assert c.info().n_tris == len(idx)
    ref = _stage(c, name)
    hits = {k: r[:, 1] != 0xFFFFFFFF for k, (_, r) in ref.items()}
    if name == "empty":
        assert not any(h.any() for h in hits.values())
        return
    # the sets do what they are there for on this scene, by the reference's own answers
    assert hits["aimed"].mean() >= 0.9 and hits["links"].mean() >= 0.25, (name, hits["aimed"].mean(), hits["links"].mean())
    if name in ("copies", "point"):                              # exact ties, or 1 264 triangles collapsed to one point: triangle 0 or nothing
        assert all((r[h, 1] == 0).all() for h, (_, r) in zip(hits.values(), ref.values()))
    if name == "zero_area":                                      # zero-area triangles are hit like any other: by their edges and vertices
        zero = qs.zero_area_mask(v, idx)
        assert sum(int(zero[r[h, 1]].sum()) for h, (_, r) in zip(hits.values(), ref.values())) >= 20


@pytest.mark.parametrize("target", ("flat", "point", "x1e6", "plus1e7"))
def test_refit_into_and_out_of(ctxs, target):
    """The box refitted to the target equals the reference on the target's sets — at x1e6 and plus1e7 the scene box the refit records is
    what the widenings' scene term must follow —, and refitted back it answers as before."""
    c = ctxs("box")
    st = qs.state_of(c)
    box_casts = cr.cast_set("aimed", *qs.box()[:2], n=257)
    before = gc._query(st, box_casts)[0]
    qs._refit(c, qs.SCENES[target].arrays()[0])
    for k in cr.SCENE_SETS:
        casts, want = cast_reference(target)[k]
        rec, blocked = gc._query(st, casts)
        assert np.array_equal(rec, want), (target, k) + gc._diff(rec, want)
        assert np.array_equal(blocked, cr.blocked_of(want))
    qs._refit(c, qs.box()[0])
    assert np.array_equal(gc._query(st, box_casts)[0], before)
    v, idx, ids = qs.box()[:3]
    assert np.array_equal(before, cr.box_records(box_casts, v, idx.reshape(-1), ids))
