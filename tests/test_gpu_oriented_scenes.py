"""pt_query_overlap_oriented, _any and _lists on the scenes of tests/query_scenes.py that break walks: flat, collapsed and zero-area
geometry, no triangles, 20 000 copies of one triangle (a tree of ~96 levels), four magnitudes, through the same builders and both node
formats.

Every count, index, any byte and CSR list is held to oriented_ref's brute force, as bits; pt_debug_overlap_oriented_visits gives the
same counts with visits the tree bounds.  64 bytes of 0xCD behind every output stay.  The sets are oriented_ref's "random" and
"walls_turned", regenerated from the scene's own triangles (the box's for the scene without any and for the collapsed one), 1 000 boxes
each, 257 on the 20 000-triangle scene.  At x1e6 and plus1e7 an admission margin that forgot the scene's magnitude loses triangles."""
import numpy as np
import pytest

from acgpathtracing_amd import _native
import oriented_ref as ob
import query_scenes as qs
import test_gpu_oriented as go

pytestmark = pytest.mark.gpu

NAMES = ("flat", "point", "zero_area", "empty", "copies") + tuple(qs.MAGNITUDES)
CASES = [c for c in qs.CASES if c[0] in NAMES] + [("empty", None, None), ("empty", None, 1)]
SETS = ("random", "walls_turned")
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


def box_reference(name):
    """set -> (boxes, reference) of the scene by oriented_ref's brute force: computed once per scene, shared, never written"""
    if name not in _cache:
        s = qs.SCENES[name]
        v, idx = s.arrays()[:2]
        sv, sidx = s.set_arrays()[:2]          # a scene without a box of its own borrows the box's
        out = {}
        for k in SETS:
            boxes = ob.box_set(k, sv, sidx.reshape(-1), n=s.n_queries)
            assert boxes.shape == (s.n_queries, 16) and ob.searchable(boxes).all(), (name, k)
            boxes.setflags(write=False)
            out[k] = (boxes, go._reference(v, idx.reshape(-1), boxes))
        _cache[name] = out
    return _cache[name]


def _stage(c, name):
    st = qs.state_of(c)
    info = c.info()
    before = info.device_bytes
    ref = box_reference(name)
    for k, (boxes, want) in ref.items():
        n = boxes.shape[0]
        go._check_all(st, boxes, want, sizes=(n,), ks=(0, 8), what=(name, k))
        counts, visits = go.visits(st, boxes)
        assert np.array_equal(counts, want[0]), (name, k)
        assert (visits[:, 1] <= info.n_tris).all() and (visits[:, 0] <= info.n_nodes).all(), (name, k, visits.max(axis=0))
        assert info.n_tris != 0 or not visits.any()
    assert c.info().device_bytes == before
    return ref


def test_kernel_source_hash_is_the_parents():
    assert _native.hip().pt_kernel_source_hash().decode() == go.PARENT_KERNEL_HASH


@pytest.mark.parametrize("name,build_mode,tuning", CASES, ids=["%s-mode%s-%s" % (n, m, "default" if t is None else "tuning%d" % t) for n, m, t in CASES])
def test_scene(ctxs, name, build_mode, tuning):
    c = ctxs(name, build_mode, tuning)
    v, idx = qs.SCENES[name].arrays()[:2]
    assert c.info().n_tris == len(idx)
    ref = _stage(c, name)
    found = {k: r[0] != 0 for k, (_, r) in ref.items()}
    if name == "empty":
        assert not any(f.any() for f in found.values())
        return
    # the sets do what they are there for on this scene, by the reference's own answers (the collapsed scene is one point, which the
    # box's sets rarely hold)
    if name != "point":
        assert found["random"].mean() >= 0.10 and found["walls_turned"].mean() >= 0.25, (name, found["random"].mean(), found["walls_turned"].mean())
    if name == "copies":                                         # 20 000 coincident triangles: a box holds all of them or none
        assert all(set(np.unique(r[0]).tolist()) <= {0, 20000} for _, r in ref.values())


@pytest.mark.parametrize("target", ("flat", "point", "x1e6", "plus1e7"))
def test_refit_into_and_out_of(ctxs, target):
    """The box refitted to the target equals the reference on the target's sets — at x1e6 and plus1e7 the scene box the refit records is
    what the margin's scene term must follow —, and refitted back it answers as before."""
    c = ctxs("box")
    st = qs.state_of(c)
    boxes, want = box_reference(target)["random" if target == "point" else "walls_turned"]      # the few boxes that hold the point are random ones
    assert want[0].any()
    v, idx = qs.box()[:2]
    box_boxes = ob.box_set("walls_turned", v, idx.reshape(-1), n=257)
    box_want = go._reference(v, idx.reshape(-1), box_boxes)
    go._check_all(st, box_boxes, box_want, sizes=(257,), ks=(8,), what=("before",))
    qs._refit(c, qs.SCENES[target].arrays()[0])
    go._check_all(st, boxes, want, sizes=(boxes.shape[0],), ks=(0, 8), what=("refitted to", target))
    qs._refit(c, qs.box()[0])
    go._check_all(st, box_boxes, box_want, sizes=(257,), ks=(8,), what=("refitted back",))
