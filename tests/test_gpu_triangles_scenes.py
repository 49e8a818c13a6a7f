"""pt_query_triangles / pt_query_triangles_any on the hard scenes of tests/query_scenes.py: flat, collapsed and zero-area geometry, no
triangles, a tree of ~96 levels (more than 64 KiB of LDS lane stack) and four magnitudes, through that module's builder and format
matrix.

The sets that are made of the scene's own triangles — `self`, `coplanar`, `wall_touch` — are regenerated per scene (from the box of
the scene it borrows its sets from where it has none), 1 000 queries each, 257 on the 20 000-triangle scenes.  Every count, index and
any byte is held to tritri_ref's brute force, as bits; pt_debug_triangles_visits gives the same counts with visits the tree bounds.
64 bytes of 0xCD behind every output stay."""
import numpy as np
import pytest

from acgpathtracing_amd import _native
import tritri_ref as tt
import query_scenes as qs
import test_gpu_triangles as gt

pytestmark = pytest.mark.gpu

PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
SETS = ("self", "coplanar", "wall_touch")
NAMES = ("flat", "point", "zero_area", "copies") + tuple(qs.MAGNITUDES)
CASES = [c for c in qs.CASES if c[0] in NAMES]
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


def triangles_reference(name):
    """set name -> (records, (counts, prims at 8, any)) of the scene by tritri_ref's brute force: computed once per scene, shared,
    never written"""
    if name not in _cache:
        s = qs.SCENES[name]
        v, idx = s.arrays()[:2]
        sv, sidx = s.set_arrays()[:2]
        out = {}
        for k in SETS:
            recs = tt.query_set(k, sv, sidx.reshape(-1), n=s.n_queries)
            assert recs.shape == (s.n_queries, 12) and tt.searchable(recs).all(), (name, k)
            ref = tt.triangle_records(recs, v, idx.reshape(-1), tt.MAX_PRIMS, chunk=qs._chunk(len(idx)))
            for a in (recs,) + ref:
                a.setflags(write=False)
            out[k] = (recs, ref)
        _cache[name] = out
    return _cache[name]


def _stage(c, name):
    """Every set of the scene on context c, which holds it"""
    st = qs.state_of(c)
    info = c.info()
    before = info.device_bytes
    ref = triangles_reference(name)
    out = {}
    for k, (recs, want) in ref.items():
        n = recs.shape[0]
        gt._check_all(st, recs, want, sizes=(n,), ks=(0, 3, 8), what=(name, k))
        # the counting twin: the same counts, visits the tree bounds
        counts, visits = gt._visits(st, recs)
        assert np.array_equal(counts, want[0]), (name, k)
        assert (visits[:, 1] >= counts).all() and (visits[:, 1] <= info.n_tris).all() and (visits[:, 0] <= info.n_nodes).all(), (name, k, visits.max(axis=0))
        assert info.n_tris == 0 or (visits[:, 0] >= 1).all()
        assert info.n_tris != 0 or not visits.any()
        out[k] = (counts, visits)
    assert c.info().device_bytes == before
    return out


def test_kernel_source_hash_is_the_parents():
    assert _native.hip().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@pytest.mark.parametrize("name,build_mode,tuning", CASES, ids=["%s-mode%s-%s" % (n, m, "default" if t is None else "tuning%d" % t) for n, m, t in CASES])
def test_scene(ctxs, name, build_mode, tuning):
    c = ctxs(name, build_mode, tuning)
    info = c.info()
    v, idx = qs.SCENES[name].arrays()[:2]
    assert info.n_tris == len(idx)
    if name == "copies":                                         # the scene tagged for the stack depth
        assert info.stack_entries * 1024 > 65536 and info.max_depth < info.stack_entries <= 128
    _stage(c, name)
    ref = triangles_reference(name)
    if qs.SCENES[name].sets_of is None:                          # the sets are the scene's own triangles: each names itself
        assert (ref["self"][1][0] >= 1).all(), name
    if name == "copies":                                         # 20 000 triangles in one place: a query takes all of them or none, the lowest indices first
        counts, prims, _ = ref["self"][1]
        assert (counts == 20000).all() and (prims == np.arange(8, dtype=np.uint32)).all()
        assert np.isin(np.concatenate([r[0] for _, r in ref.values()]), (0, 20000)).all()
    if name == "point":                                          # 1 264 triangles collapsed to one point: all or none
        assert np.isin(np.concatenate([r[0] for _, r in ref.values()]), (0, len(idx))).all()
    if name == "flat":                                           # everything in one plane: the in-plane axes decide every pair
        counts = ref["coplanar"][1][0]
        assert (counts != 0).mean() >= 0.25
    if name == "zero_area":                                      # zero-area triangles are found like any other
        zero = qs.zero_area_mask(v, idx)
        named = np.concatenate([r[1][r[1] != 0xFFFFFFFF] for _, r in ref.values()])
        assert zero[named].sum() >= 20


@pytest.mark.parametrize("tuning", [None, 1])
def test_a_scene_without_triangles(ctxs, tuning):
    c = ctxs("empty", None, tuning)
    assert c.info().n_tris == 0
    out = _stage(c, "empty")
    assert all(not counts.any() and not visits.any() for counts, visits in out.values())
