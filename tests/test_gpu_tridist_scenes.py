"""pt_query_triangle_distance on the scenes of tests/query_scenes.py: the box under every builder, the icosphere with the tangent
triangles on which the scene's vertices and the edge pairs win, 20 000 coincident copies (exact ties, a tree of ~96 levels), one and
two triangles, no triangles, flat, collapsed and zero-area geometry and four magnitudes, through that module's builder and format
matrix.

The five query sets of tests/tridist_ref.py are generated per scene from the scene's own box (from the box of the scene it borrows its
sets from where it has none), 1 000 queries each, 257 on the 20 000-triangle scenes, at max_radius = +inf and at each set's finite
radius; the icosphere runs its tangent triangles alone.  All 48 bytes of every record are held to tridist_ref's brute force, computed in chunks;
pt_debug_triangle_distance_visits gives the same records with visits the tree bounds; the box refitted into each hard state equals
the reference of that state, which the state built fresh equals too.  64 bytes of 0xCD behind every output stay."""
import numpy as np
import pytest

from acgpathtracing_amd import _native
import query_scenes as qs
import tridist_ref as tr
import test_gpu_tridist as gt

pytestmark = pytest.mark.gpu

PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
MISS = qs.MISS
NAMES = ("box", "sphere", "copies", "one_triangle", "two_triangles", "flat", "point", "zero_area", "scaled") + tuple(qs.MAGNITUDES)
# one builder for the two big scenes (the builders are test_gpu_query_scenes' business), every format the matrix has
CASES = [c for c in qs.CASES if c[0] in NAMES and (c[0] not in ("box", "sphere") or c[1] == 2)] + [("scaled", None, None)]
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
    """set name -> (triangles [n, 9], radius, records at +inf, records at the radius) of the scene by tridist_ref's brute force:
    computed once per scene, shared, never written"""
    if name not in _cache:
        s = qs.SCENES[name]
        v, idx, ids, _ = s.arrays()
        sv, sidx = s.set_arrays()[:2]
        lo, hi, c, scale = qs._extent(sv, sidx)
        out = {}
        # the icosphere's 20 480 distinct triangles make every set cost seconds of brute force: it runs the set it is there for
        names = ("tangent",) if name == "sphere" else tr.QUERY_SETS
        for k in names:
            if k == "tangent":
                tris, r = tr.tangent_triangles(sv, sidx, n=s.n_queries), np.float32(0.02) * scale
            else:
                tris, r = tr.query_set(k, sv, sidx, n=s.n_queries), tr.set_radius(k, sv, sidx)
            rec_inf, d2 = tr.triangle_distance_records(tr.as_records(tris, np.inf), v, idx.reshape(-1), ids, chunk=max(4, qs._chunk(len(idx)) // 48), return_d2=True)
            rec_r = tr.records_within(rec_inf, d2, r)
            for a in (tris, rec_inf, rec_r):
                a.setflags(write=False)
            out[k] = (tris, np.float32(r), rec_inf, rec_r)
        _cache[name] = out
    return _cache[name]


def _stage(c, name):
    """Every set of scene `name` on context c, which holds it (built or refitted)"""
    st = qs.state_of(c)
    info = c.info()
    before = info.device_bytes
    out = {}
    for k, (tris, r, ref_inf, ref_r) in triangles_reference(name).items():
        for rad, ref in ((np.inf, ref_inf), (r, ref_r)):
            g = tr.as_records(tris, rad)
            d = gt._DeviceTriangles(st, g)
            try:
                rec = d.query()
                assert np.array_equal(rec, ref), (name, k, float(rad)) + gt._diff(rec, ref)
                if np.isinf(rad):
                    # the counting twin: the same records, visits the tree bounds
                    rec2, visits = d.visits(0)
                    assert np.array_equal(rec2, ref), (name, k) + gt._diff(rec2, ref)
                    assert (visits[:, 0] <= info.n_nodes).all() and (visits[:, 1] <= info.n_tris).all(), (name, k, visits.max(axis=0))
                    assert info.n_tris == 0 or (visits[:, 1] >= 1).all()
                    assert info.n_tris != 0 or not visits.any()
                    out[k] = visits
            finally:
                d.free()
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
    visits = _stage(c, name)
    ref = triangles_reference(name)
    found_inf = np.concatenate([r[2][:, 1] != MISS for r in ref.values()])
    assert found_inf.all(), name                                 # without a radius every query finds something
    if name not in ("point", "one_triangle", "two_triangles"):   # the finite radii still split the sets
        found_r = np.concatenate([r[3][:, 1] != MISS for r in ref.values()])
        assert found_r.mean() >= 0.2 and (~found_r).mean() >= 0.1, (name, found_r.mean())
    if name == "sphere":                                         # the set the scene's vertices and the edge pairs win
        groups = np.bincount(tr.group_of(ref["tangent"][2].view(np.float32)[:, 2]), minlength=5) / len(ref["tangent"][2])
        assert groups[1] >= 0.20 and groups[2] >= 0.20, groups
    if name in ("copies", "point"):                              # exact ties in d2: every record names triangle 0
        assert all((r[2][:, 1] == 0).all() for r in ref.values()), name
    if name == "one_triangle":                                   # the second child's NaN bound is never admitted: exactly one triangle tested
        assert all((vis[:, 1] == 1).all() and (vis[:, 0] == 1).all() for vis in visits.values())
    if name == "zero_area":                                      # zero-area triangles are found like any other: their edges answer
        zero = qs.zero_area_mask(v, idx)
        named = np.concatenate([r[2][:, 1] for r in ref.values()])
        assert zero[named].sum() >= 20


@pytest.mark.parametrize("tuning", [None, 1])
def test_a_scene_without_triangles(ctxs, tuning):
    c = ctxs("empty", None, tuning)
    assert c.info().n_tris == 0
    visits = _stage(c, "empty")
    ref = triangles_reference("empty")
    assert all(np.array_equal(r[2], tr.miss_records(len(r[2]))) for r in ref.values())
    assert all(not vis.any() for vis in visits.values())


@pytest.mark.parametrize("target", qs.REFIT_TARGETS)
def test_refit_into_and_out_of(ctxs, target):
    """The box refitted into each hard state answers as that state's reference says — which the state built fresh equals too
    (test_scene) —, and refitted back it answers as the box.  At x1e6 / x1e-6 the scene box the refit records is what the
    threshold's absolute term must follow."""
    c = ctxs("box", 2, None)
    qs._refit(c, qs.SCENES[target].arrays()[0])
    _stage(c, target)
    qs._refit(c, qs.box()[0])
    _stage(c, "box")
