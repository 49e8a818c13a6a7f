"""pt_query_nearest_k / pt_query_within_any on the scenes of tests/query_scenes.py: the box under every builder, the icosphere, 20 000
coincident copies (every list is triangles 0 .. k - 1 at one d2, a tree of ~96 levels), one and two triangles (trailing misses), no
triangles, flat, collapsed and zero-area geometry (a NaN d2 is neither listed nor counted) and four magnitudes, through that module's
builder and format matrix.

The point sets are that module's, generated per scene from the scene's own box, 1 000 points each, 257 on the 20 000-triangle
scenes, at max_radius = +inf and at each set's finite radius.  Every list (k = 1, 3, 8 with counts and without), every count and
every byte is held to tests/nearest_k_ref.py's brute force, record 0 to pt_query_nearest on the device; the counting twin gives the
same records with visits the tree bounds; the box refitted into each hard state equals the reference of that state, which the state
built fresh equals too.  64 bytes of 0xCD in front of and behind every output stay."""
import numpy as np
import pytest

from acgpathtracing_amd import _native
import nearest_k_ref as kr
import nearest_ref as nr
import query_scenes as qs
import test_gpu_nearest_k as gk

pytestmark = pytest.mark.gpu

PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
MISS = qs.MISS
KS = (1, 3, 8)
NAMES = ("box", "sphere", "copies", "one_triangle", "two_triangles", "flat", "point", "zero_area") + tuple(qs.MAGNITUDES)
# one builder for the two big scenes (the builders are test_gpu_query_scenes' business), every format the matrix has
CASES = [c for c in qs.CASES if c[0] in NAMES and (c[0] not in ("box", "sphere") or c[1] == 2)]
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


def lists_reference(name):
    """set name -> (points [n, 3], radius, reference at +inf, reference at the radius), each reference (records [n, 8, 8], counts,
    bytes) of the scene by nearest_k_ref's brute force, the distances computed once for both radii: computed once per scene, shared,
    never written"""
    if name not in _cache:
        v, idx, ids, _ = qs.SCENES[name].arrays()
        out = {}
        for k, (pts, r) in qs.point_sets(name).items():
            ref_inf, ref_r = kr.nearest_k_radii(pts, (np.inf, r), v, idx.reshape(-1), ids, chunk=qs._chunk(len(idx)))
            for a in ref_inf + ref_r:
                a.setflags(write=False)
            out[k] = (pts, np.float32(r), ref_inf, ref_r)
        _cache[name] = out
    return _cache[name]


def _stage(c, name):
    """Every set of scene `name` on context c, which holds it (built or refitted).  Returns set -> the twin's visits at +inf, k = 8
    without counts"""
    st = qs.state_of(c)
    info = c.info()
    before = info.device_bytes
    out = {}
    for k, (pts, r, ref_inf, ref_r) in lists_reference(name).items():
        n = pts.shape[0]
        for rad, ref in ((np.inf, ref_inf), (r, ref_r)):
            d = gk.Device(st, nr.with_radius(pts, rad))
            try:
                gk.check_all_forms(d, ref, n, ks=KS, what=(name, k, float(rad)))
                if np.isinf(rad):
                    # the counting twin: the same records, visits the tree bounds
                    rec, _, visits = d.lists(8, False, visits=True)
                    assert np.array_equal(rec, ref[0]), (name, k) + gk._diff(rec, ref[0])
                    rec, cnt, all_visits = d.lists(8, True, visits=True)
                    assert np.array_equal(rec, ref[0]) and np.array_equal(cnt, ref[1])
                    hit, hit_visits = d.within(visits=True)
                    assert np.array_equal(hit, ref[2])
                    for vis in (visits, all_visits, hit_visits):
                        assert (vis[:, 0] <= info.n_nodes).all() and (vis[:, 1] <= info.n_tris).all(), (name, k, vis.max(axis=0))
                        assert info.n_tris != 0 or not vis.any()
                    assert (visits <= all_visits).all() and (hit_visits <= all_visits).all()
                    searchable = nr.searchable(d.points)
                    assert info.n_tris == 0 or (all_visits[searchable, 1] == info.n_tris).all()      # with counts at +inf: the whole tree
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
    n_tris = len(idx)
    assert info.n_tris == n_tris
    if name == "copies":                                         # the scene tagged for the stack depth
        assert info.stack_entries * 1024 > 65536 and info.max_depth < info.stack_entries <= 128
    visits = _stage(c, name)
    ref = lists_reference(name)
    found_inf = np.concatenate([r[2][2] for r in ref.values()])
    assert found_inf.all(), name                                 # without a radius every point finds something
    if name not in ("point", "one_triangle", "two_triangles"):   # the finite radii still split the sets
        found_r = np.concatenate([r[3][2] for r in ref.values()]) != 0
        assert found_r.mean() >= 0.2 and (~found_r).mean() >= 0.1, (name, found_r.mean())
    if name in ("copies", "point"):                              # exact ties in d2: every list is triangles 0 .. 7 at one distance
        for r in ref.values():
            assert (r[2][0][:, :, 1] == np.arange(8, dtype=np.uint32)[None]).all() and (r[2][0][:, :, 0] == r[2][0][:, :1, 0]).all(), name
            assert (r[2][1] == n_tris).all()
    if name in ("one_triangle", "two_triangles"):                # trailing misses, and the count says how many are real
        for r in ref.values():
            assert (r[2][1] == n_tris).all() and (r[2][0][:, :n_tris, 1] != MISS).all()
            assert np.array_equal(r[2][0][:, n_tris:], kr.miss_lists(len(r[2][1]), 8 - n_tris))
    if name == "one_triangle":                                   # the second child's NaN bound is never admitted: exactly one triangle tested
        assert all((vis[:, 1] == 1).all() and (vis[:, 0] == 1).all() for vis in visits.values())
    if name == "zero_area":                                      # a NaN d2 is neither listed nor counted; the other zero-area triangles are found by their edges
        zero = qs.zero_area_mask(v, idx)
        counts_inf = np.concatenate([r[2][1] for r in ref.values()])
        assert (counts_inf < n_tris).any() and (counts_inf >= n_tris - zero.sum()).all()
        named = np.concatenate([r[2][0][:, :, 1].reshape(-1) for r in ref.values()])
        assert zero[named[named != MISS]].sum() >= 20


@pytest.mark.parametrize("tuning", [None, 1])
def test_a_scene_without_triangles(ctxs, tuning):
    c = ctxs("empty", None, tuning)
    assert c.info().n_tris == 0
    visits = _stage(c, "empty")
    ref = lists_reference("empty")
    for r in ref.values():
        assert np.array_equal(r[2][0], kr.miss_lists(len(r[2][1]), 8)) and not r[2][1].any() and not r[2][2].any()
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
