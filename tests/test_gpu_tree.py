"""The built BVH read back from the device (pt_debug_read_tree) and held, node by node, to its triangles by tests/tree_ref.py: every
builder, the scenes of tests/query_scenes.py, the block boundaries of the 256-thread build kernels and kOptimizeMaxTris from both sides,
the depth-first numbering above kDepthFirstTris; the fp32 nodes regenerated from the fp16 topology against the build's own; the tree
after pt_update_vertices(PT_UPDATE_REFIT) and after pt_update_materials; and the hook's own refusals.

The arrays come into existence by the paths the library has: pt_set_tuning(ctx, 0, 1) keeps the build's fp32 nodes, one pt_trace_closest
ray regenerates them, pt_bench_traversal with one ray and node_format 1 / 3 / 4 ensures the four-wide records, the {lo, hi} nodes, the
centre / half-extent nodes.

After a refit pt_update_vertices settles the scene as pt_set_scene does: the one node array the render variant reads is held (the fp32
nodes under pt_set_tuning(ctx, 0, 1); the centre / half-extent nodes, encoded from the refitted fp32 nodes, under the default variant)
and every other derived array is gone until its first use.

Each case prints, per array format, the largest distance of a device plane from the exact one as a share of tree_ref's bound."""
import ctypes as C
import functools

import numpy as np
import pytest

import query_scenes as qs
import tree_ref as tr
from acgpathtracing_amd import _native
from test_gpu_refit_edges import _jitter_and_move

pytestmark = pytest.mark.gpu

F = np.float32
WORDS = {1: 16, 2: 8, 3: 8, 4: 12, 5: 12, 6: 4}          # 32-bit words per element
NODE_ARRAYS = (1, 2, 3)
ONE_RAY = np.array([[278.0, 273.0, -800.0, 0.0, 0.0, 1.0, 0.01, 1e16]], F)


@pytest.fixture
def ctxs():
    made = []

    def make(v, idx, ids, mats, **kw):
        c = qs._Ctx.from_arrays(v, idx, ids, mats, **kw)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


# ---- reading -----------------------------------------------------------------------------------------------------------------------

def _info(c):
    ti = _native.TreeInfo()
    assert c.L.pt_debug_read_tree(c.ctx, 0, None, 0, C.byref(ti)) == 0, c.err()
    return ti


def _held(c):
    h = _info(c).held
    return {w for w in range(1, 7) if h >> (w - 1) & 1}


def _read(c, what):
    ti = _info(c)
    count = ti.n_wrecs if what == 4 else ti.n_tris if what in (5, 6) else ti.n_nodes
    out = np.zeros(count * WORDS[what], np.uint32)
    assert c.L.pt_debug_read_tree(c.ctx, what, out.ctypes.data, out.nbytes, None) == 0, c.err()
    return out


def _read_held(c):
    return {w: _read(c, w) for w in sorted(_held(c))}


def _morton(c):
    n = _info(c).n_tris
    codes, prims = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert c.L.pt_read_morton(c.ctx, codes.ctypes.data, prims.ctypes.data) == 0, c.err()
    return codes, prims


def _ensure_all(c):
    """Every array the scene can hold, by the library's own paths"""
    c.trace(ONE_RAY)                    # the fp32 nodes
    for fmt in (3, 4, 1):               # {lo, hi}, centre / half extent, four-wide
        c.bench(ONE_RAY, fmt)
    assert _held(c) == {1, 2, 3, 4, 5, 6}


def _validate(c, v, idx, ids, label, depth_first=None):
    """Brings every array into existence, reads all six and validates them together; returns (arrays, info)"""
    before = _read_held(c)
    _ensure_all(c)
    arrays = _read_held(c)
    for w, a in before.items():
        assert np.array_equal(a, arrays[w]), "array %d changed when the others were brought back" % w
    info = tr.Info.of(_info(c))
    bi = c.info()
    assert (bi.n_tris, bi.n_nodes, bi.max_depth) == (info.n_tris, info.n_nodes, info.max_depth)
    vs = tr.validate(arrays, info, v, idx, ids, morton=_morton(c), stack_entries=bi.stack_entries,
                     depth_first=(info.n_tris > tr.K_DEPTH_FIRST_TRIS) if depth_first is None else depth_first)
    print("%s: mode %d, %d triangles, depth %d, wide depth %d; slack as a share of the bound: %s"
          % (label, info.mode, info.n_tris, info.max_depth, info.wide_depth, ", ".join("%s %.4f" % kv for kv in sorted(vs.slack.items()))))
    assert vs == [], "%s: %d violations: %s" % (label, len(vs), vs[:8])
    return arrays, info


# ---- scenes ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _soup(n):
    """A seeded soup of n small triangles in the Cornell box's volume"""
    rng = np.random.default_rng(1000 + n)
    t = rng.uniform(20.0, 530.0, (n, 1, 3)) + rng.normal(scale=4.0, size=(n, 3, 3))
    v = np.zeros((3 * n, 4), F)
    v[:, :3] = t.reshape(-1, 3)
    mats = qs.box()[3]
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), (np.arange(n) % len(mats)).astype(np.uint32), mats


@functools.lru_cache(maxsize=None)
def _s82k():
    """(verts, idx, mat_ids, materials, jittered verts) of the 82 k-triangle stress scene; the OBJ it is read from is removed again"""
    import os
    import tempfile
    with tempfile.TemporaryDirectory(prefix="tree_s82k_") as d:
        path = os.path.join(d, "s82k.obj")
        v, idx, ids, mats = qs._stress(path, n_spheres=4, subdiv=5)
        vn = _jitter_and_move(path, v)
    assert len(idx) == 4 * 20480 + 12 > tr.K_DEPTH_FIRST_TRIS
    return v, idx, ids, mats, vn


def _scene(name):
    if name == "s82k":
        return _s82k()[:4]
    if name.startswith("soup"):
        return _soup(int(name[4:]))
    return qs.SCENES[name].arrays()


BUILT = ([("box", m) for m in (0, 1, 2)] + [("sphere", m) for m in (0, 1, 2)] +
         [("copies", 0), ("copies_lifted", 0)] +          # the radix tree over 20 000 equal Morton codes: k_hierarchy's tie rule
         [(name, None) for name in ("copies", "copies_lifted", "one_triangle", "two_triangles", "flat", "point", "zero_area") + tuple(qs.MAGNITUDES)] +
         [("s82k", 1), ("s82k", 2)] + [("soup%d" % n, 2) for n in (255, 256, 257, 16384, 16385)])


@pytest.mark.parametrize("name,build_mode", BUILT, ids=["%s-mode%s" % (n, "default" if m is None else m) for n, m in BUILT])
def test_built_tree(ctxs, name, build_mode):
    v, idx, ids, mats = _scene(name)
    c = ctxs(v, idx, ids, mats, build_mode=build_mode)
    held = _held(c)
    if name in qs.SCENES:           # the one node array of the scene's default variant, the records and nothing else
        assert held == {1 if qs.DEFAULT_FORMAT.get(name, 11) == 0 else 3, 5, 6}, held
    assert len(held & set(NODE_ARRAYS)) == 1 and 4 not in held
    arrays, info = _validate(c, v, idx, ids, "%s mode %s" % (name, build_mode))
    n = len(idx)
    # the mode the tree was really built in: tree_ref holds a mode-0 tree to the radix tree, so the Karras checks ran where 0 was asked
    # for; the default is mode 2, also for `copies`, whose hashed pairing keeps the tree within the lane stacks (no fallback to mode 0)
    assert info.mode == (2 if build_mode is None else build_mode)
    if name == "copies":
        codes = _morton(c)[0]
        assert (codes == codes[0]).all()                         # 20 000 equal codes
    if build_mode == 2 and n > tr.K_OPTIMIZE_MAX_TRIS:
        # past kOptimizeMaxTris the host's insertion pass is not run: mode 2 is PLOC plus the parallel reinsertion on the device, and
        # max_depth comes from the reinsertion's own heights (validated above against the longest path)
        other = ctxs(v, idx, ids, mats, build_mode=1)
        other.trace(ONE_RAY)
        assert tr.Info.of(_info(other)).mode == 1
        assert not np.array_equal(tr.children_of(1, _read(other, 1))[0], tr.children_of(1, arrays[1])[0])      # the reinsertion ran: not the PLOC tree
    if name == "flat":
        hs = info.hspace
        # the flat axis keeps a scale of its own: the triangles' pad (1e-5 of the coordinate) is above 2^-20 of the longest half extent,
        # so the 2^-20 fallback of build_impl is not reached; every face of the thin scene box sits at |g| = 1023
        assert 0 < hs[5] < hs[3] * 1e-4 and hs[4] != hs[5]
    if name == "point":
        assert np.all(info.scene_hi - info.scene_lo < 1e-2)
    if name == "one_triangle":
        assert info.n_nodes == 1 and info.max_depth == 1


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_regenerated_fp32_nodes_are_the_builds_own(ctxs, name):
    v, idx, ids, mats = _scene(name)
    kept = ctxs(v, idx, ids, mats, variant=1)
    assert _held(kept) == {1, 5, 6}
    c = ctxs(v, idx, ids, mats)
    assert _held(c) == {3, 5, 6}
    c.trace(ONE_RAY)
    assert _held(c) == {1, 3, 5, 6}
    a, b = _read(kept, 1), _read(c, 1)
    assert a.size == b.size and np.array_equal(a, b), np.flatnonzero(a != b)[:8] // 16
    for w in (5, 6):
        assert np.array_equal(_read(kept, w), _read(c, w))


# ---- refit -------------------------------------------------------------------------------------------------------------------------

def _refit_cases():
    """(scene, target, build mode)"""
    return ([("box", kind, None) for kind in ("rigid", "jitter", "scale", "drag")] + [("box", t, None) for t in qs.REFIT_TARGETS] +
            [("s82k", "jitter", 1), ("s82k", "jitter", 2)])


def _refit_target(name, kind):
    if name == "s82k":
        return _s82k()[4]
    v = qs.box()[0]
    return qs.SCENES[kind].arrays()[0] if kind in qs.SCENES else qs._deformations(v)[kind]


@pytest.mark.parametrize("holding", ["fp16", "fp32"])
@pytest.mark.parametrize("name,kind,build_mode", _refit_cases(), ids=["%s-%s-mode%s" % (n, k, "default" if m is None else m) for n, k, m in _refit_cases()])
def test_refit(ctxs, name, kind, build_mode, holding):
    v, idx, ids, mats = _scene(name)
    vn = _refit_target(name, kind)
    assert vn.shape == v.shape
    # fp16: the refit reads the topology from the centre / half-extent nodes and writes a new fp32 array; fp32: it rewrites the nodes in place
    what = 3 if holding == "fp16" else 1
    c = ctxs(v, idx, ids, mats, variant=None if holding == "fp16" else 1, build_mode=build_mode)
    assert _held(c) == {what, 5, 6}
    kids0, raw0 = tr.children_of(what, _read(c, what))
    depth0 = _info(c).max_depth
    qs._refit(c, vn)
    held = _held(c)
    # fp32: only the fp32 array, rewritten in place.  fp16: the variant is chosen anew for the new geometry, as for a fresh scene of
    # it — the fp32 nodes for `zero_area` (query_scenes.DEFAULT_FORMAT), the centre / half-extent nodes for every other target —,
    # its array encoded from the refitted fp32 nodes, and nothing derived from the old boxes is left
    now = 1 if holding == "fp32" or qs.DEFAULT_FORMAT.get(kind, 11) == 0 else 3
    assert held == {now, 5, 6}, held
    kids1, raw1 = tr.children_of(now, _read(c, now))
    assert np.array_equal(kids0, kids1)
    if now == what:
        assert np.array_equal(raw0, raw1)                 # byte for byte
    assert _info(c).max_depth == depth0
    arrays, info = _validate(c, vn, idx, ids, "%s (mode %s) refitted to %s holding %s" % (name, build_mode, kind, holding))      # each derived format brought back, over the new vertices
    assert np.array_equal(tr.children_of(what, arrays[what])[1], raw0) and info.max_depth == depth0


# ---- material edits ----------------------------------------------------------------------------------------------------------------

def test_material_edit_changes_the_material_words_only(ctxs):
    v, idx, ids, mats = _scene("box")
    c = ctxs(v, idx, ids, mats)
    before, _ = _validate(c, v, idx, ids, "box before the edit")
    new_ids = ((ids.astype(np.int64) + 1 + np.arange(len(ids)) % 2) % len(mats)).astype(np.uint32)
    assert (new_ids != ids).all()
    c.update_materials(list(mats), new_ids)
    assert 4 not in _held(c)                                 # the four-wide records carried the old material words
    after, _ = _validate(c, v, idx, new_ids, "box after the edit")
    for w in NODE_ARRAYS:
        assert np.array_equal(before[w], after[w]), w
    t0, t1 = before[5].reshape(-1, 12), after[5].reshape(-1, 12)
    prim = t1[:, 9].astype(np.int64)
    other = np.arange(12) != 10
    assert np.array_equal(t0[:, other], t1[:, other]) and np.array_equal(t1[:, 10], new_ids[prim])
    s0, s1 = before[6].reshape(-1, 4), after[6].reshape(-1, 4)
    assert np.array_equal(s0[:, 0:3], s1[:, 0:3])
    bsdf = np.array([m.bsdfType for m in mats], np.uint32)
    lit = np.array([not (m.emission.x == 0 and m.emission.y == 0 and m.emission.z == 0) for m in mats])
    want = new_ids[prim] | ((bsdf[new_ids[prim]] & 3) << 24) | (lit[new_ids[prim]].astype(np.uint32) << 26)
    assert np.array_equal(s1[:, 3], want)
    w0, w1 = before[4].reshape(-1, 12), after[4].reshape(-1, 12)
    assert w0.shape == w1.shape
    diff = np.argwhere(w0 != w1)
    assert len(diff) and (diff[:, 1] == 10).all()            # triangle records' material words and nothing else


# ---- the hook itself ---------------------------------------------------------------------------------------------------------------

def test_the_hook_refuses_and_changes_nothing(ctxs):
    L = _native.hip()
    ti = _native.TreeInfo()
    buf = np.zeros(1 << 16, np.uint32)
    assert L.pt_debug_read_tree(None, 0, None, 0, C.byref(ti)) != 0
    bare = C.c_void_p()
    assert L.pt_create(C.byref(bare), 0) == 0
    try:
        assert L.pt_debug_read_tree(bare, 0, None, 0, C.byref(ti)) != 0 and b"no scene" in L.pt_last_error(bare)
        assert L.pt_debug_read_tree(bare, 5, buf.ctypes.data, buf.nbytes, None) != 0 and b"no scene" in L.pt_last_error(bare)
    finally:
        L.pt_destroy(bare)
    v, idx, ids, mats = _scene("box")
    c = ctxs(v, idx, ids, mats)
    image = c.render()
    bytes0, held0 = c.info().device_bytes, _held(c)
    assert held0 == {3, 5, 6}
    for what, out, cap, info, text in ((1, buf.ctypes.data, buf.nbytes, None, b"not held"), (2, buf.ctypes.data, buf.nbytes, None, b"not held"),
                                       (4, buf.ctypes.data, buf.nbytes, None, b"not held"),
                                       (3, buf.ctypes.data, _info(c).n_nodes * 32 - 1, None, b"capacity"), (5, buf.ctypes.data, 0, None, b"capacity"),
                                       (7, buf.ctypes.data, buf.nbytes, None, b"what"), (-1, buf.ctypes.data, buf.nbytes, None, b"what"),
                                       (3, None, buf.nbytes, None, b"null"), (0, None, 0, None, b"null")):
        buf[:] = 0xCDCDCDCD
        assert L.pt_debug_read_tree(c.ctx, what, out, cap, info) != 0, what
        assert text in c.err(), (what, c.err())
        assert (buf == 0xCDCDCDCD).all()
    n_bytes = _info(c).n_nodes * 32
    buf[:] = 0xCDCDCDCD
    assert L.pt_debug_read_tree(c.ctx, 3, buf.ctypes.data, n_bytes, C.byref(ti)) == 0          # the exact capacity, array and info in one call
    assert (buf[n_bytes // 4:] == 0xCDCDCDCD).all() and not (buf[:n_bytes // 4] == 0xCDCDCDCD).all() and ti.n_tris == len(idx)
    _read_held(c)
    assert c.info().device_bytes == bytes0 and _held(c) == held0
    for x, y in zip(c.render(), image):
        assert np.array_equal(x, y)
