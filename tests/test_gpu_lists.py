"""Complete lists in CSR form on the GPU: pt_list_offsets against the NumPy cumsum at the sizes its three kernels change path at;
pt_query_overlap_lists and pt_query_triangles_lists against tests/lists_ref.py (offsets, every index, found: words) on every scene,
box and triangle set and size; the ladder at every list length around the cuts, under every builder and on 20 000 coincident
triangles; offsets that do not fit (nothing outside the slices is written, the call says so, the context goes on); surplus slots; bad
queries; the refusals; the render state; scene edits; the wrappers, meshCollisions(pairs="all") and acgpt_main."""
import ctypes as C
import json
import os
import subprocess
import types

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import lists_ref as lr
import nearest_ref as nr
import overlap_ref as ov
import tritri_ref as tt
import query_scenes as qs
import test_gpu_overlap as go
from test_gpu_overlap import scenes            # noqa: F401  (the three scenes: box, diffuse, fp32 nodes)

pytestmark = pytest.mark.gpu

BOX = go.BOX
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
GUARD = 64                                      # bytes of 0xCD kept behind every output
REG, LDS, TILE, RUNS = _native.LIST_REGISTER, _native.LIST_SORT_LDS, _native.LIST_SCAN_TILE, _native.LIST_SCAN_RUNS      # the cuts (csrc/lists.h)
# two tile sums per lane of the second-level workgroup, and one more tile: its lanes' runs are three tiles long
SCAN_NS = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 2 * TILE * RUNS + 1)
LADDER_LENGTHS = tuple(sorted({0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 20000,
                               REG - 1, REG, REG + 1, LDS - 1, LDS, LDS + 1}))
MISMATCH = "do not fit this scene and these queries"
KINDS = {"box": ("pt_query_overlap", "pt_query_overlap_lists", 32), "tri": ("pt_query_triangles", "pt_query_triangles_lists", 48)}


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


class _Dev:
    """Device buffers of one test, each with GUARD bytes of 0xCD behind it; freed together"""
    def __init__(self, state):
        self.state, self.ptrs = state, []

    def alloc(self, nbytes, fill=0xCD):
        p = pt.pathtracer._device_buffers(self.state, 1, nbytes + GUARD)[0]
        self.ptrs.append(p)
        assert nbytes == 0 or _L().pt_device_memset(self.state.context, p, fill, nbytes) == 0
        assert _L().pt_device_memset(self.state.context, p + nbytes, 0xCD, GUARD) == 0
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            assert _L().pt_copy_to_device(self.state.context, p, a.ctypes.data, a.nbytes) == 0
        return p

    def down(self, p, nbytes, what, dtype=np.uint32):
        raw = np.zeros(nbytes + GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, p, raw.nbytes) == 0
        assert (raw[nbytes:] == 0xCD).all(), "%s: written past its end" % what
        return raw[:nbytes].view(dtype)

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.ptrs)
        self.ptrs = []


def _scan(state, counts):
    """(rc, offsets uint32 [n + 1], total) of pt_list_offsets on device copies, the guard behind offsets[n] checked"""
    d = _Dev(state)
    try:
        n = len(counts)
        d_c, d_o = d.up(np.asarray(counts, np.uint32)), d.alloc((n + 1) * 4)
        total = C.c_uint64(0xDEAD)
        rc = _L().pt_list_offsets(state.context, d_c if n else None, n, d_o, C.byref(total))
        return rc, d.down(d_o, (n + 1) * 4, "offsets").copy(), int(total.value)
    finally:
        d.free()


def _fill(state, kind, recs, offsets, capacity=None, pattern=0xCD, found=True):
    """(rc, prims uint32 [capacity] over a buffer pre-filled with `pattern`, found uint32 [n] or None) of the fill call with these
    offsets; the guards behind prims[capacity] and found[n] checked"""
    fn = getattr(_L(), KINDS[kind][1])
    n = recs.shape[0]
    offsets = np.asarray(offsets, np.uint32)
    assert offsets.shape == (n + 1,)
    capacity = int(offsets[-1]) if capacity is None else capacity
    d = _Dev(state)
    try:
        d_r, d_o, d_p, d_f = d.up(recs), d.up(offsets), d.alloc(capacity * 4, pattern), d.alloc(n * 4)
        rc = fn(state.context, d_r, n, d_o, d_p, capacity, d_f if found else None)
        return rc, d.down(d_p, capacity * 4, "prims").copy(), (d.down(d_f, n * 4, "found").copy() if found else None)
    finally:
        d.free()


def _csr(state, kind, recs):
    """The caller's sequence through the C ABI: (offsets uint32 [n + 1], prims, found, counts)"""
    count_fn = getattr(_L(), KINDS[kind][0])
    n = recs.shape[0]
    d = _Dev(state)
    try:
        d_r, d_c = d.up(recs), d.alloc(n * 4)
        assert count_fn(state.context, d_r, n, 0, None, d_c) == 0, _err(state)
        counts = d.down(d_c, n * 4, "counts").copy()
    finally:
        d.free()
    rc, offsets, total = _scan(state, counts)
    assert rc == 0 and total == int(offsets[-1]), _err(state)
    rc, prims, found = _fill(state, kind, recs, offsets)
    assert rc == 0, _err(state)
    return offsets, prims, found, counts


def _same(got, want, what):
    offsets, prims, found, counts = got
    w_off, w_prims, w_counts = want
    assert np.array_equal(counts, w_counts), what + ("counts",)
    assert np.array_equal(offsets.astype(np.uint64), w_off), what + ("offsets",)
    assert np.array_equal(found, w_counts), what + ("found", np.flatnonzero(found != w_counts)[:4])
    bad = np.flatnonzero(prims != w_prims)
    assert bad.size == 0, what + ("prims", bad[:4], prims[bad][:4], w_prims[bad][:4])


def _prefix(want, n):
    off, prims, counts = want
    return off[:n + 1], prims[:int(off[n])], counts[:n]


# ---- the scan alone ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bare():
    """A context without a scene: the scan needs none"""
    ctx = C.c_void_p()
    assert _L().pt_create(C.byref(ctx), 0) == 0
    yield types.SimpleNamespace(context=ctx)
    _L().pt_destroy(ctx)


@pytest.mark.parametrize("n", SCAN_NS)
def test_scan_equals_the_cumsum(bare, n):
    rng = np.random.default_rng(1000 + n % 997)
    counts = np.where(rng.random(n) < 0.6, 0, rng.integers(0, 3000, n)).astype(np.uint32)          # many zeros, lists of every class
    want = lr.offsets_of(counts)
    assert want[-1] <= 0xFFFFFFFF
    rc, offsets, total = _scan(bare, counts)
    assert rc == 0, _err(bare)
    assert total == int(want[-1]) and np.array_equal(offsets.astype(np.uint64), want), (n, np.flatnonzero(offsets != want)[:4])
    rc2, again, total2 = _scan(bare, counts)
    assert rc2 == 0 and total2 == total and np.array_equal(again, offsets)                          # two calls give the same bits
    if n > TILE * RUNS:
        assert (n + TILE - 1) // TILE > 2 * RUNS                                                    # runs of three tile sums per lane


def test_scan_without_a_total_and_without_counts(bare):
    d = _Dev(bare)
    try:
        d_c, d_o = d.up(np.array([5, 0, 7], np.uint32)), d.alloc(16)
        assert _L().pt_list_offsets(bare.context, d_c, 3, d_o, None) == 0, _err(bare)
        assert d.down(d_o, 16, "offsets").tolist() == [0, 5, 5, 12]
        total = C.c_uint64(77)
        assert _L().pt_list_offsets(bare.context, None, 0, None, C.byref(total)) == 0 and total.value == 0        # nothing to write
    finally:
        d.free()


@pytest.mark.parametrize("n", [3, 2 * TILE + 1, TILE * RUNS + 5])
def test_scan_total_at_and_above_32_bits(bare, n):
    """0xFFFFFFFF is the last total 32-bit offsets describe; 0x100000000 is refused after it has been computed, with *total set"""
    counts = np.zeros(n, np.uint32)
    counts[0], counts[n // 2], counts[n - 1] = 0x80000000, 0x7FFFFFF0, 0xF
    rc, offsets, total = _scan(bare, counts)
    assert rc == 0 and total == 0xFFFFFFFF and np.array_equal(offsets.astype(np.uint64), lr.offsets_of(counts)), _err(bare)
    counts[n // 2] += 1
    rc, _, total = _scan(bare, counts)
    assert rc != 0 and total == 0x100000000 and "4294967296" in _err(bare) and "split the batch" in _err(bare)
    counts[:] = 0xFFFFFFFF                                                                          # far above: the sums are 64-bit
    rc, _, total = _scan(bare, counts)
    assert rc != 0 and total == n * 0xFFFFFFFF
    rc, offsets, total = _scan(bare, [1, 2, 3])                                                     # the context goes on
    assert rc == 0 and total == 6 and offsets.tolist() == [0, 1, 3, 6]


def test_scan_refusals(bare):
    L, ctx = _L(), bare.context
    d = _Dev(bare)
    try:
        c, o = d.up(np.arange(256, dtype=np.uint32)), d.alloc(257 * 4)
        t = C.c_uint64(0)
        cases = {"null counts": L.pt_list_offsets(ctx, None, 256, o, C.byref(t)), "null offsets": L.pt_list_offsets(ctx, c, 256, None, C.byref(t)),
                 "too many": L.pt_list_offsets(ctx, c, 0x80000000, o, C.byref(t)), "counts not aligned": L.pt_list_offsets(ctx, c + 2, 16, o, C.byref(t)),
                 "offsets not aligned": L.pt_list_offsets(ctx, c, 16, o + 1, C.byref(t)), "in place": L.pt_list_offsets(ctx, c, 256, c, C.byref(t)),
                 "offsets begin in the last count": L.pt_list_offsets(ctx, c, 256, c + 255 * 4, C.byref(t)),
                 "counts lie inside offsets": L.pt_list_offsets(ctx, o + 64, 16, o, C.byref(t)), "null context": L.pt_list_offsets(None, c, 256, o, C.byref(t))}
        assert all(rc != 0 for rc in cases.values()), cases
        # the order: a null argument before the size, the size before the alignment, the alignment before the overlap
        assert L.pt_list_offsets(ctx, None, 0x80000000, o, None) != 0 and "null argument" in _err(bare)
        assert L.pt_list_offsets(ctx, c + 2, 0x80000000, o, None) != 0 and "too many counts" in _err(bare)
        assert L.pt_list_offsets(ctx, c + 2, 256, c, None) != 0 and "4-byte aligned" in _err(bare)
        assert L.pt_list_offsets(ctx, c, 256, c + 4, None) != 0 and "overlaps counts" in _err(bare) and _err(bare).startswith("pt_list_offsets: ")
        assert (d.down(o, 257 * 4, "offsets", np.uint8) == 0xCD).all()                              # no refusal wrote anything
        assert L.pt_list_offsets(ctx, c, 256, o, C.byref(t)) == 0 and t.value == 255 * 128
    finally:
        d.free()


# ---- the lists against the brute force ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def references(scenes):          # noqa: F811
    """(kind, scene, set) -> (records, (offsets, prims, counts)) by the brute force on the whole set: computed once, shared, never
    written.  The fp32-node scene is the box: it shares the box's."""
    cache = {}

    def get(kind, scene, name):
        key = (kind, "box" if scene == "fp32" else scene, name)
        if key not in cache:
            state, obj = scenes(key[1])
            verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
            first = lambda rays: go._host_closest(state, rays)                                      # noqa: E731
            if kind == "box":
                recs = ov.box_set(name, verts, idx, go._camera(state), first_hits=first)
                want = lr.csr_of_matrix(ov.overlap_matrix(recs, verts, idx))
            else:
                recs = tt.query_set(name, verts, idx, go._camera(state), first_hits=first)
                want = lr.csr_of_matrix(tt.intersect_matrix(recs, verts, idx))
            for a in (recs,) + want:
                a.setflags(write=False)
            cache[key] = (recs, want)
        return cache[key]

    return get


@pytest.mark.parametrize("kind,name", [("box", s) for s in ov.BOX_SETS] + [("tri", s) for s in tt.QUERY_SETS])
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_lists_equal_the_brute_force(scenes, references, scene, kind, name):          # noqa: F811
    state, obj = scenes(scene)
    recs, want = references(kind, scene, name)
    before = pt.getBvhInfo(state).device_bytes
    for n in SIZES:
        _same(_csr(state, kind, recs[:n]), _prefix(want, n), (scene, kind, name, n))
    assert pt.getBvhInfo(state).device_bytes == before


def test_two_calls_give_the_same_bits(scenes, references):          # noqa: F811
    state, _ = scenes("diffuse")
    for kind, name in (("box", "wall_faces"), ("tri", "whole")):
        recs, want = references(kind, "diffuse", name)
        a, b = _csr(state, kind, recs), _csr(state, kind, recs)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        _same(a, want, (kind, name))


def test_the_timing_hook_changes_no_list(scenes, references):          # noqa: F811
    """pt_debug_list_phases (tools/lists_timing.py): the fill without the register list gives the product's lists at every length
    class; the fill alone leaves the long slices as sets, in walk order; the sort alone finishes them; the refusals"""
    state, obj = scenes("box")
    L, ctx = _L(), state.context
    try:
        for kind, name in (("box", "wall_faces"), ("tri", "whole")):
            recs, want = references(kind, "box", name)
            assert L.pt_debug_list_phases(ctx, 7) == 0
            _same(_csr(state, kind, recs), want, (kind, name, "no register list"))
            assert L.pt_debug_list_phases(ctx, 1) == 0
            offsets, prims, found, counts = _csr(state, kind, recs)
            assert np.array_equal(found, want[2])
            for i in range(recs.shape[0]):
                lo, hi = int(offsets[i]), int(offsets[i + 1])
                assert np.array_equal(np.sort(prims[lo:hi]), want[1][lo:hi]) and (hi - lo > REG or np.array_equal(prims[lo:hi], want[1][lo:hi])), (kind, i)
        for bad in (0, 4, 8, 11):
            assert L.pt_debug_list_phases(ctx, bad) != 0 and "pt_debug_list_phases" in _err(state)
        assert L.pt_debug_list_phases(None, 3) != 0
    finally:
        assert L.pt_debug_list_phases(ctx, 3) == 0
    recs, want = references("box", "box", "wall_faces")
    _same(_csr(state, "box", recs), want, ("box", "the product again"))


# ---- the ladder ----------------------------------------------------------------------------------------------------------------------

def _interleaved():
    """The lengths so that short and long lists share a wave: the sorted lengths dealt from both ends, four times over (more than a
    wave, less than a workgroup), each copy in another order"""
    k = list(LADDER_LENGTHS)
    pairs = [x for a, b in zip(k, reversed(k)) for x in (a, b)][:len(k)]
    return np.array(pairs + pairs[5:] + pairs[:5] + pairs[11:] + pairs[:11] + pairs[::-1], np.int64)


@pytest.fixture(scope="module")
def ladder_ctxs():
    """build mode -> a context that holds the ladder; None: the copies scene of tests/query_scenes.py"""
    made = {}

    def get(mode):
        if mode not in made:
            if mode is None:
                v, idx, ids, mats = qs.copies()
            else:
                (v, idx), mats = lr.ladder(), qs.box()[3]
                ids = np.zeros(len(idx), np.uint32)
            made[mode] = qs._Ctx.from_arrays(v, idx, ids, mats, build_mode=mode)
        return made[mode]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def ladder_want():
    lengths = _interleaved()
    want = lr.ladder_expected(lengths)
    v, idx = lr.ladder()
    out = {}
    for kind, recs, m in (("box", lr.ladder_boxes(lengths), None), ("tri", lr.ladder_triangles(lengths), None)):
        # the brute force decides the lengths (on the distinct queries; the copies are copies), and they are the ones asked for
        first = recs[:len(LADDER_LENGTHS)]
        m = ov.overlap_matrix(first, v, idx.reshape(-1)) if kind == "box" else tt.intersect_matrix(first, v, idx.reshape(-1))
        assert np.array_equal(m.sum(axis=1), lengths[:len(LADDER_LENGTHS)])
        out[kind] = recs
    assert sorted(set(lengths.tolist())) == list(LADDER_LENGTHS) and 64 < lengths.size < 256
    assert {REG - 1, REG, REG + 1, LDS - 1, LDS, LDS + 1, 20000} <= set(LADDER_LENGTHS)
    return out, want


@pytest.mark.parametrize("kind", ["box", "tri"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ladder_under_every_builder(ladder_ctxs, ladder_want, mode, kind):
    """Every list length around every cut in one call, short and long lists in one wave; ascending whatever tree the builder made"""
    c = ladder_ctxs(mode)
    recs, want = ladder_want
    _same(_csr(qs.state_of(c), kind, recs[kind]), want, ("ladder", mode, kind))


@pytest.mark.parametrize("kind", ["box", "tri"])
def test_all_of_twenty_thousand_coincident_triangles(ladder_ctxs, kind):
    """The copies scene: the deepest tree the suite has, and one query whose list is 0 .. 19 999 beside queries that find nothing"""
    c = ladder_ctxs(None)
    assert c.info().n_tris == 20000
    tri = np.array([[100, 100, 300], [400, 100, 300], [100, 400, 300]], np.float32)
    if kind == "box":
        recs = ov.as_boxes([[250, 250, 300], [250, 250, 900], [200, 200, 300]], [[200, 200, 1], [10, 10, 10], [0, 0, 0]])
    else:
        recs = tt.as_records(np.stack([tri, tri + np.float32(500.0), tri[::-1]]))
    v, idx = qs.copies()[:2]
    want = lr.csr_of_matrix((ov.overlap_matrix if kind == "box" else tt.intersect_matrix)(recs, v, idx.reshape(-1)))
    assert want[2].tolist() == [20000, 0, 20000]                          # the brute force decides
    offsets, prims, found, counts = _csr(qs.state_of(c), kind, recs)
    assert counts.tolist() == [20000, 0, 20000] and found.tolist() == [20000, 0, 20000] and offsets.tolist() == [0, 20000, 20000, 40000]
    assert np.array_equal(prims, np.tile(np.arange(20000, dtype=np.uint32), 2))


# ---- offsets that do not fit ----------------------------------------------------------------------------------------------------------

def _slices_only(prims, offsets, capacity, pattern):
    """No word outside the valid slices changed: everything not inside a slice lo <= hi <= capacity still holds the pattern"""
    inside = np.zeros(capacity, bool)
    for lo, hi in zip(offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)):
        if lo <= hi <= capacity:
            inside[lo:hi] = True
    word = np.uint32(pattern * 0x01010101)
    assert (prims[~inside] == word).all(), np.flatnonzero((prims != word) & ~inside)[:8]


@pytest.mark.parametrize("kind", ["box", "tri"])
def test_offsets_that_do_not_fit_write_nothing_outside_the_slices(scenes, references, kind):          # noqa: F811
    state, obj = scenes("box")
    recs, want = references(kind, "box", "wall_faces" if kind == "box" else "whole")
    other, other_want = references(kind, "box", "random")
    n = 600
    recs, w_off, w_counts = recs[:n], want[0][:n + 1].astype(np.uint32), want[2][:n]
    good = _prefix(want, n)
    cap = int(w_off[-1])
    stale = other_want[0][:n + 1].astype(np.uint32)                       # offsets of a different query set
    assert (np.diff(stale.astype(np.int64)) < w_counts).any()
    short = cap // 2                                                      # a capacity below offsets[n]
    down = w_off[::-1].copy()                                             # decreasing offsets: no slice satisfies lo <= hi but the empty ones
    shifted = (w_off.astype(np.int64) + 5).astype(np.uint32)              # every slice moved: the last ones reach past the capacity
    for what, offsets, capacity in (("another set's", stale, int(stale[-1])), ("capacity too small", w_off, short), ("decreasing", down, cap),
                                    ("shifted", shifted, cap)):
        for pattern in (0xCD, 0x5A):
            rc, prims, found = _fill(state, kind, recs, offsets, capacity, pattern)
            assert rc != 0 and MISMATCH in _err(state) and _err(state).startswith(KINDS[kind][1] + ": "), (what, _err(state))
            assert np.array_equal(found, w_counts), what                  # found is right whatever the offsets say
            _slices_only(prims, offsets, capacity, pattern)
        # the slices that do fit and are long enough hold their lists
        for i in range(n):
            lo, hi = int(offsets[i]), int(offsets[i + 1])
            if lo <= hi <= capacity and hi - lo >= w_counts[i]:
                k = int(w_counts[i])
                assert np.array_equal(prims[lo:lo + k], good[1][int(w_off[i]):int(w_off[i]) + k]) and (prims[lo + k:hi] == 0xFFFFFFFF).all(), (what, i)
        _same(_csr(state, kind, recs), good, (kind, "after", what))       # the next correct call equals the reference


@pytest.mark.parametrize("kind", ["box", "tri"])
def test_offsets_from_before_a_vertex_update(gpu_state_factory, kind):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    recs = (ov.box_set("wall_faces", verts0, idx) if kind == "box" else tt.query_set("self", verts0, idx))[:500]
    # the blocks (everything strictly inside the room) move: the counts change, the offsets of before are stale
    verts = np.array(verts0, np.float32).reshape(-1, 4).copy()
    lo, hi = nr.scene_box(verts, idx)
    inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)
    verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
    brute = ov.overlap_matrix if kind == "box" else tt.intersect_matrix
    here, there = lr.csr_of_matrix(brute(recs, verts0, idx)), lr.csr_of_matrix(brute(recs, verts, idx))
    assert (here[2] != there[2]).any()
    # the direction in which some list grows, so that its old slice is too short: from the scene as loaded, or from the moved one
    before, after, want = (verts0, verts, there) if (there[2] > here[2]).any() else (verts, verts0, here)
    if before is verts:
        assert not pt.updateVertices(state, before, "refit")["rebuilt"]
    old = _csr(state, kind, recs)
    assert not pt.updateVertices(state, after, "refit")["rebuilt"]
    assert (want[2] > old[3]).any()
    rc, prims, found = _fill(state, kind, recs, old[0], pattern=0x5A)
    assert rc != 0 and MISMATCH in _err(state) and np.array_equal(found, want[2])
    _slices_only(prims, old[0], int(old[0][-1]), 0x5A)
    _same(_csr(state, kind, recs), want, (kind, "after the update"))


@pytest.mark.parametrize("kind", ["box", "tri"])
def test_surplus_slots(scenes, references, kind):          # noqa: F811
    """Offsets from counts plus a margin: no flag iff every slice is long enough, 0xFFFFFFFF behind the indices"""
    state, obj = scenes("diffuse")
    recs, want = references(kind, "diffuse", "wall_faces" if kind == "box" else "wall_touch")
    n = 700
    recs, (w_off, w_prims, w_counts) = recs[:n], _prefix(want, n)
    margin = np.arange(n, dtype=np.uint32) % 11                            # 0 .. 10 spare words: slices move across the register cut
    roomy = lr.offsets_of(w_counts + margin).astype(np.uint32)
    rc, prims, found = _fill(state, kind, recs, roomy, pattern=0x5A)
    assert rc == 0, _err(state)
    assert np.array_equal(found, w_counts)
    for i in range(n):
        lo, k, hi = int(roomy[i]), int(w_counts[i]), int(roomy[i + 1])
        assert np.array_equal(prims[lo:lo + k], w_prims[int(w_off[i]):int(w_off[i + 1])]) and (prims[lo + k:hi] == 0xFFFFFFFF).all(), i
    # one slice one word short, among roomy ones: the flag, and still nothing outside the slices
    victim = int(np.flatnonzero(w_counts > REG + 2)[3])
    lens = (w_counts + margin).astype(np.int64)
    lens[victim] = int(w_counts[victim]) - 1
    tight = lr.offsets_of(lens).astype(np.uint32)
    rc, prims, found = _fill(state, kind, recs, tight, pattern=0x5A)
    assert rc != 0 and MISMATCH in _err(state) and np.array_equal(found, w_counts)
    for i in range(n):
        if i != victim:
            lo, k, hi = int(tight[i]), int(w_counts[i]), int(tight[i + 1])
            assert np.array_equal(prims[lo:lo + k], w_prims[int(w_off[i]):int(w_off[i + 1])]) and (prims[lo + k:hi] == 0xFFFFFFFF).all(), i
    # a short slice at or below the register cut too
    small = int(np.flatnonzero((w_counts >= 2) & (w_counts <= REG))[0])
    lens = w_counts.astype(np.int64)
    lens[small] -= 1
    rc, _, found = _fill(state, kind, recs, lr.offsets_of(lens).astype(np.uint32))
    assert rc != 0 and MISMATCH in _err(state) and np.array_equal(found, w_counts)


@pytest.mark.parametrize("kind", ["box", "tri"])
def test_bad_queries_between_good_ones(scenes, references, kind):          # noqa: F811
    state, obj = scenes("box")
    recs, want = references(kind, "box", "centroids" if kind == "box" else "self")
    recs = recs[:200].copy()
    bad, _ = ov.bad_boxes(recs[3]) if kind == "box" else tt.bad_triangles(recs[3])
    where = 5 + 3 * np.arange(len(bad))                                   # inside the first wave and beyond, good ones between
    assert where[-1] < 200 and where[1] < 64
    recs[where] = bad
    counts = want[2][:200].copy()
    counts[where] = 0
    keep = np.ones(200, bool)
    keep[where] = False
    prims = np.concatenate([want[1][int(want[0][i]):int(want[0][i + 1])] for i in np.flatnonzero(keep)])
    _same(_csr(state, kind, recs), (lr.offsets_of(counts), prims, counts), (kind, "bad between good"))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["box", "tri"])
def test_refusals_leave_the_context_usable(scenes, references, kind):          # noqa: F811
    state, obj = scenes("box")
    recs, want = references(kind, "box", "random")
    fn, ctx, rb = getattr(_L(), KINDS[kind][1]), state.context, KINDS[kind][2]
    n = 256
    off = want[0][:n + 1].astype(np.uint32)
    cap = int(off[-1])
    what = "boxes" if kind == "box" else "triangles"
    d = _Dev(state)
    try:
        r, o, p, f = d.up(recs[:n]), d.up(off), d.alloc(max(cap, 4096) * 4), d.alloc(n * 4)
        cases = {"null records": fn(ctx, None, n, o, p, cap, f), "null offsets": fn(ctx, r, n, None, p, cap, f), "null prims": fn(ctx, r, n, o, None, cap, f),
                 "too many": fn(ctx, r, 0x80000000, o, p, cap, f), "records not aligned": fn(ctx, r + 4, 16, o, p, cap, f),
                 "offsets not aligned": fn(ctx, r, 16, o + 2, p, cap, f), "prims not aligned": fn(ctx, r, 16, o, p + 1, cap, f),
                 "found not aligned": fn(ctx, r, 16, o, p, cap, f + 2), "prims are the records": fn(ctx, r, n, o, r, 64, f),
                 "offsets lie inside the records": fn(ctx, r, n, r + 16, p, cap, f), "found begins in the last record": fn(ctx, r, n, o, p, cap, r + n * rb - 16),
                 "offsets lie inside prims": fn(ctx, r, n, p + 64, p, 4096, f), "found lies inside prims": fn(ctx, r, n, o, p, 4096, p + 128),
                 "found is the offsets": fn(ctx, r, n, o, p, cap, o), "found begins in offsets[n]": fn(ctx, r, n, o, p, cap, o + n * 4),
                 "null context": fn(None, r, n, o, p, cap, f)}
        assert all(rc != 0 for rc in cases.values()), cases
        # the order: a null argument before the size, the size before the alignment, the alignment before the overlap
        assert fn(ctx, None, 0x80000000, o, p, cap, f) != 0 and "null argument" in _err(state)
        assert fn(ctx, r + 4, 0x80000000, o, p, cap, f) != 0 and "too many " + what in _err(state)
        assert fn(ctx, r + 4, n, o, r, cap, f) != 0 and "16-byte aligned" in _err(state)
        assert fn(ctx, r, n, o + 2, r, cap, f) != 0 and "4-byte aligned" in _err(state)
        assert fn(ctx, r, n, o, r, 64, f) != 0 and "prims overlaps the " + what in _err(state) and _err(state).startswith(KINDS[kind][1] + ": ")
        for buf, nbytes in ((p, max(cap, 4096) * 4), (f, n * 4)):
            assert (d.down(buf, nbytes, "an output", np.uint8) == 0xCD).all()        # no refusal wrote anything
        assert fn(ctx, r, 0, o, p, cap, f) == 0 and fn(ctx, None, 0, None, None, 0, None) == 0                     # n == 0: a no-op
        # capacity == 0 allows a null prims: lists that are all empty need no array (and any other offsets raise the flag, unwritten)
        z = d.up(np.zeros(n + 1, np.uint32))
        far = ov.as_boxes(np.full((n, 3), 1e6), 1.0) if kind == "box" else tt.as_records(np.full((n, 3, 3), 1e6) + np.eye(3))
        rf = d.up(far)
        assert fn(ctx, rf, n, z, None, 0, f) == 0, _err(state)
        assert not d.down(f, n * 4, "found").any()
        assert fn(ctx, r, n, o, None, 0, f) != 0 and MISMATCH in _err(state)
        assert np.array_equal(d.down(f, n * 4, "found"), want[2][:n])
        # a context without a scene
        bare = C.c_void_p()
        assert _L().pt_create(C.byref(bare), 0) == 0
        try:
            assert fn(bare, r, n, o, p, cap, f) != 0 and b"no scene" in _L().pt_last_error(bare)
        finally:
            _L().pt_destroy(bare)
    finally:
        d.free()
    _same(_csr(state, kind, recs[:n]), _prefix(want, n), (kind, "after the refusals"))


# ---- other state ----------------------------------------------------------------------------------------------------------------------

def test_list_queries_leave_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    boxes, tris = ov.box_set("wall_faces", verts, idx)[:300], tt.query_set("self", verts, idx)[:300]
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        a = pt.queryOverlapLists(state, boxes)
        b = pt.queryTrianglesLists(state, tris)
        assert a["prim"].size > 2400 and b["prim"].size > 2400
        assert pt.getBvhInfo(state).device_bytes == before               # the scratch is the context's, not the scene's
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_after_updates_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    boxes = np.concatenate([ov.box_set(name, verts0, idx)[:300] for name in ("random", "wall_faces", "centroids")])
    tris = np.concatenate([tt.query_set(name, verts0, idx)[:300] for name in ("self", "whole", "wall_touch")])
    sets = (("box", boxes, ov.overlap_matrix), ("tri", tris, tt.intersect_matrix))
    old = {kind: lr.csr_of_matrix(fn(recs, verts0, idx)) for kind, recs, fn in sets}
    for kind, recs, _ in sets:
        _same(_csr(state, kind, recs), old[kind], (kind, "before"))
    pt.updateMaterials(state, material_ids=(np.asarray(obj.getMaterialIndices(), np.uint32)[::-1]).copy())
    for kind, recs, _ in sets:
        _same(_csr(state, kind, recs), old[kind], (kind, "materials"))
    verts = np.array(verts0, np.float32).reshape(-1, 4).copy()
    lo, hi = nr.scene_box(verts, idx)
    inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)
    verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
    moved = pt.TinyObjWrapper(BOX)
    moved._vertices = verts.reshape(-1).copy()
    fresh = go._fresh_state(state, moved)
    try:
        want = {kind: lr.csr_of_matrix(fn(recs, verts, idx)) for kind, recs, fn in sets}
        assert all((want[k][2] != old[k][2]).any() for k in want)        # the move shows in the answers
        for mode, rebuilt in (("refit", False), ("rebuild", True)):
            assert bool(pt.updateVertices(state, verts if mode == "refit" else verts0, mode)["rebuilt"]) == rebuilt
            if mode == "rebuild":                                         # back, rebuilt, and to the moved vertices again by a rebuild
                assert pt.updateVertices(state, verts, mode)["rebuilt"]
            for kind, recs, _ in sets:
                _same(_csr(state, kind, recs), want[kind], (kind, mode))
                _same(_csr(fresh, kind, recs), want[kind], (kind, "fresh"))
    finally:
        pt.CleanAllTheThings(fresh)


# ---- the layers above -----------------------------------------------------------------------------------------------------------------

def test_wrappers_numpy_path(scenes, references):          # noqa: F811
    state, obj = scenes("diffuse")
    for kind, name, fn in (("box", "wall_faces", pt.queryOverlapLists), ("tri", "self", pt.queryTrianglesLists)):
        recs, want = references(kind, "diffuse", name)
        got = fn(state, recs)
        assert sorted(got) == ["count", "offsets", "prim"] and all(a.dtype == np.uint32 for a in got.values())
        assert np.array_equal(got["offsets"].astype(np.uint64), want[0]) and np.array_equal(got["prim"], want[1]) and np.array_equal(got["count"], want[2])
    boxes, want = references("box", "diffuse", "centroids")
    got = pt.queryOverlapLists(state, boxes[:100, 0:3].astype(np.float64), boxes[:100, 3:6])      # centres and half extents
    assert np.array_equal(got["prim"], _prefix(want, 100)[1])
    tris, want = references("tri", "diffuse", "edge")
    got = pt.queryTrianglesLists(state, tt.vertices_of(tris[:100]))                                # (n, 3, 3) vertices
    assert np.array_equal(got["prim"], _prefix(want, 100)[1]) and np.array_equal(got["offsets"].astype(np.uint64), want[0][:101])
    far = pt.queryOverlapLists(state, np.full((5, 3), 1e6), 1.0)                                   # nothing found: an empty prim
    assert far["prim"].shape == (0,) and not far["count"].any() and not far["offsets"].any()


def test_wrappers_torch_path(scenes, references, monkeypatch):          # noqa: F811
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    L = _L()
    dev = torch.device("cuda", 0)
    for kind, name, fn, sym in (("box", "wall_faces", pt.queryOverlapLists, "pt_query_overlap_lists"), ("tri", "self", pt.queryTrianglesLists, "pt_query_triangles_lists")):
        recs, want = references(kind, "box", name)
        seen = {}
        real = getattr(L, sym)
        monkeypatch.setattr(L, sym, lambda ctx, r, n, o, p, cap, f, real=real, seen=seen: seen.update(call=(r, n, p, cap)) or real(ctx, r, n, o, p, cap, f))
        x = (torch.from_numpy(recs.copy()).to(dev) * 1.0).contiguous()        # a result of torch's own kernels
        got = fn(state, x)
        assert seen["call"] == (x.data_ptr(), recs.shape[0], got["prim"].data_ptr(), int(want[0][-1]))      # no copy in, torch's allocation out
        assert all(v.device == dev for v in got.values())
        assert got["prim"].dtype == torch.int32 and got["count"].dtype == torch.int32 and got["offsets"].dtype == torch.int64
        assert np.array_equal(got["offsets"].cpu().numpy().astype(np.uint64), want[0])
        assert np.array_equal(got["prim"].cpu().numpy().view(np.uint32), want[1]) and np.array_equal(got["count"].cpu().numpy().view(np.uint32), want[2])
        for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :5].contiguous(), "expected an")):
            with pytest.raises(pt.PathTracerError, match=what):
                fn(state, bad)
        empty = fn(state, x[:0])
        assert empty["prim"].shape == (0,) and empty["offsets"].tolist() == [0] and empty["count"].shape == (0,)


def test_mesh_collisions_all_pairs(scenes, references):          # noqa: F811
    """The mesh against itself, what a collision pass sees at contact: every triple, where pairs=True cuts 97 % of the lists"""
    state, obj = scenes("box")
    verts = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    idx = np.asarray(obj.getIndexBuffer(), np.uint32).reshape(-1, 3)
    T = 400
    poses = np.stack([np.eye(4, dtype=np.float32)[:3], np.array([[1, 0, 0, 3], [0, 1, 0, 0], [0, 0, 1, -2]], np.float32)])
    recs = np.concatenate([pt.triangleRecords(verts, idx[:T], p) for p in poses])
    m = tt.intersect_matrix(recs, obj.getVerticesFloat(), obj.getIndexBuffer())
    rows, cols = np.nonzero(m)
    got = pt.meshCollisions(state, verts, idx[:T], poses, pairs="all")
    assert got["pairs"].dtype == np.int64 and np.array_equal(got["pairs"], np.stack([rows // T, rows % T, cols], axis=1))
    capped = pt.meshCollisions(state, verts, idx[:T], poses, pairs=True)
    assert np.array_equal(got["counts"], capped["counts"]) and np.array_equal(got["counts"], m.sum(axis=1).reshape(2, T))
    assert (m.sum(axis=1) > 8).sum() >= 100 and len(capped["pairs"]) < len(got["pairs"])             # by the brute force: lists that pairs=True cuts
    have = set(map(tuple, got["pairs"].tolist()))
    assert all(tuple(t) in have for t in capped["pairs"].tolist())
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        tv, ti, tp = torch.from_numpy(verts).to(dev), torch.from_numpy(idx[:T].astype(np.int64)).to(dev), torch.from_numpy(poses[:1]).to(dev)
        tgot = pt.meshCollisions(state, tv, ti, tp, pairs="all")
        assert tgot["pairs"].device == dev and np.array_equal(tgot["pairs"].cpu().numpy(), got["pairs"][got["pairs"][:, 0] == 0])


def test_cli_all_prints_what_the_wrappers_say(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (np.float32(0.5) * (lo + hi)).astype(np.float32)
    boxes = ov.as_boxes([c, c, [hi[0] + 100, c[1], c[2]], [c[0], lo[1], c[2]]], [[300, 300, 300], [300, 300, 300], [10, 10, 10], [40, 0, 40]])
    tris = np.array([[[c[0] - 300, c[1], c[2] - 300], [c[0] + 300, c[1] + 10, c[2]], [c[0], c[1] - 10, c[2] + 300]],
                     [[c[0] - 300, c[1], c[2] - 300], [c[0] + 300, c[1] + 10, c[2]], [c[0], c[1] - 10, c[2] + 300]],
                     [[hi[0] + 100, c[1], c[2]], [hi[0] + 120, c[1], c[2]], [hi[0] + 100, c[1] + 20, c[2]]]], np.float32)
    b_ks, t_ks = ["all", "8", "all", "all"], ["all", None, "all"]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for b, k in zip(boxes, b_ks):
        cmd += ["--overlap", ",".join("%r" % float(a) for a in b[:6]) + "," + k]
    for t, k in zip(tris, t_ks):
        cmd += ["--intersect", ",".join("%r" % float(a) for a in t.reshape(-1)) + ("" if k is None else "," + k)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    over = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"overlap"')]
    inter = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"intersect"')]
    assert len(over) == 4 and len(inter) == 3
    bl, tl = pt.queryOverlapLists(state, boxes), pt.queryTrianglesLists(state, tris)
    assert bl["count"][0] > 100 and bl["count"][2] == 0 and bl["count"][3] >= 1 and tl["count"][0] > 8 and tl["count"][2] == 0
    for lines, got, ks in ((over, bl, b_ks), (inter, tl, t_ks)):
        for i, line in enumerate(lines):
            full = [int(t) for t in got["prim"][int(got["offsets"][i]):int(got["offsets"][i + 1])]]
            assert line["count"] == int(got["count"][i]) == len(full)
            assert line["triangles"] == (full if ks[i] == "all" else full[:8])
    assert len(over[0]["materials"]) == len(over[0]["triangles"]) and over[1]["triangles"] == over[0]["triangles"][:8]
    # the numeric forms print what they printed: the same line whether or not an "all" stands beside them
    alone = subprocess.run(cmd[:13] + ["--overlap", cmd[cmd.index("--overlap") + 3], "--intersect", ",".join("%r" % float(a) for a in tris[1].reshape(-1))],
                           capture_output=True, text=True, timeout=300)
    assert alone.returncode == 0, alone.stdout + alone.stderr
    for key, idx_ in (('{"overlap"', 1), ('{"intersect"', 1)):
        mine = [l for l in run.stdout.splitlines() if l.startswith(key)][idx_]
        theirs = [l for l in alone.stdout.splitlines() if l.startswith(key)]
        assert theirs == [mine]
    for opt, arg in (("--overlap", "1,2,3,4,5,all"), ("--overlap", "1,2,3,4,5,6,8,all"), ("--intersect", "1,2,3,1,1,1,2,2,all"), ("--intersect", "1,2,3,1,1,1,2,2,2,3,all")):
        bad = subprocess.run([exe, "--obj", BOX, opt, arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and opt in bad.stderr, arg
