"""The K closest triangles and the within-radius byte on the GPU: pt_query_nearest_k and pt_query_within_any against
tests/nearest_k_ref.py's brute force (every record, count and byte, bits) on every scene, size, point set, radius and k, with counts,
without and counts alone; record 0 against pt_query_nearest on the device; the points that are a miss before any traversal, the
outputs' bounds, the scene's memory, scene edits, the render state, the refusals, the counting twin, torch tensors, sphereContacts
and acgpt_main --nearest-k / --within."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import nearest_ref as nr
import nearest_k_ref as kr

F = np.float32
pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
KS = (1, 2, 3, 4, 5, 8)                            # every list size the kernels have, and a max_k below its list's size (3, 5)
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
MISS = 0xFFFFFFFF
GUARD = 64                                         # bytes of 0xCD kept in front of and behind every output


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


def _camera(state):
    p = state.params
    return p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple()


def _host_closest(state, rays):
    rays = np.ascontiguousarray(rays, np.float32)
    n = rays.shape[0]
    t = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32)
    assert _L().pt_trace_closest(state.context, rays.ctypes.data, n, t.ctypes.data, prim.ctypes.data) == 0, _err(state)
    return t, prim


class Device:
    """points in a device buffer with room for every output of the largest call and a guard in front of and behind each; the C ABI
    called as a C caller would.  Calls take the first n points.  The hit bytes start at an odd address."""

    def __init__(self, state, points):
        self.state, self.n_max = state, points.shape[0]
        self.points = np.ascontiguousarray(points, np.float32)
        assert self.points.shape == (self.n_max, 4)
        m = max(self.n_max, 1)
        self.bufs = pt.pathtracer._device_buffers(state, 6, m * kr.MAX_K * 32 + 2 * GUARD + 16)
        self.p = self.bufs[0]
        self.out, self.counts, self.hit, self.visits, self.one = (b + GUARD for b in self.bufs[1:])
        self.hit += 1
        assert _L().pt_copy_to_device(state.context, self.p, self.points.ctypes.data, max(self.points.nbytes, 16)) == 0

    def _arm(self, ptr, nbytes):
        assert _L().pt_device_memset(self.state.context, ptr - GUARD, 0xCD, nbytes + 2 * GUARD) == 0

    def _read(self, ptr, nbytes, what):
        raw = np.zeros(nbytes + 2 * GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, ptr - GUARD, raw.nbytes) == 0
        assert (raw[:GUARD] == 0xCD).all(), "written in front of " + what
        assert (raw[GUARD + nbytes:] == 0xCD).all(), "written past the end of " + what
        return raw[GUARD:GUARD + nbytes].copy()

    def lists(self, k, counts, n=None, visits=False):
        """(records uint32 [n, k, 8] or None with k = 0, counts uint32 [n] or None[, visits uint32 [n, 2]])"""
        L, s = _L(), self.state
        n = self.n_max if n is None else n
        self._arm(self.out, n * k * 32)
        self._arm(self.counts, n * 4)
        out, cnt = (self.out if k else None), (self.counts if counts else None)
        if visits:
            self._arm(self.visits, n * 8)
            assert L.pt_debug_nearest_k_visits(s.context, self.p, n, k, out, cnt, None, self.visits) == 0, _err(s)
        else:
            assert L.pt_query_nearest_k(s.context, self.p, n, k, out, cnt) == 0, _err(s)
        rec = self._read(self.out, n * k * 32, "out").view(np.uint32).reshape(n, k, 8)
        c = self._read(self.counts, n * 4 if counts else 0, "counts").view(np.uint32)
        got = (rec if k else None, c if counts else None)
        return got + (self._read(self.visits, n * 8, "visits").view(np.uint32).reshape(n, 2),) if visits else got

    def within(self, n=None, visits=False):
        L, s = _L(), self.state
        n = self.n_max if n is None else n
        self._arm(self.hit, n)
        if visits:
            self._arm(self.visits, n * 8)
            assert L.pt_debug_nearest_k_visits(s.context, self.p, n, 0, None, None, self.hit, self.visits) == 0, _err(s)
        else:
            assert L.pt_query_within_any(s.context, self.p, n, self.hit) == 0, _err(s)
        hit = self._read(self.hit, n, "hit").copy()
        return (hit, self._read(self.visits, n * 8, "visits").view(np.uint32).reshape(n, 2)) if visits else hit

    def nearest(self, n=None):
        """pt_query_nearest on the same points: what record 0 must equal"""
        n = self.n_max if n is None else n
        self._arm(self.one, n * 32)
        assert _L().pt_query_nearest(self.state.context, self.p, n, self.one) == 0, _err(self.state)
        return self._read(self.one, n * 32, "pt_query_nearest's out").view(np.uint32).reshape(n, 8)

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _diff(rec, ref):
    bad = np.flatnonzero((rec != ref).reshape(rec.shape[0], -1).any(axis=1))
    return (bad[:4], rec[bad][:1], rec[bad][:1].view(np.float32), ref[bad][:1], ref[bad][:1].view(np.float32))


def check_all_forms(d, ref, n, ks=KS, what=()):
    """Every form of the two calls on the first n points against the reference (records [*, 8, 8], counts, bytes): each k with
    counts and without, the counts alone, the byte, and record 0 against pt_query_nearest on the device"""
    ref_rec, ref_counts, ref_hit = ref
    first = d.nearest(n)
    assert np.array_equal(first, ref_rec[:n, 0]), what + (n,) + _diff(first, ref_rec[:n, 0])
    for k in ks:
        with_counts, c = d.lists(k, True, n)
        without, none = d.lists(k, False, n)
        assert none is None
        assert np.array_equal(with_counts, ref_rec[:n, :k]), what + (n, k, "with counts") + _diff(with_counts, ref_rec[:n, :k])
        assert np.array_equal(without, ref_rec[:n, :k]), what + (n, k, "without counts") + _diff(without, ref_rec[:n, :k])
        assert np.array_equal(c, ref_counts[:n]), what + (n, k)
        assert np.array_equal(without[:, 0], first)
    none, c = d.lists(0, True, n)
    assert none is None and np.array_equal(c, ref_counts[:n]), what + (n, "counts alone")
    hit = d.within(n)
    assert np.array_equal(hit, ref_hit[:n]) and np.array_equal(hit != 0, ref_counts[:n] != 0), what + (n, "within_any")


def _reference(obj, points):
    return kr.nearest_k_of_scene(obj, points)


def _fresh_state(like, obj, tuning=None):
    """A context of its own with like's parameters and obj's scene; tuning: pt_set_tuning's variant, set before the build"""
    state = pt.PathTracerState()
    C.memmove(C.byref(state.params), C.byref(like.params), C.sizeof(state.params))
    state.params.accumulationBuffer = None
    pt.createDeviceContext(state)
    if tuning is not None:
        assert _L().pt_set_tuning(state.context, 0, tuning) == 0
    pt.buildTheAccelarationStructure(state, obj)
    return state


@pytest.fixture(scope="module")
def scenes(gpu_state_factory):
    """The three scenes, each set up once: the Cornell fixtures under the default variant (fp16 centre / half-extent nodes) and the
    box under an fp32-node variant.  name -> (state, obj)"""
    made = {}
    extra = []

    def get(name):
        if name not in made:
            if name == "fp32":
                base, obj = get("box")
                state = _fresh_state(base, obj, tuning=1)           # variant 1: fp32 nodes
                extra.append(state)
                made[name] = (state, obj)
            else:
                made[name] = gpu_state_factory({"box": BOX, "diffuse": BOX_DIFFUSE}[name], width=97, height=61, max_depth=4, spp=8)
        return made[name]

    yield get
    for s in extra:
        pt.CleanAllTheThings(s)


@pytest.fixture(scope="module")
def references(scenes):
    """(scene, set) -> (points, radius, reference at +inf, reference at the radius), each reference (records [n, 8, 8], counts, bytes)
    by the brute force on the whole set: computed once, shared, never written.  The fp32-node scene is the box: it shares the box's."""
    cache = {}

    def get(scene, name):
        key = ("box" if scene == "fp32" else scene, name)
        if key not in cache:
            state, obj = scenes(key[0])
            verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
            pts = nr.point_set(name, verts, idx, _camera(state), first_hits=lambda rays: _host_closest(state, rays))
            radius = kr.set_radius(name, verts, idx)
            out = (pts, radius, _reference(obj, nr.with_radius(pts, np.inf)), _reference(obj, nr.with_radius(pts, radius)))
            for a in (out[0],) + out[2] + out[3]:
                a.setflags(write=False)
            cache[key] = out
        return cache[key]

    return get


def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@pytest.mark.parametrize("name", nr.POINT_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_lists_counts_and_bytes_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    pts, radius, ref_inf, ref_r = references(scene, name)
    # the set still does what it is there for, by the reference's own answers (tests/test_nearest_k_host.py holds the shares)
    none, few, eight, many = kr.classes(ref_r[1])
    assert none > 0 and few > 0 and (many >= 0.1 or name in ("surface", "wall_planes")), (name, none, few, many)
    assert (ref_inf[1] == len(obj.getIndexBuffer()) // 3).all()
    before = pt.getBvhInfo(state).device_bytes
    for r, ref in ((np.inf, ref_inf), (radius, ref_r)):
        d = Device(state, nr.with_radius(pts, r))
        try:
            for n in SIZES:
                check_all_forms(d, ref, n, what=(scene, name, float(r)))
        finally:
            d.free()
    assert pt.getBvhInfo(state).device_bytes == before


def test_bad_points_between_good_ones(scenes, references):
    state, obj = scenes("box")
    pts, radius, ref_inf, ref_r = references("box", "inside")
    good = nr.with_radius(pts[:64], radius)
    bad, why = nr.bad_points(good[0])
    assert bad.shape[0] < 32
    mixed = good.copy()
    where = 2 * np.arange(bad.shape[0]) + 1                 # every other lane of the first wave
    mixed[where] = bad
    still_good = np.ones(64, bool); still_good[where] = False
    ref = _reference(obj, mixed)
    assert np.array_equal(ref[0][where], kr.miss_lists(where.size, 8)) and not ref[1][where].any() and not ref[2][where].any(), why
    assert np.array_equal(ref[0][still_good], ref_r[0][:64][still_good]) and ref[1][still_good].any()
    d = Device(state, mixed)
    try:
        check_all_forms(d, ref, 64)
    finally:
        d.free()
    # points that look odd and are points: a radius of +-0 on a surface point and beside it, a huge radius whose square overflows
    v = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)[obj.getIndexBuffer()[0], :3]
    odd = np.array([[v[0], v[1], v[2], 0.0], [v[0], v[1], v[2], -0.0], [v[0] + 1.0, v[1] + 1.0, v[2] + 1.0, 0.0], [v[0], v[1], v[2], 1e30]], np.float32)
    assert nr.searchable(odd).all()
    ref = _reference(obj, odd)
    assert ref[1][0] >= 1 and ref[1][1] == ref[1][0] and ref[1][2] == 0 and ref[1][3] == len(obj.getIndexBuffer()) // 3
    d = Device(state, odd)
    try:
        check_all_forms(d, ref, 4)
    finally:
        d.free()


def test_two_calls_give_the_same_bits(scenes, references):
    state, obj = scenes("diffuse")
    pts, radius, ref_inf, ref_r = references("diffuse", "wall_planes")
    d = Device(state, nr.with_radius(pts[:257], radius))
    try:
        a, b = d.lists(8, True), d.lists(8, True)                  # lists() checks the 0xCD guards
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], ref_r[0][:257])
        assert np.array_equal(d.within(), d.within())
    finally:
        d.free()


def test_scene_memory_is_what_it_was(gpu_state_factory):
    """A default scene holds the fp16 nodes only, and the calls leave it so."""
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    before = pt.getBvhInfo(state).device_bytes
    pts = nr.point_set("inside", obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))[:256]
    points = nr.with_radius(pts, kr.set_radius("inside", obj.getVerticesFloat(), obj.getIndexBuffer()))
    d = Device(state, points)
    try:
        check_all_forms(d, _reference(obj, points), 256, ks=(4,))
    finally:
        d.free()
    assert pt.getBvhInfo(state).device_bytes == before


def test_queries_leave_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    pts = nr.point_set("inside", obj.getVerticesFloat(), obj.getIndexBuffer(), _camera(state))
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        pt.queryNearestK(state, pts, k=8, max_radius=80.0, counts=True)
        pt.queryNearestK(state, pts, k=3)
        pt.queryWithinAny(state, pts, 80.0)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_after_scene_edits_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    cam = _camera(state)
    pts = np.concatenate([nr.point_set(name, verts0, idx, cam, first_hits=lambda rays: _host_closest(state, rays))[:300] for name in ("surface", "inside", "wall_planes")])
    points = np.concatenate([nr.with_radius(pts[::3], np.inf), nr.with_radius(pts, kr.set_radius("inside", verts0, idx))])
    n = points.shape[0]
    fresh, devs = [], []

    def run(s, ref):
        d = Device(s, points)
        devs.append(d)
        check_all_forms(d, ref, n, ks=(1, 4, 8))

    try:
        ref0 = _reference(obj, points)
        run(state, ref0)                                         # the queries have run on the scene before it changes
        # 1. a refit: the tall block's and the short block's vertices (everything strictly inside the room) move
        verts = np.array(verts0, np.float32).reshape(-1, 4).copy()
        lo, hi = nr.scene_box(verts, idx)
        inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)
        assert 8 <= inner.sum() < verts.shape[0]
        verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
        info = pt.updateVertices(state, verts, "refit")
        assert not info["rebuilt"]
        moved = pt.TinyObjWrapper(BOX)
        moved._vertices = verts.reshape(-1).copy()
        fresh.append(_fresh_state(state, moved))
        ref1 = _reference(moved, points)
        run(state, ref1)
        run(fresh[-1], ref1)
        assert (ref1[0] != ref0[0]).any() and (ref1[1] != ref0[1]).any()         # the move shows in the answers
        # 2. new material assignments on top: the ids rotate by one
        n_mats = obj.getNumMaterials()
        ids = ((np.asarray(obj.getMaterialIndices(), np.uint32) + 1) % n_mats).astype(np.uint32)
        pt.updateMaterials(state, material_ids=ids)
        moved._materialIndices = ids
        fresh.append(_fresh_state(state, moved))
        ref2 = _reference(moved, points)
        run(state, ref2)
        run(fresh[-1], ref2)
        found = ref1[0][:, :, 1] != MISS
        assert np.array_equal(ref2[0][:, :, :7], ref1[0][:, :, :7]) and (ref2[0][:, :, 7] != ref1[0][:, :, 7])[found].all() and found.mean() >= 0.1
    finally:
        for d in devs:
            d.free()
        for s in fresh:
            pt.CleanAllTheThings(s)


def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    pts, radius, ref_inf, ref_r = references("box", "inside")
    L = _L()
    d = Device(state, nr.with_radius(pts[:256], radius))
    ref = tuple(a[:256] for a in ref_r)
    try:
        check_all_forms(d, ref, 256, ks=(4,))
        ctx, p, o, c, h = state.context, d.p, d.out, d.counts, d.hit
        K = L.pt_query_nearest_k
        refused = {
            "out and counts both null": K(ctx, p, 256, 0, None, None),
            "out null with max_k != 0": K(ctx, p, 256, 4, None, c),
            "out with max_k == 0": K(ctx, p, 256, 0, o, c),
            "max_k too large": K(ctx, p, 256, 9, o, c),
            "null points": K(ctx, None, 256, 4, o, c),
            "too many": K(ctx, p, 0x80000000, 4, o, c),
            "out is the points": K(ctx, p, 256, 4, p, c),
            "out overlaps the points' end": K(ctx, p, 256, 1, p + 255 * 16, None),
            "the points lie inside out": K(ctx, o + 1024, 64, 4, o, None),
            "counts is the points": K(ctx, p, 256, 4, o, p),
            "counts inside out": K(ctx, p, 256, 4, o, o + 256 * 4 * 32 - 4),
            "out inside counts": K(ctx, p, 16, 1, c + 16, c),
            "points not aligned": K(ctx, p + 4, 16, 4, o, c),
            "out not aligned": K(ctx, p, 16, 4, o + 8, c),
            "counts not aligned": K(ctx, p, 16, 4, o, c + 2),
            "null context": K(None, p, 256, 4, o, c),
            "within: null points": L.pt_query_within_any(ctx, None, 256, h),
            "within: null hit": L.pt_query_within_any(ctx, p, 256, None),
            "within: too many": L.pt_query_within_any(ctx, p, 0x80000000, h),
            "within: hit is the points": L.pt_query_within_any(ctx, p, 256, p),
            "within: hit inside the points": L.pt_query_within_any(ctx, p, 256, p + 256 * 16 - 1),
            "within: points not aligned": L.pt_query_within_any(ctx, p + 4, 16, h),
            "within: null context": L.pt_query_within_any(None, p, 256, h),
            "twin: null visits": L.pt_debug_nearest_k_visits(ctx, p, 256, 4, o, c, None, None),
            "twin: hit with a list": L.pt_debug_nearest_k_visits(ctx, p, 256, 4, o, None, h, d.visits),
            "twin: visits overlap out": L.pt_debug_nearest_k_visits(ctx, p, 256, 4, o, None, None, o + 8),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert K(ctx, None, 256, 4, o, c) != 0 and _err(state).startswith("pt_query_nearest_k: ")
        assert K(ctx, p, 256, 9, o, c) != 0 and "at most 8" in _err(state)
        assert K(ctx, p, 256, 0, None, None) != 0 and "nothing to write" in _err(state)
        assert K(ctx, p, 256, 4, None, c) != 0 and "both or neither" in _err(state)
        assert K(ctx, p, 0x80000000, 4, o, c) != 0 and "too many points" in _err(state)
        assert K(ctx, p, 256, 4, p, c) != 0 and "overlaps" in _err(state)
        assert K(ctx, p + 4, 16, 4, o, c) != 0 and "aligned" in _err(state)
        assert L.pt_query_within_any(ctx, p, 256, None) != 0 and _err(state).startswith("pt_query_within_any: ")
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert K(bare, p, 256, 4, o, c) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_within_any(bare, p, 256, h) != 0 and b"no scene" in L.pt_last_error(bare)
            assert K(bare, None, 0, 0, None, None) == 0                        # no points: nothing to do, nothing to refuse
            assert L.pt_query_within_any(bare, None, 0, None) == 0
        finally:
            L.pt_destroy(bare)
        assert K(ctx, None, 0, 4, None, None) == 0 and L.pt_query_within_any(ctx, None, 0, None) == 0
        check_all_forms(d, ref, 256, ks=(4,))                                   # the next valid calls
    finally:
        d.free()


@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_the_counting_twin(scenes, references, scene):
    """pt_debug_nearest_k_visits: the product kernels' bits, and visits that say what the two regimes and the early exit are for —
    without counts no query tests more triangles than with them and on `inside` the sum is strictly smaller; the within-radius walk
    tests no more than k = 1 does, point by point (the same order of visits, left at the first candidate or run to its end)."""
    state, obj = scenes(scene)
    n_tris = len(obj.getIndexBuffer()) // 3
    for name in ("inside", "features"):
        pts, radius, ref_inf, ref_r = references(scene, name)
        n = 257
        d = Device(state, nr.with_radius(pts[:n], radius))
        try:
            tested = {}
            for k in KS:
                rec_c, cnt, vis_c = d.lists(k, True, visits=True)
                rec_p, _, vis_p = d.lists(k, False, visits=True)
                assert np.array_equal(rec_c, ref_r[0][:n, :k]) and np.array_equal(rec_p, ref_r[0][:n, :k]) and np.array_equal(cnt, ref_r[1][:n])
                assert np.array_equal(rec_p, d.lists(k, False)[0])
                assert (vis_p <= vis_c).all(), (name, k)
                assert (vis_c[:, 1] <= n_tris).all() and (vis_c[:, 0] < n_tris).all() and (vis_c[:, 1] >= cnt).all()
                tested[k] = (int(vis_p[:, 1].sum()), int(vis_c[:, 1].sum()))
                if k == 1:
                    vis_1 = vis_p
            _, cnt, vis_0 = d.lists(0, True, visits=True)
            assert np.array_equal(cnt, ref_r[1][:n]) and np.array_equal(vis_0, vis_c)        # with counts every k walks the same nodes
            hit, vis_w = d.within(visits=True)
            assert np.array_equal(hit, ref_r[2][:n]) and np.array_equal(hit, d.within())
            assert (vis_w <= vis_1).all() and (vis_w[hit == 0] == vis_1[hit == 0]).all()
            assert (vis_w[:, 1] >= hit).all()
            print(scene, name, "triangles tested without / with counts per k:", tested, "within_any:", int(vis_w[:, 1].sum()))
            if name == "inside":
                assert all(a < b for a, b in tested.values()), tested
            assert tested[1][0] <= tested[8][0]
        finally:
            d.free()


def test_querynearestk_numpy_path(scenes, references):
    state, obj = scenes("diffuse")
    pts, radius, ref_inf, ref_r = references("diffuse", "inside")
    got = pt.queryNearestK(state, pts, k=5, max_radius=float(radius), counts=True)
    assert got["distance"].dtype == np.float32 and got["prim"].dtype == np.uint32 and got["material"].dtype == np.uint32 and got["count"].dtype == np.uint32
    assert got["point"].shape == (pts.shape[0], 5, 3) and got["u"].shape == (pts.shape[0], 5)
    packed = np.concatenate([got["distance"].view(np.uint32)[..., None], got["prim"][..., None], got["u"].view(np.uint32)[..., None], got["v"].view(np.uint32)[..., None],
                             got["point"].view(np.uint32), got["material"][..., None]], axis=2)
    assert np.array_equal(packed, ref_r[0][:, :5]) and np.array_equal(got["count"], ref_r[1])
    one = pt.queryNearest(state, pts, float(radius))
    assert all(np.array_equal(got[key][:, 0], one[key]) for key in one)
    got = pt.queryNearestK(state, nr.with_radius(pts, np.inf).tolist(), k=2)    # anything np.asarray takes; the radius in the fourth column
    assert "count" not in got and np.array_equal(got["prim"], ref_inf[0][:, :2, 1]) and np.array_equal(got["distance"].view(np.uint32), ref_inf[0][:, :2, 0])
    alone = pt.queryNearestK(state, pts, k=0, max_radius=float(radius), counts=True)
    assert alone["distance"].shape == (pts.shape[0], 0) and np.array_equal(alone["count"], ref_r[1])
    within = pt.queryWithinAny(state, pts, float(radius))
    assert within.dtype == bool and np.array_equal(within, ref_r[2] != 0)
    assert np.array_equal(pt.queryWithinAny(state, nr.with_radius(pts, radius)), within)


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    pts, radius, ref_inf, ref_r = references("box", "inside")
    points = nr.with_radius(pts, radius)
    L = _L()
    seen = {}
    real, real_within = L.pt_query_nearest_k, L.pt_query_within_any
    monkeypatch.setattr(L, "pt_query_nearest_k", lambda ctx, p, n, k, out, c: seen.update(call=(p, n, k, out, c)) or real(ctx, p, n, k, out, c))
    monkeypatch.setattr(L, "pt_query_within_any", lambda ctx, p, n, h: seen.update(within=(p, n, h)) or real_within(ctx, p, n, h))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(points.copy()).to(dev)
    got = pt.queryNearestK(state, x, k=3, counts=True)
    assert seen["call"][:3] == (x.data_ptr(), points.shape[0], 3)
    assert all(v.device == dev for v in got.values())
    assert seen["call"][3] == got["distance"].data_ptr() and seen["call"][4] == got["count"].data_ptr()      # views of what the library wrote
    assert got["distance"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["material"].dtype == torch.int32 and got["count"].dtype == torch.int32
    assert got["point"].shape == (points.shape[0], 3, 3)
    ref = ref_r[0][:, :3]
    cols = {"distance": ref[:, :, 0], "prim": ref[:, :, 1], "u": ref[:, :, 2], "v": ref[:, :, 3], "material": ref[:, :, 7]}
    for key, want in cols.items():
        assert np.array_equal(got[key].cpu().numpy().view(np.uint32), want), key
    assert np.array_equal(got["point"].cpu().numpy().view(np.uint32), ref[:, :, 4:7])
    assert np.array_equal(got["count"].cpu().numpy().view(np.uint32), ref_r[1])
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    again = pt.queryNearestK(state, y, k=3)
    assert seen["call"][0] == y.data_ptr() and seen["call"][4] is None and "count" not in again
    assert torch.equal(again["prim"], got["prim"]) and torch.equal(again["distance"], got["distance"])
    hit = pt.queryWithinAny(state, y)
    assert seen["within"][:2] == (y.data_ptr(), points.shape[0]) and hit.dtype == torch.bool and hit.device == dev
    assert np.array_equal(hit.cpu().numpy(), ref_r[2] != 0)
    for fn in (lambda t: pt.queryNearestK(state, t), lambda t: pt.queryWithinAny(state, t)):
        for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :3].contiguous(), "expected an")):
            with pytest.raises(pt.PathTracerError, match=what):
                fn(bad)
    with pytest.raises(pt.PathTracerError, match="fourth column"):
        pt.queryWithinAny(state, x, 1.0)
    assert pt.queryNearestK(state, x[:0], k=2)["distance"].shape == (0, 2) and pt.queryWithinAny(state, x[:0]).shape == (0,)


def test_spherecontacts_of_a_ball_in_a_corner(scenes):
    """A ball of radius 25 centred 20 from the floor (y = 0), the back wall (z = 559.2) and the green wall (x = 0) of the box: three
    contacts at distance 20 exactly, in the order of their triangles (1, 4, 6), each penetrating by 5, pushed out along +y, -z, +x.
    Next to it a ball that touches nothing and one that only the floor holds, through two triangles or one."""
    state, obj = scenes("box")
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    centres = np.array([[20.0, 20.0, 539.2], [30.0, 30.0, 529.2], [40.0, 10.0, 500.0]], np.float32)
    got = pt.sphereContacts(state, centres, 25.0, max_contacts=4)
    assert got["point"].shape == (3, 4, 3) and got["normal"].shape == (3, 4, 3) and got["penetration"].shape == (3, 4) and got["count"].dtype == np.uint32
    assert [int(c) for c in got["count"][:2]] == [3, 0]
    assert [int(x) for x in got["prim"][0]] == [1, 4, 6, MISS]
    assert np.array_equal(got["penetration"][0, :3], np.full(3, 5.0, np.float32)) and np.isnan(got["penetration"][0, 3]) and np.isnan(got["penetration"][1]).all()
    assert [names[int(m)] for m in got["material"][0, :3]] == ["white", "white", "green"]
    want = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    assert np.abs(got["normal"][0] - want).max() < 1e-5 and not got["normal"][1].any()
    assert np.abs(got["point"][0, :3] - np.array([[20.0, 0.0, 539.2], [20.0, 20.0, 559.2], [0.0, 20.0, 539.2]], np.float32)).max() < 1e-3
    # the third ball rests on the floor alone: every contact is a floor triangle straight below it, penetration 15
    k = int(min(got["count"][2], 4))
    assert 1 <= k <= 2 and np.array_equal(got["penetration"][2, :k], np.full(k, 15.0, np.float32)) and np.abs(got["normal"][2, :k] - [0.0, 1.0, 0.0]).max() < 1e-5
    ref = kr.nearest_k_of_scene(obj, nr.with_radius(centres, 25.0), k=4)
    assert np.array_equal(got["prim"], ref[0][:, :, 1]) and np.array_equal(got["count"], ref[1])
    # a truncated manifold: count says so
    few = pt.sphereContacts(state, centres[:1], 25.0, max_contacts=2)
    assert few["count"][0] == 3 and [int(x) for x in few["prim"][0]] == [1, 4]
    # one radius per ball
    per = pt.sphereContacts(state, centres[:2], [25.0, 35.0], max_contacts=8)
    assert per["count"][0] == 3 and per["count"][1] >= 3 and np.array_equal(per["penetration"][1, :3], np.full(3, 5.0, np.float32))


def test_cli_nearest_k_and_within_print_what_the_wrappers_say(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    far = (hi + np.array([100.0, 50.0, 0.0], np.float32)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    queries = [(20.0, 20.0, F(539.2), 4, 25.0), (20.0, 20.0, F(539.2), 2, None), (far[0], far[1], far[2], 4, 1.0), (F(278.0), F(273.0), F(280.0), 8, F(150.0)), (1.0, 2.0, 3.0, 1, None)]
    queries = [tuple(None if a is None else (a if isinstance(a, int) else float(np.float32(a))) for a in q) for q in queries]
    withins = [(20.0, 20.0, float(F(539.2)), 25.0), (20.0, 20.0, float(F(539.2)), 19.5), (float(far[0]), float(far[1]), float(far[2]), 1.0), (float(far[0]), float(far[1]), float(far[2]), 1e4)]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for x, y, z, k, r in queries:
        cmd += ["--nearest-k", "%r,%r,%r,%d" % (x, y, z, k) + ("" if r is None else ",%r" % r)]
    for w in withins:
        cmd += ["--within", "%r,%r,%r,%r" % w]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"nearest_k"')]
    assert len(lines) == len(queries)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    for (x, y, z, k, r), line in zip(queries, lines):
        point = np.array([[x, y, z, np.inf if r is None else r]], np.float32)
        got = pt.queryNearestK(state, point, k=k, counts=True)
        listed = int((got["prim"][0] != MISS).sum())
        assert np.array_equal(np.array(line["nearest_k"], np.float32), point[0, :3]) and line["k"] == k and line["count"] == int(got["count"][0])
        assert len(line["list"]) == listed == min(k, line["count"])
        for j, e in enumerate(line["list"]):
            assert e["triangle"] == int(got["prim"][0, j]) and np.float32(e["distance"]) == got["distance"][0, j]
            assert e["material"] == names[int(got["material"][0, j])]
            assert np.array_equal(np.array(e["point"], np.float32), got["point"][0, j])
            assert np.float32(e["u"]) == got["u"][0, j] and np.float32(e["v"]) == got["v"][0, j]
    assert [l["count"] for l in lines[:3]] == [3, len(obj.getIndexBuffer()) // 3, 0] and [e["triangle"] for e in lines[0]["list"]] == [1, 4, 6]
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"within"')]
    assert len(lines) == len(withins)
    want = pt.queryWithinAny(state, np.array(withins, np.float32))
    assert [l["hit"] for l in lines] == [bool(w) for w in want] == [True, False, False, True]
    for w, l in zip(withins, lines):
        assert np.array_equal(np.array(l["within"] + [l["radius"]], np.float32), np.array(w, np.float32))
    for flag, args in (("--nearest-k", ("1,2,3", "1,2,nan,4", "1,2,3,0", "1,2,3,9", "1,2,3,2.5", "1,2,3,4,-1", "1,2,3,4,nan")), ("--within", ("1,2,3", "1,2,inf,4", "1,2,3,-1", "1,2,3,nan"))):
        for arg in args:
            bad = subprocess.run([exe, "--obj", BOX, flag, arg], capture_output=True, text=True, timeout=300)
            assert bad.returncode == 2 and flag in bad.stderr, arg
