"""Oriented-box overlap queries on the GPU: pt_query_overlap_oriented, pt_query_overlap_oriented_any and
pt_query_overlap_oriented_lists against tests/oriented_ref.py's brute force (every count, index, any byte and CSR list, bits) on every
scene, size, box set and list length — the set at the edge of the orthonormality tolerance among them —, the identity set against
pt_query_overlap on the same device, pt_pose_boxes against its NumPy statement, the posed-mesh implication, the records that are a miss
before any traversal, the outputs' bounds, the refusals, list lengths around the cuts, stale offsets, a refit, the render state, the
counting twin, torch tensors, bakeOccupancy(frame=...) and acgpt_main --overlap-oriented."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import lists_ref as lr
import nearest_ref as nr
import oriented_ref as ob
import poses_ref as pr
import query_scenes as qs

F = np.float32
pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
MAX_PRIMS = (0, 1, 4, 8)
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
GUARD = 64                                         # bytes of 0xCD kept behind every output
REG, LDS = _native.LIST_REGISTER, _native.LIST_SORT_LDS
MISMATCH = "the offsets do not fit"


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


class _DeviceOBoxes:
    """records in a device buffer, and buffers for the outputs with a guard behind each; the C ABI called as a C caller would.  Every
    call may take a prefix of the records."""
    def __init__(self, state, boxes, width=16):
        self.state, self.n, self.width = state, boxes.shape[0], width
        self.boxes = np.ascontiguousarray(boxes, np.float32)
        assert self.boxes.shape == (self.n, width)
        m = max(self.n, 1)
        self.bufs = pt.pathtracer._device_buffers(state, 1, m * 64) + pt.pathtracer._device_buffers(state, 1, m * 32 + GUARD) + \
            pt.pathtracer._device_buffers(state, 1, m * 4 + GUARD) + pt.pathtracer._device_buffers(state, 1, m + GUARD) + \
            pt.pathtracer._device_buffers(state, 1, (m + 1) * 4 + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], self.boxes.ctypes.data, self.boxes.nbytes) == 0

    def _fill(self, buf, nbytes, pattern=0xCD):
        assert _L().pt_device_memset(self.state.context, buf, pattern, nbytes + GUARD) == 0

    def _read(self, buf, nbytes, what, pattern=0xCD):
        raw = np.zeros(nbytes + GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, buf, raw.nbytes) == 0
        assert (raw[nbytes:] == pattern).all(), "%s: written past its end" % what
        return raw[:nbytes]

    def overlap(self, k, counts=True, n=None, fn=None):
        """(prims uint32 [n, k] or None, counts uint32 [n] or None)"""
        n = self.n if n is None else n
        s = self.state
        fn = fn or _L().pt_query_overlap_oriented
        _, d_prims, d_counts = self.bufs[:3]
        self._fill(d_prims, n * k * 4)
        self._fill(d_counts, n * 4)
        assert fn(s.context, self.bufs[0], n, k, d_prims if k else None, d_counts if counts else None) == 0, _err(s)
        prims = self._read(d_prims, n * k * 4, "prims").view(np.uint32).reshape(n, k)
        cnt = self._read(d_counts, n * 4 if counts else 0, "counts").view(np.uint32)
        return (prims if k else None), (cnt if counts else None)

    def any(self, n=None, fn=None):
        n = self.n if n is None else n
        self._fill(self.bufs[3], n)
        assert (fn or _L().pt_query_overlap_oriented_any)(self.state.context, self.bufs[0], n, self.bufs[3]) == 0, _err(self.state)
        return self._read(self.bufs[3], n, "hit")

    def lists(self, n=None, offsets=None, capacity=None, pattern=0xCD, expect_ok=True):
        """(rc, offsets, prims uint32 [capacity], found): the counting call, pt_list_offsets and the fill, or the fill alone on the
        offsets given.  Guards behind offsets, prims and found."""
        n = self.n if n is None else n
        L, s = _L(), self.state
        d_counts, d_off = self.bufs[2], self.bufs[4]
        if offsets is None:
            assert L.pt_query_overlap_oriented(s.context, self.bufs[0], n, 0, None, d_counts) == 0, _err(s)
            self._fill(d_off, (n + 1) * 4)
            total = C.c_uint64(0)
            assert L.pt_list_offsets(s.context, d_counts, n, d_off, C.byref(total)) == 0, _err(s)
            offsets = self._read(d_off, (n + 1) * 4, "offsets").view(np.uint32).copy()
            assert int(offsets[-1]) == total.value
        else:
            offsets = np.ascontiguousarray(offsets, np.uint32)
            assert offsets.shape == (n + 1,)
            assert L.pt_copy_to_device(s.context, d_off, offsets.ctypes.data, offsets.nbytes) == 0
        capacity = int(offsets[-1]) if capacity is None else capacity
        d_prims = pt.pathtracer._device_buffers(s, 1, capacity * 4 + GUARD)[0]
        d_found = pt.pathtracer._device_buffers(s, 1, n * 4 + GUARD)[0]
        try:
            self._fill(d_prims, capacity * 4, pattern)
            self._fill(d_found, n * 4)
            rc = L.pt_query_overlap_oriented_lists(s.context, self.bufs[0], n, d_off, d_prims if capacity else None, capacity, d_found)
            assert (rc == 0) or not expect_ok, _err(s)
            prims = self._read(d_prims, capacity * 4, "prims", pattern).view(np.uint32).copy()
            found = self._read(d_found, n * 4, "found").view(np.uint32).copy()
        finally:
            pt.pathtracer._free_device_buffers(s, [d_prims, d_found])
        return rc, offsets, prims, found

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _reference(verts, idx, boxes):
    """(counts, prims at 8, any, (offsets, prims, counts) in CSR form) by the brute force: computed once per set, never written"""
    m = ob.overlap_matrix(boxes, verts, idx)
    ref = ob.lists_of_matrix(m, ob.MAX_PRIMS) + (lr.csr_of_matrix(m),)
    for a in ref[:3] + ref[3]:
        a.setflags(write=False)
    return ref


def _check_all(state, boxes, ref, sizes=SIZES, ks=MAX_PRIMS, what=()):
    """Every count, index and any byte of the device equals ref at every n and max_prims, with and without counts; the CSR lists of the
    largest n equal the brute force's"""
    counts, prims, hit, csr = ref
    d = _DeviceOBoxes(state, boxes)
    try:
        for n in sizes:
            n = min(n, boxes.shape[0])
            got = d.any(n)
            assert np.array_equal(got, hit[:n]), what + ("any", n, np.flatnonzero(got != hit[:n])[:4])
            for k in ks:
                for with_counts in ((True,) if k == 0 else (True, False)):
                    p, c = d.overlap(k, with_counts, n)
                    if with_counts:
                        assert np.array_equal(c, counts[:n]), what + ("counts", n, k, np.flatnonzero(c != counts[:n])[:4], c[c != counts[:n]][:4], counts[:n][c != counts[:n]][:4])
                    if k:
                        bad = np.flatnonzero((p != prims[:n, :k]).any(axis=1))
                        assert bad.size == 0, what + ("prims", n, k, with_counts, bad[:4], p[bad][:2], prims[:n, :k][bad][:2])
        n = min(max(sizes), boxes.shape[0])
        rc, offsets, lists, found = d.lists(n)
        assert np.array_equal(offsets, csr[0][:n + 1].astype(np.uint32)) and np.array_equal(found, counts[:n]), what + ("lists: offsets, found",)
        assert np.array_equal(lists, csr[1][:int(csr[0][n])]), what + ("lists",)
    finally:
        d.free()


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
    """(scene, set) -> (boxes, reference) by the brute force on the whole set: computed once, shared, never written.  The fp32-node
    scene is the box: it shares the box's."""
    cache = {}

    def get(scene, name):
        key = ("box" if scene == "fp32" else scene, name)
        if key not in cache:
            state, obj = scenes(key[0])
            verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
            boxes = ob.box_set(name, verts, idx)
            boxes.setflags(write=False)
            cache[key] = (boxes, _reference(verts, idx, boxes))
        return cache[key]

    return get


def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@pytest.mark.parametrize("name", ob.BOX_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_counts_lists_and_any_equal_the_brute_force(scenes, references, scene, name):
    state, obj = scenes(scene)
    boxes, ref = references(scene, name)
    counts = ref[0]
    n_tris = len(obj.getIndexBuffer()) // 3
    info = pt.getBvhInfo(state)
    # the set still does what it is there for, by the reference's own answers: a set that lost its finds must not pass vacuously
    if name in ob.MIXED_SETS:
        assert (counts == 0).mean() >= 0.10 and (counts != 0).mean() >= 0.25 and min((counts > k).mean() for k in (1, 4, 8)) >= 0.01
    if name in ("walls_turned", "flat", "far", "identity", "axis_turns"):
        assert (counts != 0).mean() >= 0.25 and (counts == 0).mean() >= 0.10, (name, (counts != 0).mean())
    if name == "tolerance":
        inside = ob.tolerance_kinds(boxes.shape[0]) < 3
        assert np.array_equal(ob.searchable(boxes), inside) and not counts[~inside].any() and (counts[inside] != 0).mean() >= 0.25
    if name == "whole":
        assert (counts == n_tris).all()
    if name == "outside":
        assert not counts.any()
    before = info.device_bytes
    _check_all(state, boxes, ref, what=(scene, name))
    assert pt.getBvhInfo(state).device_bytes == before


@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_identity_set_equals_pt_query_overlap_on_the_same_device(scenes, references, scene):
    """Two kernels, one answer: the exact identity as the 3 x 3 part reproduces the axis-aligned query"""
    state, obj = scenes(scene)
    boxes, ref = references(scene, "identity")
    aabbs = ob.identity_aabbs(obj.getVerticesFloat(), obj.getIndexBuffer())
    assert np.array_equal(aabbs[:, 0:3], boxes[:, 3:12:4]) and np.array_equal(aabbs[:, 3:6], boxes[:, 12:15])
    d, a = _DeviceOBoxes(state, boxes), _DeviceOBoxes(state, aabbs, width=8)
    try:
        p, c = d.overlap(8)
        q, e = a.overlap(8, fn=_L().pt_query_overlap)
        assert np.array_equal(p, q) and np.array_equal(c, e) and c.any()
        assert np.array_equal(d.any(), a.any(fn=_L().pt_query_overlap_any))
    finally:
        d.free(); a.free()


def test_bad_boxes_between_good_ones(scenes, references):
    state, obj = scenes("box")
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    boxes, ref = references("box", "walls_turned")
    good = boxes[:128]
    bad, why = ob.bad_boxes(good[0])
    assert bad.shape[0] == 51 and not ob.searchable(bad).any()
    mixed = good.copy()
    where = 2 * np.arange(bad.shape[0]) + 1                 # every other lane of the first two waves
    mixed[where] = bad
    still_good = np.ones(128, bool); still_good[where] = False
    d = _DeviceOBoxes(state, mixed)
    try:
        p, c = d.overlap(8)
        hit = d.any()
    finally:
        d.free()
    wrong = (c[where] != 0) | (p[where] != 0xFFFFFFFF).any(axis=1) | (hit[where] != 0)
    assert not wrong.any(), [why[i] for i in np.flatnonzero(wrong)]
    assert np.array_equal(c[still_good], ref[0][:128][still_good]) and np.array_equal(p[still_good], ref[1][:128][still_good]) and ref[0][:128][still_good].any()
    _check_all(state, mixed, _reference(verts, idx, mixed), sizes=(128,))
    # records that look odd and are boxes: a point on a vertex with h = +0 and h = -0 under a mirror, junk in the reserved float, an h
    # whose products overflow, the largest finite h
    v = np.asarray(verts, np.float32).reshape(-1, 4)[idx[0], :3]
    mirror = np.diag([-1.0, 1.0, 1.0]).astype(np.float32)
    odd = np.concatenate([ob.as_oboxes([v], [[0, 0, 0]], mirror), ob.as_oboxes([v], [[-0.0, -0.0, -0.0]], ob.rotations(np.random.default_rng(1), 1)),
                          ob.as_oboxes([v + 1], [[0, 0, 0]], mirror), ob.as_oboxes([v], [[1e30, 1e30, 1e30]], ob.rotations(np.random.default_rng(2), 1)),
                          ob.as_oboxes([[1e30, 0, 0]], [[3e38, 3e38, 3e38]], np.eye(3))])
    odd[1, 15] = np.nan
    assert ob.searchable(odd).all()
    ref_odd = _reference(verts, idx, odd)
    assert ref_odd[0][0] >= 1 and ref_odd[0][3] == len(idx) // 3
    _check_all(state, odd, ref_odd, sizes=(5,))


def test_two_calls_give_the_same_bits_and_nothing_is_written_past_n(scenes, references):
    state, obj = scenes("diffuse")
    boxes, ref = references("diffuse", "links")
    d = _DeviceOBoxes(state, boxes[:257])
    try:
        a, b = d.overlap(8), d.overlap(8)                      # overlap() checks the 0xCD guard behind each output
        h1, h2 = d.any(), d.any()
        l1, l2 = d.lists(), d.lists()
    finally:
        d.free()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(h1, h2) and all(np.array_equal(x, y) for x, y in zip(l1[1:], l2[1:]))
    assert np.array_equal(a[0], ref[1][:257]) and np.array_equal(a[1], ref[0][:257]) and np.array_equal(h1, ref[2][:257])


@pytest.mark.parametrize("P", [1, 64, 65, 1000])
def test_pose_boxes_equal_the_numpy_statement(scenes, P):
    state, obj = scenes("box")
    rng = np.random.default_rng(3820 + P)
    poses = pr.as_poses(pr._rigid(ob.rotations(rng, P).astype(np.float64), rng.uniform(-500.0, 500.0, (P, 3))))
    poses[::7, :] *= F(1.5)                                    # any matrix is posed, orthonormal or not
    local_box = np.array([3.5, -20.25, 7.125, 30.0, 0.0, 12.5], np.float32)
    want = ob.pose_boxes(poses, local_box)
    L = _L()
    bufs = pt.pathtracer._device_buffers(state, 1, P * 48) + pt.pathtracer._device_buffers(state, 1, P * 64 + GUARD)
    try:
        assert L.pt_copy_to_device(state.context, bufs[0], poses.ctypes.data, poses.nbytes) == 0
        assert L.pt_device_memset(state.context, bufs[1], 0xCD, P * 64 + GUARD) == 0
        lb = local_box.ctypes.data_as(C.POINTER(C.c_float))
        assert L.pt_pose_boxes(state.context, bufs[0], P, lb, bufs[1]) == 0, _err(state)
        raw = np.zeros(P * 64 + GUARD, np.uint8)
        assert L.pt_copy_to_host(state.context, raw.ctypes.data, bufs[1], raw.nbytes) == 0
        assert (raw[P * 64:] == 0xCD).all()
        assert np.array_equal(raw[:P * 64].view(np.uint32), want.view(np.uint32).reshape(-1))
        # the refusals, and the context after them
        ctx = state.context
        for k, val in ((0, np.nan), (2, np.inf), (3, -1.0), (5, np.nan), (4, np.inf)):
            bad = local_box.copy(); bad[k] = val
            assert L.pt_pose_boxes(ctx, bufs[0], P, bad.ctypes.data_as(C.POINTER(C.c_float)), bufs[1]) != 0 and "local_box" in _err(state)
        refused = {"null poses": L.pt_pose_boxes(ctx, None, P, lb, bufs[1]), "null out": L.pt_pose_boxes(ctx, bufs[0], P, lb, None),
                   "null box": L.pt_pose_boxes(ctx, bufs[0], P, None, bufs[1]), "too many": L.pt_pose_boxes(ctx, bufs[0], 0x80000000, lb, bufs[1]),
                   "poses not aligned": L.pt_pose_boxes(ctx, bufs[0] + 4, 1, lb, bufs[1]),
                   "out not aligned": L.pt_pose_boxes(ctx, bufs[0], 1, lb, bufs[1] + 8), "out is the poses": L.pt_pose_boxes(ctx, bufs[0], P, lb, bufs[0]),
                   "null context": L.pt_pose_boxes(None, bufs[0], P, lb, bufs[1])}
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_pose_boxes(ctx, None, 0, None, None) == 0
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_pose_boxes(bare, bufs[0], P, lb, bufs[1]) == 0, L.pt_last_error(bare)      # needs neither a scene nor a query mesh
        finally:
            L.pt_destroy(bare)
        assert np.array_equal(pt.poseBoxes(state, poses, local_box[:3] - local_box[3:], local_box[:3] + local_box[3:]), want)
    finally:
        pt.pathtracer._free_device_buffers(state, bufs)


@pytest.mark.parametrize("mesh,set_name", [("box", "mixed"), ("sphere", "mixed"), ("box", "touching"), ("box", "deep"), ("strip65", "mixed"), ("box", "free")])
def test_a_pose_whose_padded_box_is_free_does_not_collide(scenes, mesh, set_name):
    state, obj = scenes("box")
    v, idx = pr.mesh(mesh)
    poses = pr.pose_set(set_name, v)
    try:
        pt.setQueryMesh(state, v, idx)
        boxes = pt.posedMeshBoxes(state, v, poses)
        assert ob.searchable(boxes).all()
        free = ~pt.queryOverlapOrientedAny(state, boxes)
        hit = pt.queryPosesAny(state, poses)
        assert not (free & hit).any(), np.flatnonzero(free & hit)
        assert hit.any() or set_name == "free"
        if set_name == "free":
            assert free.any() and not hit.any()                # the box alone clears poses
    finally:
        pt.setQueryMesh(state, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))


def test_refusals_leave_the_context_usable(scenes, references):
    state, obj = scenes("box")
    boxes, ref = references("box", "random")
    L = _L()
    d = _DeviceOBoxes(state, boxes[:256])
    try:
        expected = d.overlap(8)
        b, p, c, h, o = d.bufs
        ctx = state.context
        Q, A, LS = L.pt_query_overlap_oriented, L.pt_query_overlap_oriented_any, L.pt_query_overlap_oriented_lists
        refused = {
            "null boxes": Q(ctx, None, 256, 8, p, c),
            "too many": Q(ctx, b, 0x80000000, 8, p, c),
            "prims and counts both null": Q(ctx, b, 256, 0, None, None),
            "prims null with max_prims != 0": Q(ctx, b, 256, 4, None, c),
            "prims with max_prims == 0": Q(ctx, b, 256, 0, p, c),
            "max_prims too large": Q(ctx, b, 256, 9, p, c),
            "boxes not aligned": Q(ctx, b + 4, 16, 8, p, c),
            "prims not aligned": Q(ctx, b, 16, 8, p + 8, c),
            "counts not aligned": Q(ctx, b, 16, 8, p, c + 2),
            "prims are the boxes": Q(ctx, b, 256, 8, b, c),
            "prims overlap the boxes' end": Q(ctx, b, 256, 8, b + 255 * 64, c),
            "counts lie inside the boxes": Q(ctx, b, 256, 8, p, b + 1024),
            "the boxes lie inside prims": Q(ctx, p + 1024, 64, 8, p, c),
            "counts lie inside prims": Q(ctx, b, 256, 8, p, p + 64),
            "prims lie inside counts": Q(ctx, b, 8, 4, c + 16, c),
            "null context": Q(None, b, 256, 8, p, c),
            "any: null boxes": A(ctx, None, 256, h),
            "any: null hit": A(ctx, b, 256, None),
            "any: too many": A(ctx, b, 0x80000000, h),
            "any: boxes not aligned": A(ctx, b + 8, 16, h),
            "any: hit is the boxes": A(ctx, b, 256, b),
            "any: hit inside the boxes": A(ctx, b, 256, b + 16383),
            "any: null context": A(None, b, 256, h),
            "lists: null boxes": LS(ctx, None, 256, o, p, 64, c),
            "lists: null offsets": LS(ctx, b, 256, None, p, 64, c),
            "lists: null prims with a capacity": LS(ctx, b, 256, o, None, 64, c),
            "lists: too many": LS(ctx, b, 0x80000000, o, p, 64, c),
            "lists: boxes not aligned": LS(ctx, b + 4, 16, o, p, 64, c),
            "lists: offsets not aligned": LS(ctx, b, 16, o + 2, p, 64, c),
            "lists: prims not aligned": LS(ctx, b, 16, o, p + 2, 64, c),
            "lists: found not aligned": LS(ctx, b, 16, o, p, 64, c + 2),
            "lists: capacity too large": LS(ctx, b, 16, o, p, (1 << 63), c),
            "lists: prims are the boxes": LS(ctx, b, 256, o, b, 64, c),
            "lists: offsets lie inside the boxes": LS(ctx, b, 256, b + 64, p, 64, c),
            "lists: found lies inside prims": LS(ctx, b, 16, o, p, 2048, p + 128),
            "lists: found overlaps offsets": LS(ctx, b, 256, o, p, 64, o + 512),
            "lists: null context": LS(None, b, 256, o, p, 64, c),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert Q(ctx, None, 256, 8, p, c) != 0 and _err(state).startswith("pt_query_overlap_oriented: ")
        assert Q(ctx, b, 0x80000000, 8, p, c) != 0 and "too many boxes" in _err(state)
        assert Q(ctx, b, 256, 8, b, c) != 0 and "overlaps" in _err(state)
        assert Q(ctx, b + 4, 16, 8, p, c) != 0 and "aligned" in _err(state)
        assert Q(ctx, b, 256, 9, p, c) != 0 and "max_prims" in _err(state)
        assert Q(ctx, b, 256, 0, None, None) != 0 and "nothing to write" in _err(state)
        assert A(ctx, b, 256, None) != 0 and _err(state).startswith("pt_query_overlap_oriented_any: ")
        assert LS(ctx, b, 256, None, p, 64, c) != 0 and _err(state).startswith("pt_query_overlap_oriented_lists: ")
        assert A(ctx, b, 255, h + 1) == 0, _err(state)           # hit may have any alignment
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert Q(bare, b, 256, 8, p, c) != 0 and b"no scene" in L.pt_last_error(bare)
            assert A(bare, b, 256, h) != 0 and b"no scene" in L.pt_last_error(bare)
            assert LS(bare, b, 256, o, p, 64, c) != 0 and b"no scene" in L.pt_last_error(bare)
            assert Q(bare, None, 0, 8, None, None) == 0 and A(bare, None, 0, None) == 0 and LS(bare, None, 0, None, None, 0, None) == 0
        finally:
            L.pt_destroy(bare)
        assert Q(ctx, None, 0, 0, None, None) == 0 and A(ctx, None, 0, None) == 0 and LS(ctx, None, 0, None, None, 0, None) == 0
        again = d.overlap(8)                                                        # the next valid call
        assert np.array_equal(again[0], expected[0]) and np.array_equal(again[1], expected[1])
        assert np.array_equal(expected[0], ref[1][:256]) and np.array_equal(expected[1], ref[0][:256])
    finally:
        d.free()


# ---- CSR lists: lengths around the cuts, offsets that do not fit ------------------------------------------------------------------------

LADDER_LENGTHS = (0, 1, REG - 1, REG, REG + 1, 63, 64, 65, LDS - 1, LDS, LDS + 1, 5000)


def _ladder_oboxes(lengths):
    """lists_ref's ladder boxes as oriented records under a quarter turn about z: local x is world y, so the local half extents are the
    world ones with x and y exchanged — the same boxes through the rotated path"""
    a = lr.ladder_boxes(lengths)
    turn = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    return ob.as_oboxes(a[:, 0:3], a[:, [4, 3, 5]], turn)


@pytest.mark.parametrize("tuning", [None, 1])
def test_list_lengths_around_the_cuts(tuning):
    """Lengths one below, at and one above kListRegister and kListSortLds in one call, short and long lists in one wave, under both node
    formats; ascending whatever order the walk met them in"""
    lengths = np.array(LADDER_LENGTHS + LADDER_LENGTHS[::-1] + LADDER_LENGTHS[3:] + LADDER_LENGTHS[:3], np.int64)
    v, idx = lr.ladder()
    boxes = _ladder_oboxes(lengths)
    first = ob.overlap_matrix(boxes[:len(LADDER_LENGTHS)], v, idx.reshape(-1))
    assert np.array_equal(first.sum(axis=1), LADDER_LENGTHS)              # the brute force decides the lengths
    want = lr.ladder_expected(lengths)
    c = qs._Ctx.from_arrays(v, idx, np.zeros(len(idx), np.uint32), qs.box()[3], variant=tuning)
    try:
        d = _DeviceOBoxes(qs.state_of(c), boxes)
        try:
            rc, offsets, prims, found = d.lists()
        finally:
            d.free()
        assert np.array_equal(offsets, want[0].astype(np.uint32)) and np.array_equal(found, want[2]) and np.array_equal(prims, want[1])
    finally:
        c.close()


def test_offsets_that_do_not_fit_write_nothing_outside_the_slices(scenes, references):
    state, obj = scenes("box")
    boxes, ref = references("box", "walls_turned")
    other = references("box", "random")[1]
    n = 600
    csr = ref[3]
    w_off, w_counts = csr[0][:n + 1].astype(np.uint32), csr[2][:n]
    cap = int(w_off[-1])
    stale = other[3][0][:n + 1].astype(np.uint32)                        # offsets of a different query set
    assert (np.diff(stale.astype(np.int64)) < w_counts).any()
    down = w_off[::-1].copy()
    shifted = (w_off.astype(np.int64) + 5).astype(np.uint32)
    d = _DeviceOBoxes(state, boxes[:n])
    try:
        for what, offsets, capacity in (("another set's", stale, int(stale[-1])), ("capacity too small", w_off, cap // 2), ("decreasing", down, cap), ("shifted", shifted, cap)):
            for pattern in (0xCD, 0x5A):
                rc, _, prims, found = d.lists(offsets=offsets, capacity=capacity, pattern=pattern, expect_ok=False)
                assert rc != 0 and MISMATCH in _err(state) and _err(state).startswith("pt_query_overlap_oriented_lists: "), (what, _err(state))
                assert np.array_equal(found, w_counts), what              # found is right whatever the offsets say
                inside = np.zeros(capacity, bool)
                for lo, hi in zip(offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)):
                    if lo <= hi <= capacity:
                        inside[lo:hi] = True
                assert (prims[~inside] == np.uint32(pattern * 0x01010101)).all(), what
            for i in range(n):                                           # the slices that do fit and are long enough hold their lists
                lo, hi, k = int(offsets[i]), int(offsets[i + 1]), int(w_counts[i])
                if lo <= hi <= capacity and hi - lo >= k:
                    assert np.array_equal(prims[lo:lo + k], csr[1][int(w_off[i]):int(w_off[i]) + k]) and (prims[lo + k:hi] == 0xFFFFFFFF).all(), (what, i)
        # a margin on every slice is accepted without a flag: the surplus slots hold 0xFFFFFFFF
        roomy = lr.offsets_of(w_counts.astype(np.int64) + 3).astype(np.uint32)
        rc, _, prims, found = d.lists(offsets=roomy)
        assert rc == 0 and np.array_equal(found, w_counts)
        for i in (0, 1, n // 2, n - 1):
            lo, k = int(roomy[i]), int(w_counts[i])
            assert np.array_equal(prims[lo:lo + k], csr[1][int(w_off[i]):int(w_off[i]) + k]) and (prims[lo + k:lo + k + 3] == 0xFFFFFFFF).all()
        rc, offsets, prims, found = d.lists()                            # the next correct call equals the reference
        assert np.array_equal(offsets, w_off) and np.array_equal(prims, csr[1][:cap]) and np.array_equal(found, w_counts)
    finally:
        d.free()


# ---- scene and state ---------------------------------------------------------------------------------------------------------------------

def test_after_a_refit_equals_a_fresh_scene(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    verts0, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    boxes = np.concatenate([ob.box_set(name, verts0, idx)[:400] for name in ("random", "links", "grid_frame", "walls_turned")])
    old = _reference(verts0, idx, boxes)
    _check_all(state, boxes, old, sizes=(boxes.shape[0],), ks=(8,))          # the queries have run on the scene before it changes
    fresh = None
    try:
        # a refit: the tall block's and the short block's vertices (everything strictly inside the room) move
        verts = np.array(verts0, np.float32).reshape(-1, 4).copy()
        lo, hi = nr.scene_box(verts, idx)
        inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)
        assert 8 <= inner.sum() < verts.shape[0]
        verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
        info = pt.updateVertices(state, verts, "refit")
        assert not info["rebuilt"]
        moved = pt.TinyObjWrapper(BOX)
        moved._vertices = verts.reshape(-1).copy()
        fresh = _fresh_state(state, moved)
        ref = _reference(moved.getVerticesFloat(), idx, boxes)
        assert (ref[0] != old[0]).any()                        # the move shows in the answers
        _check_all(state, boxes, ref, sizes=(boxes.shape[0],), ks=(0, 8), what=("refitted",))
        _check_all(fresh, boxes, ref, sizes=(boxes.shape[0],), ks=(0, 8), what=("fresh",))
    finally:
        if fresh is not None:
            pt.CleanAllTheThings(fresh)


def test_queries_leave_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    boxes = ob.box_set("links", obj.getVerticesFloat(), obj.getIndexBuffer())
    frame = np.hstack([ob.rotations(np.random.default_rng(5), 1)[0].astype(np.float64), [[278.0], [274.0], [280.0]]])
    out = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, out), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), out.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        pt.queryOverlapOriented(state, boxes)
        pt.queryOverlapOrientedAny(state, boxes)
        pt.queryOverlapOrientedLists(state, boxes)
        pt.bakeOccupancy(state, (4, 4, 4), bounds=((-300, -300, -300), (300, 300, 300)), counts=True, frame=frame)
        assert pt.getBvhInfo(state).device_bytes == before
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(out.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, out), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        out.free()


# ---- the visit hook -----------------------------------------------------------------------------------------------------------------------

def visits(state, boxes, fn=None, width=16):
    """(counts, visits [n, 2]) of pt_debug_overlap_oriented_visits (or its axis-aligned twin)"""
    L = _L()
    fn = fn or L.pt_debug_overlap_oriented_visits
    n = boxes.shape[0]
    d = _DeviceOBoxes(state, boxes, width)
    vis = pt.pathtracer._device_buffers(state, 1, n * 8)
    try:
        assert fn(state.context, d.bufs[0], n, d.bufs[2], vis[0]) == 0, _err(state)
        counts = np.zeros(n, np.uint32); v = np.zeros((n, 2), np.uint32)
        assert L.pt_copy_to_host(state.context, counts.ctypes.data, d.bufs[2], counts.nbytes) == 0
        assert L.pt_copy_to_host(state.context, v.ctypes.data, vis[0], v.nbytes) == 0
        assert fn(state.context, d.bufs[0], n, d.bufs[2], None) != 0 and "null argument" in _err(state)
        assert fn(state.context, d.bufs[0], n, None, vis[0]) != 0 and "null argument" in _err(state)
        return counts, v
    finally:
        pt.pathtracer._free_device_buffers(state, vis)
        d.free()


@pytest.mark.parametrize("name", ["links", "grid_frame"])
@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_visit_counts_of_the_test_hook(scenes, references, scene, name):
    """The hook's counts are the product's; its visits are bounded by the tree, and far below a brute force's and below what the world
    AABB of the same boxes costs pt_query_overlap — a walk that prunes on the world axes alone must not pass"""
    state, obj = scenes(scene)
    boxes, ref = references(scene, name)
    counts, v = visits(state, boxes)
    info = pt.getBvhInfo(state)
    n_tris = len(obj.getIndexBuffer()) // 3
    assert np.array_equal(counts, ref[0])
    assert (v[:, 1] >= counts).all() and (v[:, 1] <= n_tris).all() and (v[:, 0] <= info.n_nodes).all() and (v[:, 0] >= 1).all()
    _, va = visits(state, ob.world_aabbs(boxes), _L().pt_debug_overlap_visits, 8)
    print("%s %s: %.1f inner nodes and %.1f triangles per box (max %d / %d), %.1f overlap; the world AABBs: %.1f and %.1f" % (
        scene, name, v[:, 0].mean(), v[:, 1].mean(), v[:, 0].max(), v[:, 1].max(), counts.mean(), va[:, 0].mean(), va[:, 1].mean()))
    assert v[:, 1].mean() < n_tris / 4
    assert v[:, 1].mean() <= va[:, 1].mean() and v[:, 0].mean() <= va[:, 0].mean()
    # the other arm of the admission's measurement: the same counts, and the nine further axes only ever prune
    counts15, v15 = visits(state, boxes, _L().pt_debug_overlap_oriented_visits_cross)
    assert np.array_equal(counts15, counts) and (v15 <= v).all() and (v15[:, 0] >= 1).all()
    print("  with the nine cross axes: %.1f inner nodes and %.1f triangles per box" % (v15[:, 0].mean(), v15[:, 1].mean()))


# ---- the front ends -------------------------------------------------------------------------------------------------------------------------

def test_numpy_wrappers(scenes, references):
    state, obj = scenes("diffuse")
    boxes, ref = references("diffuse", "random")
    got = pt.queryOverlapOriented(state, boxes)
    assert got["prim"].dtype == np.uint32 and got["prim"].shape == (boxes.shape[0], 8) and got["count"].dtype == np.uint32
    assert np.array_equal(got["prim"], ref[1]) and np.array_equal(got["count"], ref[0])
    got = pt.queryOverlapOriented(state, boxes.tolist(), max_prims=3, counts=False)          # anything np.asarray takes
    assert sorted(got) == ["prim"] and np.array_equal(got["prim"], ref[1][:, :3])
    got = pt.queryOverlapOriented(state, boxes, max_prims=0)
    assert got["prim"].shape == (boxes.shape[0], 0) and np.array_equal(got["count"], ref[0])
    hit = pt.queryOverlapOrientedAny(state, boxes)
    assert hit.dtype == np.bool_ and np.array_equal(hit.view(np.uint8), ref[2])
    lists = pt.queryOverlapOrientedLists(state, boxes)
    assert np.array_equal(lists["offsets"], ref[3][0].astype(np.uint32)) and np.array_equal(lists["prim"], ref[3][1]) and np.array_equal(lists["count"], ref[0])
    same = pt.orientedBoxes(boxes[:, 3:12:4], boxes[:, 12:15], boxes[:, :12].reshape(-1, 3, 4)[:, :, :3])
    assert np.array_equal(same, boxes)
    tol = references("diffuse", "tolerance")[0]
    with pytest.raises(ValueError, match="orthonormal"):
        pt.queryOverlapOrientedAny(state, tol)
    inside = tol[ob.tolerance_kinds(tol.shape[0]) < 3]
    assert np.array_equal(pt.queryOverlapOriented(state, inside, max_prims=0)["count"], ob.overlap_records(inside, obj.getVerticesFloat(), obj.getIndexBuffer(), 0)[0])


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, references, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    boxes, ref = references("box", "links")
    L = _L()
    seen = {}
    real, real_any, real_lists, real_pose = L.pt_query_overlap_oriented, L.pt_query_overlap_oriented_any, L.pt_query_overlap_oriented_lists, L.pt_pose_boxes
    monkeypatch.setattr(L, "pt_query_overlap_oriented", lambda ctx, b, n, k, p, c: seen.update(call=(b, n, k, p, c)) or real(ctx, b, n, k, p, c))
    monkeypatch.setattr(L, "pt_query_overlap_oriented_any", lambda ctx, b, n, h: seen.update(any=(b, n, h)) or real_any(ctx, b, n, h))
    monkeypatch.setattr(L, "pt_query_overlap_oriented_lists", lambda ctx, b, n, o, p, cap, f: seen.update(lists=(b, n, o, p, cap)) or real_lists(ctx, b, n, o, p, cap, f))
    monkeypatch.setattr(L, "pt_pose_boxes", lambda ctx, p, n, lb, o: seen.update(pose=(p, n, o)) or real_pose(ctx, p, n, lb, o))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(boxes.copy()).to(dev)
    got = pt.queryOverlapOriented(state, x, max_prims=4)
    assert seen["call"][:3] == (x.data_ptr(), boxes.shape[0], 4)
    assert seen["call"][3] == got["prim"].data_ptr() and seen["call"][4] == got["count"].data_ptr()      # the tensors the library wrote
    assert all(v.device == dev for v in got.values()) and got["prim"].dtype == torch.int32 and got["count"].dtype == torch.int32
    assert np.array_equal(got["prim"].cpu().numpy().view(np.uint32), ref[1][:, :4]) and np.array_equal(got["count"].cpu().numpy().view(np.uint32), ref[0])
    only = pt.queryOverlapOriented(state, x, max_prims=0)
    assert seen["call"][3] is None and only["prim"].shape == (boxes.shape[0], 0) and torch.equal(only["count"], got["count"])
    assert sorted(pt.queryOverlapOriented(state, x, counts=False)) == ["prim"] and seen["call"][4] is None
    # a result of torch's own kernels, still in flight on torch's stream when the wrapper is entered
    y = (x * 1.0).contiguous()
    hit = pt.queryOverlapOrientedAny(state, y)
    assert seen["any"][0] == y.data_ptr() and seen["any"][2] == hit.data_ptr() and hit.dtype == torch.bool and hit.device == dev
    assert np.array_equal(hit.cpu().numpy().view(np.uint8), ref[2])
    lists = pt.queryOverlapOrientedLists(state, x)
    assert seen["lists"][0] == x.data_ptr() and seen["lists"][3] == lists["prim"].data_ptr() and lists["prim"].device == dev
    assert np.array_equal(lists["prim"].cpu().numpy().view(np.uint32), ref[3][1]) and np.array_equal(lists["offsets"].cpu().numpy(), ref[3][0].astype(np.int64))
    # a record that is not orthonormal is a miss on the device, not an error
    z = x.clone(); z[:, :12] *= 1.5
    assert not pt.queryOverlapOrientedAny(state, z).any()
    for fn in (pt.queryOverlapOriented, pt.queryOverlapOrientedAny, pt.queryOverlapOrientedLists):
        for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :8].contiguous(), "expected an")):
            with pytest.raises(pt.PathTracerError, match=what):
                fn(state, bad)
    assert pt.queryOverlapOriented(state, x[:0])["prim"].shape == (0, 8) and pt.queryOverlapOrientedAny(state, x[:0]).shape == (0,)
    # poses on the device become records on the device
    v, idx = pr.mesh("box")
    poses = pr.pose_set("mixed", v)
    t = torch.from_numpy(poses.copy()).to(dev)
    recs = pt.poseBoxes(state, t, v.min(axis=0), v.max(axis=0))
    assert seen["pose"] == (t.data_ptr(), poses.shape[0], recs.data_ptr()) and recs.device == dev and recs.shape == (poses.shape[0], 16)
    assert np.array_equal(recs.cpu().numpy(), pt.poseBoxes(state, poses, v.min(axis=0), v.max(axis=0)))
    assert np.array_equal(pt.posedMeshBoxes(state, v, t).cpu().numpy(), pt.posedMeshBoxes(state, v, poses))


def test_bake_occupancy_in_a_frame_against_the_reference(scenes):
    state, obj = scenes("box")
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    lo, hi = nr.scene_box(verts, idx)
    cen = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
    frame = np.hstack([ob.rotations(np.random.default_rng(3830), 1)[0].astype(np.float64), cen[:, None]])
    half = 0.5 * (hi - lo).astype(np.float64)
    bounds = (tuple(-half), tuple(half))
    occ = pt.bakeOccupancy(state, (9, 7, 5), bounds=bounds, frame=frame)
    cnt = pt.bakeOccupancy(state, (9, 7, 5), bounds=bounds, counts=True, frame=frame)
    assert occ.shape == (9, 7, 5) and occ.dtype == np.bool_ and cnt.shape == (9, 7, 5) and cnt.dtype == np.uint32
    cells = pt.occupancyBoxes((9, 7, 5), *bounds, frame=frame)
    assert cells.shape == (315, 16) and ob.searchable(cells).all()
    ref = ob.overlap_records(cells, verts, idx, 0)
    assert np.array_equal(cnt.reshape(-1), ref[0]) and np.array_equal(occ.reshape(-1).view(np.uint8), ref[2])
    assert occ.mean() >= 0.25 and (~occ).mean() >= 0.10
    # the identity frame is the grid of before
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    world = ((float(lo[0]), float(lo[1]), float(lo[2])), (float(hi[0]), float(hi[1]), float(hi[2])))
    assert np.array_equal(pt.bakeOccupancy(state, (5, 5, 5), bounds=world, counts=True, frame=eye), pt.bakeOccupancy(state, (5, 5, 5), bounds=world, counts=True))
    with pytest.raises(ValueError, match="orthonormal"):
        pt.bakeOccupancy(state, (2, 2, 2), bounds=bounds, frame=np.hstack([1.5 * np.eye(3), np.zeros((3, 1))]))


def test_cli_overlap_oriented_prints_what_the_wrapper_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    state, obj = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=1)
    lo, hi = nr.scene_box(obj.getVerticesFloat(), obj.getIndexBuffer())
    c = (F(0.5) * (lo + hi)).astype(np.float32)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32; the quaternions are not normalised
    queries = [(c[0], c[1], c[2], F(250.0), F(180.0), F(120.0), 1.0, 2.0, -0.5, 0.25, None), (lo[0], c[1], c[2], F(0.0), F(30.5), F(200.25), 0.5, 0.5, 0.5, 0.5, 3),
               (c[0], lo[1], c[2], F(50.0), F(0.0), F(50.0), 3.0, 0.0, 4.0, 0.0, 0), (hi[0] + F(400.0), c[1], c[2], F(10.0), F(10.0), F(10.0), 1.0, 0.0, 0.0, 0.0, 8),
               (c[0], c[1], c[2], F(800.0), F(800.0), F(800.0), 0.1, 0.2, 0.3, 0.4, "all")]
    queries = [tuple(a if i == 10 else float(a) for i, a in enumerate(q)) for q in queries]
    cmd = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for q in queries:
        cmd += ["--overlap-oriented", ",".join("%r" % a for a in q[:10]) + ("" if q[10] is None else ",%s" % q[10])]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"overlap_oriented"')]
    assert len(lines) == len(queries)
    quats = np.array([q[6:10] for q in queries], np.float64)
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    boxes = pt.orientedBoxes([q[0:3] for q in queries], [q[3:6] for q in queries], ob._of_quaternions(quats))
    got = pt.queryOverlapOriented(state, boxes)
    lists = pt.queryOverlapOrientedLists(state, boxes)
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    mats = np.asarray(obj.getMaterialIndices(), np.uint32)
    assert got["count"][0] > 8 and got["count"][1] >= 1 and got["count"][2] >= 1 and got["count"][3] == 0 and got["count"][4] == len(mats)
    for i, line in enumerate(lines):
        assert np.array_equal(np.array(line["overlap_oriented"][:6], np.float32), np.array(queries[i][:6], np.float32))
        assert np.allclose(line["overlap_oriented"][6:], quats[i], rtol=0, atol=1e-15)
        assert line["count"] == int(got["count"][i])
        if queries[i][10] == "all":
            want = [int(t) for t in lists["prim"][int(lists["offsets"][i]):int(lists["offsets"][i + 1])]]
        else:
            k = 8 if queries[i][10] is None else queries[i][10]
            want = [int(t) for t in got["prim"][i, :k] if t != 0xFFFFFFFF]
            assert len(want) == min(k, int(got["count"][i]))
        assert line["triangles"] == want
        assert line["materials"] == [names[int(mats[t])] for t in want]
    for arg in ("1,2,3,4,5,6,1,0,0", "1,2,nan,1,1,1,1,0,0,0", "1,2,3,-1,1,1,1,0,0,0", "1,2,3,1,1,inf,1,0,0,0", "1,2,3,1,1,1,0,0,0,0", "1,2,3,1,1,1,1,0,0,0,9",
                "1,2,3,1,1,1,1,0,0,0,-1"):
        bad = subprocess.run([exe, "--obj", BOX, "--overlap-oriented", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--overlap-oriented" in bad.stderr, arg
