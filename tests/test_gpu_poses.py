"""Posed-mesh queries on the GPU: pt_pose_triangles against tests/poses_ref.py's transform (bits), pt_query_poses_any and
pt_query_poses_distance against its brute force and against the per-triangle queries on the materialised records, on both Cornell
fixtures, the fp32-node scene and the three build modes; the radii, the ties, the debug hook's flags, the mesh's lifetime, the render
state, the refusals and their order, the wrappers with arrays and tensors and their split over whole poses, the parent's host path
where the two transforms agree, and acgpt_main --collide."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import poses_ref as pr
import tridist_ref as tr

F = np.float32
gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 257, 1000)       # poses: around a wave and a workgroup, and several workgroups
GUARD = 64                               # bytes of 0xCD kept behind every output
MISS = 0xFFFFFFFF


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


def _set_mesh(state, records):
    r = np.ascontiguousarray(records, np.float32)
    assert _L().pt_set_query_mesh(state.context, r.ctypes.data if r.size else None, r.shape[0]) == 0, _err(state)


class _Device:
    """host arrays in device buffers, each output with a guard behind it; the C ABI called as a C caller would"""
    def __init__(self, state):
        self.state, self.bufs = state, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = pt.pathtracer._device_buffers(self.state, 1, max(a.nbytes, 16))[0]
        self.bufs.append(p)
        assert _L().pt_copy_to_device(self.state.context, p, a.ctypes.data, a.nbytes) == 0
        return p

    def out(self, nbytes):
        p = pt.pathtracer._device_buffers(self.state, 1, nbytes + GUARD)[0]
        self.bufs.append(p)
        assert _L().pt_device_memset(self.state.context, p, 0xCD, nbytes + GUARD) == 0
        return p

    def get(self, p, nbytes, dtype):
        raw = np.zeros(nbytes + GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, p, raw.nbytes) == 0
        assert (raw[nbytes:] == 0xCD).all(), "written past the output"
        return raw[:nbytes].view(dtype).copy()

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)
        self.bufs = []


def _posed(state, poses, T):
    d = _Device(state)
    try:
        P = poses.shape[0]
        out = d.out(P * T * 48)
        assert _L().pt_pose_triangles(state.context, d.put(poses), P, out) == 0, _err(state)
        return d.get(out, P * T * 48, np.uint32).reshape(P, T, 12)
    finally:
        d.free()


def _any(state, poses, first=True, flags=None):
    """(hit, first) of pt_query_poses_any, or of the debug hook with flags"""
    d = _Device(state)
    try:
        P = poses.shape[0]
        hit, fst = d.out(P), d.out(P * 4) if first else None
        if flags is None:
            assert _L().pt_query_poses_any(state.context, d.put(poses), P, hit, fst) == 0, _err(state)
        else:
            assert _L().pt_debug_query_poses(state.context, d.put(poses), P, 0.0, hit, fst, None, flags) == 0, _err(state)
        return d.get(hit, P, np.uint8), d.get(fst, P * 4, np.uint32) if first else None
    finally:
        d.free()


def _distance(state, poses, radius, flags=None):
    d = _Device(state)
    try:
        P = poses.shape[0]
        out = d.out(P * 48)
        if flags is None:
            assert _L().pt_query_poses_distance(state.context, d.put(poses), P, radius, out) == 0, _err(state)
        else:
            assert _L().pt_debug_query_poses(state.context, d.put(poses), P, radius, None, None, out, flags) == 0, _err(state)
        return d.get(out, P * 48, np.uint32).reshape(P, 12)
    finally:
        d.free()


def _triangles_any(state, records):
    """the existing pt_query_triangles_any on (n, 12) records"""
    return pt.queryTrianglesAny(state, np.ascontiguousarray(records.view(np.float32)))


def _triangle_distance(state, records, radius):
    """the existing pt_query_triangle_distance's records as uint32 [n, 12]"""
    g = np.ascontiguousarray(records.view(np.float32)).copy()
    g[:, 3] = radius
    d = _Device(state)
    try:
        out = d.out(g.shape[0] * 48)
        assert _L().pt_query_triangle_distance(state.context, d.put(g), g.shape[0], out) == 0, _err(state)
        return d.get(out, g.shape[0] * 48, np.uint32).reshape(-1, 12)
    finally:
        d.free()


def _fresh_state(like, obj, tuning=None, build_mode=None):
    state = pt.PathTracerState()
    C.memmove(C.byref(state.params), C.byref(like.params), C.sizeof(state.params))
    state.params.accumulationBuffer = None
    pt.createDeviceContext(state)
    if tuning is not None:
        assert _L().pt_set_tuning(state.context, 0, tuning) == 0
    if build_mode is not None:
        assert _L().pt_set_build_mode(state.context, build_mode) == 0
    pt.buildTheAccelarationStructure(state, obj)
    return state


@pytest.fixture(scope="module")
def scenes(gpu_state_factory):
    """name -> (state, obj): the Cornell fixtures under the default variant (fp16 centre / half-extent nodes), the box under an
    fp32-node variant and under build modes 0 and 1 (the default is 2); each set up once"""
    made, extra = {}, []

    def get(name):
        if name not in made:
            if name in ("box", "diffuse"):
                made[name] = gpu_state_factory({"box": BOX, "diffuse": BOX_DIFFUSE}[name], width=97, height=61, max_depth=4, spp=8)
            else:
                base, obj = get("box")
                state = _fresh_state(base, obj, tuning=1 if name == "fp32" else None, build_mode={"mode0": 0, "mode1": 1}.get(name))
                extra.append(state)
                made[name] = (state, obj)
        return made[name]

    yield get
    for s in extra:
        pt.CleanAllTheThings(s)


def _expected_records(ref, which, obj):
    """the reference's pose records with this scene's material ids (the two Cornell fixtures share their geometry)"""
    out = ref[which].copy()
    found = out[:, 1] != MISS
    mats = np.asarray(obj.getMaterialIndices(), np.uint32)
    out[found, 3] = mats[out[found, 1]] & tr.SHADE_MAT_MASK
    return out


def _tile(poses, n):
    return np.ascontiguousarray(np.tile(poses, ((n + poses.shape[0] - 1) // poses.shape[0], 1))[:n])


@gpu
@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: "%s-%s" % c)
def test_transform_equals_the_statement(scenes, case):
    state, _ = scenes("box")
    records, poses, _ = pr.case(*case)
    _set_mesh(state, records)
    T = records.shape[0]
    got = _posed(state, poses, T)
    assert np.array_equal(got, pr.transform(poses, records).view(np.uint32)), case
    if case in (("box", "mixed"), ("strip65", "bad"), ("single", "mixed")):
        for n in SIZES:
            many = _tile(poses, n)
            assert np.array_equal(_posed(state, many, T), pr.transform(many, records).view(np.uint32)), (case, n)


@gpu
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32", "mode0", "mode1"])
def test_yes_no_equals_the_reference_and_the_per_triangle_query(scenes, scene):
    state, obj = scenes(scene)
    for case in pr.CASES:
        ref = pr.cornell_reference(*case)
        records, poses = ref["records"], ref["poses"]
        P, T = poses.shape[0], records.shape[0]
        _set_mesh(state, records)
        hit, first = _any(state, poses, first=True)
        assert np.array_equal(hit, ref["hit"]) and np.array_equal(first, ref["first"]), (scene, case, hit, first)
        hit_only, _ = _any(state, poses, first=False)
        assert np.array_equal(hit_only, ref["hit"]), (scene, case)
        again = _any(state, poses, first=True)
        assert np.array_equal(again[0], hit) and np.array_equal(again[1], first)
        # the existing query on the materialised records, reduced on the host
        per = np.asarray(_triangles_any(state, _posed(state, poses, T).reshape(P * T, 12))).reshape(P, T)
        assert np.array_equal(per.any(axis=1), hit != 0), (scene, case)
        assert np.array_equal(np.where(per.any(axis=1), per.argmax(axis=1), MISS).astype(np.uint32), first), (scene, case)


@gpu
def test_yes_no_over_several_workgroups(scenes):
    state, _ = scenes("box")
    for case in (("strip63", "mixed"), ("strip65", "mixed"), ("box", "bad"), ("single", "mixed")):
        ref = pr.cornell_reference(*case)
        _set_mesh(state, ref["records"])
        for n in SIZES:
            many = _tile(ref["poses"], n)
            hit, first = _any(state, many)
            assert np.array_equal(hit, _tile(ref["hit"][:, None], n)[:, 0]) and np.array_equal(first, _tile(ref["first"][:, None], n)[:, 0]), (case, n)


@gpu
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32", "mode0", "mode1"])
def test_distance_records_equal_the_reference_and_the_per_triangle_query(scenes, scene):
    state, obj = scenes(scene)
    for case in pr.CASES:
        ref = pr.cornell_reference(*case)
        records, poses, radius = ref["records"], ref["poses"], ref["radius"]
        P, T = poses.shape[0], records.shape[0]
        _set_mesh(state, records)
        posed = _posed(state, poses, T)
        for r, which in ((np.inf, "out_inf"), (radius, "out_r")):
            want = _expected_records(ref, which, obj)
            got = _distance(state, poses, r)
            assert np.array_equal(got, want), (scene, case, float(r), np.flatnonzero((got != want).any(axis=1))[:4], got[:2], want[:2])
            assert np.array_equal(_distance(state, poses, r), got)
            # the existing query's record of the winning posed triangle, bit for bit, with query_triangle in the place of pad0
            found = np.flatnonzero(got[:, 1] != MISS)
            if found.size:
                win = got[found, 7]
                one = _triangle_distance(state, posed[found, win], r)
                assert (one[:, 7] == 0).all()
                one[:, 7] = win
                assert np.array_equal(one, got[found]), (scene, case, float(r))
        for r in (0.0, np.nan, -1.0):
            want = pr.reduce_distance(ref["rec_inf"], ref["d2"], r)
            found = want[:, 1] != MISS
            want[found, 3] = np.asarray(obj.getMaterialIndices(), np.uint32)[want[found, 1]] & tr.SHADE_MAT_MASK
            got = _distance(state, poses, r)
            assert np.array_equal(got, want), (scene, case, r)
            assert r == 0.0 or not found.any()


@gpu
def test_ties_go_to_the_lowest_mesh_triangle(scenes):
    state, obj = scenes("box")
    for case in (("box", "symmetric"), ("sphere", "symmetric"), ("coincident", "free")):
        ref = pr.cornell_reference(*case)
        _set_mesh(state, ref["records"])
        got = _distance(state, ref["poses"], np.inf)
        for p in range(ref["poses"].shape[0]):
            d2 = ref["d2"][p]
            tied = np.flatnonzero(d2.view(np.uint32) == F(np.nanmin(d2)).view(np.uint32))
            assert tied.size >= 2 and got[p, 7] == tied[0], (case, p, tied, got[p, 7])
    ref = pr.cornell_reference("coincident", "free")
    assert 3 in _distance(state, ref["poses"], np.inf)[:, 7]


@gpu
def test_distance_over_several_workgroups(scenes):
    state, obj = scenes("box")
    for case in (("strip65", "mixed"), ("box", "bad")):
        ref = pr.cornell_reference(*case)
        _set_mesh(state, ref["records"])
        for n in SIZES:
            many = _tile(ref["poses"], n)
            assert np.array_equal(_distance(state, many, np.inf), _tile(ref["out_inf"], n)), (case, n)
            assert np.array_equal(_distance(state, many, ref["radius"]), _tile(ref["out_r"], n)), (case, n)


@gpu
def test_debug_hook_flags_change_no_bit(scenes):
    for scene in ("box", "fp32"):
        state, obj = scenes(scene)
        for case in (("box", "mixed"), ("strip65", "mixed"), ("sphere", "mixed"), ("box", "bad"), ("coincident", "touching")):
            ref = pr.cornell_reference(*case)
            _set_mesh(state, ref["records"])
            poses = _tile(ref["poses"], 300)
            hit, first = _any(state, poses)
            rec = _distance(state, poses, ref["radius"])
            assert np.array_equal(rec, _tile(ref["out_r"], 300))
            for flags in (0, 1, 2, 3):
                h, f = _any(state, poses, flags=flags)
                assert np.array_equal(h, hit) and np.array_equal(f, first), (scene, case, flags)
                assert np.array_equal(_any(state, poses, first=False, flags=flags)[0], hit), (scene, case, flags)
                assert np.array_equal(_distance(state, poses, ref["radius"], flags=flags), rec), (scene, case, flags)
    state, _ = scenes("box")
    d = _Device(state)
    try:
        p = d.put(pr.cornell_reference("box", "mixed")["poses"])
        assert _L().pt_debug_query_poses(state.context, p, 8, 0.0, d.out(8), None, None, 4) == 1 and "flags" in _err(state)
        assert _L().pt_debug_query_poses(state.context, p, 8, 0.0, d.out(8), None, d.out(8 * 48), 0) == 1 and "out goes alone" in _err(state)
    finally:
        d.free()


def _answers(state, ref):
    return _any(state, ref["poses"]) + (_distance(state, ref["poses"], np.inf),)


@gpu
def test_mesh_lifetime(scenes):
    base, obj = scenes("box")
    diffuse_state, diffuse_obj = scenes("diffuse")
    ref = pr.cornell_reference("box", "mixed")
    state = _fresh_state(base, obj)
    try:
        L = _L()
        n, b = C.c_size_t(7), C.c_size_t(7)
        assert L.pt_get_query_mesh(state.context, C.byref(n), C.byref(b)) == 0 and (n.value, b.value) == (0, 0)
        before = pt.getBvhInfo(state).device_bytes
        _set_mesh(state, ref["records"])
        assert pt.getQueryMesh(state) == {"triangles": 12, "device_bytes": 12 * 48}
        assert pt.getBvhInfo(state).device_bytes == before
        _set_mesh(base, ref["records"])
        want = _answers(base, ref)
        got = _answers(state, ref)
        assert all(np.array_equal(a, b_) for a, b_ in zip(got, want))
        assert pt.getBvhInfo(state).device_bytes == before
        # a material edit, a refit and a rebuild with the same vertices, then another scene: the mesh stays and the answers are a fresh context's
        verts = np.ascontiguousarray(np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4))
        ids = ((np.asarray(obj.getMaterialIndices(), np.uint32) + 1) % obj.getNumMaterials()).astype(np.uint32)
        pt.updateMaterials(state, material_ids=ids)
        got = _answers(state, ref)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(np.delete(got[2], 3, axis=1), np.delete(want[2], 3, axis=1)) and np.array_equal(got[2][:, 3], ids[want[2][:, 1]])
        pt.updateMaterials(state, material_ids=np.asarray(obj.getMaterialIndices(), np.uint32))
        for mode in ("refit", "rebuild"):
            pt.updateVertices(state, verts, mode)
            got = _answers(state, ref)
            assert all(np.array_equal(a, b_) for a, b_ in zip(got, want)), mode
        pt.buildTheAccelarationStructure(state, diffuse_obj)
        assert pt.getQueryMesh(state)["triangles"] == 12
        _set_mesh(diffuse_state, ref["records"])
        want_d = _answers(diffuse_state, ref)
        got = _answers(state, ref)
        assert all(np.array_equal(a, b_) for a, b_ in zip(got, want_d))
        # replacing and freeing
        other = pr.cornell_reference("strip65", "mixed")
        _set_mesh(state, other["records"])
        assert pt.getQueryMesh(state) == {"triangles": 65, "device_bytes": 65 * 48}
        assert np.array_equal(_any(state, other["poses"])[1], other["first"])
        _set_mesh(state, np.zeros((0, 12), np.float32))
        assert pt.getQueryMesh(state) == {"triangles": 0, "device_bytes": 0}
        d = _Device(state)
        try:
            assert L.pt_query_poses_any(state.context, d.put(ref["poses"]), 8, d.out(8), None) == 1 and "pt_set_query_mesh first" in _err(state)
        finally:
            d.free()
        big = np.zeros((1, 12), np.float32)
        assert L.pt_set_query_mesh(state.context, big.ctypes.data, (1 << 20) + 1) == 1 and "too many triangles" in _err(state)
        assert L.pt_set_query_mesh(state.context, None, 3) == 1 and "null argument" in _err(state)
        assert L.pt_set_query_mesh(None, big.ctypes.data, 1) == 1
    finally:
        pt.CleanAllTheThings(state)


@gpu
def test_render_state_matches_a_twin_that_never_set_a_mesh(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    ref = pr.cornell_reference("sphere", "mixed")
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        _set_mesh(state, ref["records"])
        _answers(state, ref)
        _distance(state, ref["poses"], ref["radius"])
        _posed(state, ref["poses"], 300)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        assert pt.getBvhInfo(state).device_bytes == before == pt.getBvhInfo(twin).device_bytes
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
        assert bytes(pt.getStats(state))[:24] == bytes(pt.getStats(twin))[:24]          # the ray and path counts
    finally:
        ob.free()


@gpu
def test_refusals_and_their_order(scenes):
    base, obj = scenes("box")
    L = _L()
    ref = pr.cornell_reference("box", "mixed")
    state = pt.PathTracerState()
    C.memmove(C.byref(state.params), C.byref(base.params), C.sizeof(state.params))
    state.params.accumulationBuffer = None
    pt.createDeviceContext(state)
    d = _Device(state)
    try:
        ctx = state.context
        poses = d.put(ref["poses"])
        hit, first, out, tris = d.out(64), d.out(64), d.out(8 * 48), d.out(8 * 12 * 48)
        calls = {"pt_pose_triangles": lambda c, p, P, o=tris: L.pt_pose_triangles(c, p, P, o),
                 "pt_query_poses_any": lambda c, p, P, o=hit, f=first: L.pt_query_poses_any(c, p, P, o, f),
                 "pt_query_poses_distance": lambda c, p, P, o=out: L.pt_query_poses_distance(c, p, P, 1.0, o)}
        for name, call in calls.items():
            def refused(rc, text):
                assert rc == 1 and _err(state).startswith(name + ": ") and text in _err(state), (name, text, rc, _err(state))
            assert call(None, poses, 8) == 1                                    # 1: a null context
            assert call(ctx, None, 0) == 0 and call(ctx, None, 0, None) == 0     # 2: no poses is success, before the null pointers
            refused(call(ctx, None, 8), "null argument")                         # 3
            refused(call(ctx, poses, 8, None), "null argument")
            refused(call(ctx, poses + 4, 0x80000000), "too many poses")          # 4, before the alignment
            refused(call(ctx, poses + 4, 8), "16-byte aligned")                  # 6, before the missing mesh
            if name != "pt_query_poses_any":
                refused(call(ctx, poses, 8, out + 8), "16-byte aligned")
            else:
                refused(call(ctx, poses, 8, hit, first + 2), "4-byte aligned")
                assert call(ctx, poses, 8, hit + 1, None) == 1 and "no query mesh" in _err(state)      # hit needs no alignment
                refused(call(ctx, poses, 8, hit, hit), "overlaps")
            if name != "pt_pose_triangles":                                       # whose output has no bytes while there is no mesh
                refused(call(ctx, poses, 8, poses), "overlaps")                  # 7, before the missing mesh
            refused(call(ctx, poses, 8), "pt_set_query_mesh first")              # 8, before the missing scene
        _set_mesh(state, ref["records"])
        for name, call in calls.items():
            assert call(ctx, poses, 8, poses) == 1 and _err(state).startswith(name + ": ") and "overlaps" in _err(state)      # 7, before the missing scene
            assert call(ctx, poses, 8) == 1 and _err(state).startswith(name + ": ") and "no scene" in _err(state)      # 9
            # 5: 12 triangles times 2^28 poses is past 2^31 - 1; judged before the alignment and the overlaps
            assert call(ctx, poses + 4, 1 << 28) == 1 and "too many posed triangles (2^31 - 1 per call): split the poses" in _err(state)
        # the context is left usable
        pt.buildTheAccelarationStructure(state, obj)
        assert np.array_equal(_any(state, ref["poses"])[1], ref["first"])
        # nothing is written by a call with no poses
        g = d.out(16)
        assert L.pt_query_poses_any(ctx, poses, 0, g, None) == 0 and (d.get(g, 16, np.uint8) == 0xCD).all()
    finally:
        d.free()
        pt.CleanAllTheThings(state)


@gpu
def test_wrappers_arrays_tensors_and_the_split(scenes):
    import torch
    state, obj = scenes("box")
    ref = pr.cornell_reference("strip65", "mixed")
    v, idx = pr.mesh("strip65")
    assert pt.setQueryMesh(state, v, idx) == 65 and pt.getQueryMesh(state)["triangles"] == 65
    poses = ref["poses"]
    want_posed = pr.transform(poses, ref["records"])
    want_first = np.where(ref["hit"] != 0, ref["first"], MISS)
    forms = {"(P, 12)": poses, "(P, 3, 4)": poses.reshape(-1, 3, 4), "(P, 4, 4)": np.concatenate([poses.reshape(-1, 3, 4), np.tile([[[0, 0, 0, 1.0]]], (8, 1, 1))], axis=1)}

    def check_distance(got, want, tensors):
        found = want[:, 1] != MISS
        arr = {k: (a.cpu().numpy() if tensors else a) for k, a in got.items()}
        assert sorted(arr) == ["clearance", "feature", "material", "on_mesh", "on_query", "prim", "query_triangle"]
        assert np.array_equal(arr["clearance"].view(np.uint32), np.where(found, want[:, 0], F(np.inf).view(np.uint32)))
        assert np.array_equal(arr["query_triangle"], np.where(found, want[:, 7].astype(np.int64), -1)) and arr["query_triangle"].dtype == np.int64
        assert np.array_equal(arr["prim"].view(np.uint32), want[:, 1]) and np.array_equal(arr["material"].view(np.uint32), want[:, 3])
        assert np.array_equal(arr["feature"].view(np.uint32), want[:, 2])
        assert np.array_equal(np.ascontiguousarray(arr["on_query"]).view(np.uint32), want[:, 4:7]) and np.array_equal(np.ascontiguousarray(arr["on_mesh"]).view(np.uint32), want[:, 8:11])

    for name, form in forms.items():
        for limit in (pt.POSED_TRIANGLES_MAX, 65 * 3, 65, 1):             # whole poses per call: all, 3, 1, 1
            kw = {"_limit": limit}
            assert np.array_equal(pt.posedTriangles(state, form, **kw).view(np.uint32), want_posed.view(np.uint32)), (name, limit)
            hit = pt.queryPosesAny(state, form, **kw)
            assert hit.dtype == np.bool_ and np.array_equal(hit, ref["hit"] != 0), (name, limit)
            hit, first = pt.queryPosesAny(state, form, first=True, **kw)
            assert np.array_equal(hit, ref["hit"] != 0) and first.dtype == np.uint32 and np.array_equal(first, want_first), (name, limit)
            check_distance(pt.queryPosesDistance(state, form, **kw), ref["out_inf"], False)
            check_distance(pt.queryPosesDistance(state, form, max_radius=ref["radius"], **kw), ref["out_r"], False)
    # one matrix
    assert pt.queryPosesAny(state, poses[1].reshape(3, 4)).tolist() == [bool(ref["hit"][1])]
    # tensors: (P, 12) and (P, 3, 4) go in by data_ptr(), (P, 4, 4) is sliced
    dev = torch.device("cuda", state._device)
    seen = []
    real = _L().pt_query_poses_any
    for name, form in forms.items():
        t = torch.as_tensor(np.array(form, np.float32), device=dev)
        posed = pt.posedTriangles(state, t)
        assert posed.device == t.device and tuple(posed.shape) == (8, 65, 12) and np.array_equal(posed.cpu().numpy().view(np.uint32), want_posed.view(np.uint32))
        hit, first = pt.queryPosesAny(state, t, first=True, _limit=65 * 3)
        assert hit.dtype == torch.bool and first.dtype == torch.int32 and hit.device == t.device
        assert np.array_equal(hit.cpu().numpy(), ref["hit"] != 0) and np.array_equal(first.cpu().numpy().view(np.uint32), want_first)
        check_distance(pt.queryPosesDistance(state, t, max_radius=ref["radius"], _limit=65 * 3), ref["out_r"], True)
        got = pt.pathtracer._pose_records("t", state, t)
        seen.append((name, got.data_ptr() == t.data_ptr()))
        # the posed records feed the per-triangle queries without a copy
        per = pt.queryTrianglesAny(state, posed.view(-1, 12))
        assert np.array_equal(per.view(8, 65).any(1).cpu().numpy(), ref["hit"] != 0)
    assert seen == [("(P, 12)", True), ("(P, 3, 4)", True), ("(P, 4, 4)", False)]
    with pytest.raises(pt.PathTracerError, match="contiguous"):
        pt.queryPosesAny(state, torch.zeros((8, 24), dtype=torch.float32, device=dev)[:, ::2])
    with pytest.raises(pt.PathTracerError, match="float32"):
        pt.queryPosesAny(state, torch.zeros((8, 12), dtype=torch.float64, device=dev))
    # no poses
    assert pt.queryPosesAny(state, np.zeros((0, 12), np.float32)).shape == (0,) and pt.posedTriangles(state, np.zeros((0, 3, 4))).shape == (0, 65, 12)
    assert pt.queryPosesDistance(state, np.zeros((0, 12), np.float32))["clearance"].shape == (0,)


@gpu
def test_against_the_parent_path_where_the_transforms_agree(scenes):
    """identity and pure axis translations: x' = x + t on both paths.  The agreement of the posed vertices is checked here, so that the
    comparison cannot hide a mismatch of the inputs."""
    import torch
    state, obj = scenes("box")
    dev = torch.device("cuda", state._device)
    for mesh_name in ("box", "strip65", "sphere", "probe_last"):
        v, idx = pr.mesh(mesh_name)
        T = idx.shape[0]
        t = np.array([[0, 0, 0], [150, 0, 400], [0, 250, 400], [150, 100, 400], [100, 300, 450], [8, 8, 400], [270, 100, 160], [-40, 200, 300]], np.float64)
        poses34 = np.zeros((len(t), 3, 4), np.float32)
        poses34[:, :, :3] = np.eye(3)
        poses34[:, :, 3] = t
        pt.setQueryMesh(state, v, idx)
        for tensors in (False, True):
            args = (torch.as_tensor(v, device=dev), torch.as_tensor(idx, device=dev), torch.as_tensor(poses34, device=dev)) if tensors else (v, idx, poses34)
            parent = pt.pathtracer._posed_records("t", *args)
            ours = pt.posedTriangles(state, args[2])
            a, b = (x.cpu().numpy() if tensors else x for x in (parent, ours))
            assert a.shape == b.shape == (len(t), T, 12) and np.array_equal(a, b), (mesh_name, tensors)      # the same numbers (a zero's sign decides nothing)
            hit = pt.queryPosesAny(state, args[2])
            old = pt.meshCollisions(state, *args)
            assert np.array_equal(*(x.cpu().numpy() if tensors else x for x in (hit, old))), mesh_name
            assert 0 < int(hit.sum()) < len(t)
            new = pt.queryPosesDistance(state, args[2], max_radius=60.0)
            old = pt.meshClearance(state, *args, max_radius=60.0)
            c_new, c_old = (x.cpu().numpy() if tensors else x for x in (new["clearance"], old["clearance"]))
            assert np.array_equal(np.isfinite(c_new), np.isfinite(c_old))
            fin = np.isfinite(c_new)
            assert (np.abs(c_new[fin].view(np.int32).astype(np.int64) - c_old[fin].view(np.int32).astype(np.int64)) <= 1).all(), mesh_name
            assert fin.any() and (~fin).any()


@gpu
def test_cli_collide(scenes, tmp_path):
    state, obj = scenes("box")
    exe = os.path.join(os.path.dirname(pt.__file__), "acgpt_main")
    v, idx = pr.mesh("box")
    path = tmp_path / "box.obj"
    path.write_text("".join("v %r %r %r\n" % tuple(float(c) for c in p) for p in v) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in f) for f in idx))
    records = pr.records_of(v, idx)
    _set_mesh(state, records)
    for t, radius in (((150.0, 30.0, 400.0), None), ((150.0, 200.0, 400.0), 500.0), ((150.0, 200.0, 400.0), 5.0), ((0.0, 0.0, 0.0), 0.0)):
        arg = "%s,%r,%r,%r" % ((str(path),) + t) + ("" if radius is None else ",%r" % radius)
        if t == (0.0, 0.0, 0.0):
            arg = "%s" % path if radius is None else "%s,0,0,0,%r" % (path, radius)
        run = subprocess.run([exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png"), "--collide", arg],
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        lines = [json.loads(ln) for ln in run.stdout.splitlines() if ln.startswith('{"collide"')]
        assert len(lines) == 1, run.stdout
        got = lines[0]["collide"]
        pose = np.zeros((1, 3, 4), np.float32)
        pose[0, :, :3] = np.eye(3)
        pose[0, :, 3] = t
        hit, first = _any(state, pose.reshape(1, 12))
        assert got["triangles"] == 12 and got["hit"] == int(hit[0]) and got["first"] == (int(first[0]) if hit[0] else -1), got
        if radius is None:
            assert "distance" not in got
        else:
            rec = _distance(state, pose.reshape(1, 12), radius)[0]
            assert got["distance"] == pytest.approx(float(rec[0:1].view(np.float32)[0]), rel=1e-6)
            assert got["query_triangle"] == (int(rec[7]) if rec[1] != MISS else -1) and got["prim"] == (int(rec[1]) if rec[1] != MISS else -1)
