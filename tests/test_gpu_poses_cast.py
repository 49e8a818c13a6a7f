"""pt_query_poses_cast on the GPU: every record against the reduction of pt_query_triangle_cast over pt_pose_triangles' records (bits),
for P around a wave and a workgroup, a 20- and a 320-triangle mesh and both node formats, ties to the lowest mesh triangle, the debug
flags, the refusals and their order, a twin context that never called it, the tunnelling case that sampling poses misses, the
wrappers (queryPosesCast, meshCast, advanceUntilContact) with arrays and tensors."""
import ctypes as C
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import poses_ref as pr
import query_scenes as qs
import sweep_ref as sw
import tricast_ref as tc
import test_gpu_poses as gp
import test_gpu_tricast as gt

F = np.float32
pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
P_SIZES = (1, 3, 64, 257)


def _L():
    return _native.hip()


def _err(state):
    return (_L().pt_last_error(state.context) or b"").decode()


def _poses_cast(state, poses, motions, flags=None):
    """pt_query_poses_cast's records as uint32 [P, 8], or the debug hook's with flags"""
    d = gp._Device(state)
    try:
        P = poses.shape[0]
        out = d.out(P * 32)
        if flags is None:
            assert _L().pt_query_poses_cast(state.context, d.put(poses), d.put(motions), P, out) == 0, _err(state)
        else:
            assert _L().pt_debug_query_poses_cast(state.context, d.put(poses), d.put(motions), P, out, flags) == 0, _err(state)
        return d.get(out, P * 32, np.uint32).reshape(P, 8)
    finally:
        d.free()


def _per_triangle(state, poses, motions, T):
    """pt_query_triangle_cast's records of pt_pose_triangles' records with motions[p] behind each, as uint32 [P * T, 8]"""
    posed = gp._posed(state, poses, T).view(np.float32)
    P = poses.shape[0]
    casts = np.zeros((P, T, 16), np.float32)
    casts[:, :, 0:12] = posed
    casts[:, :, 3] = motions[:, None, 3]
    casts[:, :, 12:15] = motions[:, None, 0:3]
    return gt._query(state, casts.reshape(P * T, 16))[0]


def _pose_set(obj, P, radius, seed):
    """P rigid poses inside the room and motions towards points of the scene; every eighth starts in contact with a wall, every
    seventh has a finite tmax, and where P allows one pose and one motion are not finite"""
    verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
    lo, hi, c, diag = sw._extent(verts, idx)
    rng = np.random.default_rng(seed)
    ext = hi.astype(np.float64) - lo
    centre = lo + (0.25 + 0.5 * rng.random((P, 3))) * ext
    touching = np.arange(P) % 8 == 5
    centre[touching, 1] = lo[1] + 0.5 * radius
    poses = pr.as_poses(pr._rigid(pr._rotations(rng, P), centre))
    target = sw._targets(rng, verts, idx, P)[0]
    motions = np.zeros((P, 4), np.float32)
    motions[:, 0:3] = (target - centre) * rng.uniform(0.3, 2.0, (P, 1))
    motions[:, 3] = np.where(np.arange(P) % 7 == 3, rng.uniform(0.05, 1.5, P), np.inf)
    if P >= 64:
        motions[11, 1] = np.nan
        poses[23, 7] = np.inf
        motions[31, 3] = -1.0
        motions[37, 0:3] = 0.0
    return poses, motions


@pytest.fixture(scope="module")
def scenes(gpu_state_factory):
    made, extra = {}, []

    def get(name):
        if name not in made:
            if name == "fp32":
                base, obj = get("box")
                state = gt._fresh_state(base, obj, tuning=1)
                extra.append(state)
                made[name] = (state, obj)
            else:
                made[name] = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
        return made[name]

    yield get
    for s in extra:
        pt.CleanAllTheThings(s)


@pytest.mark.parametrize("level,T", [(0, 20), (2, 320)])
@pytest.mark.parametrize("scene", ["box", "fp32"])
def test_records_equal_the_reduction_of_the_per_triangle_query(scenes, scene, level, T):
    state, obj = scenes(scene)
    v, f = tc.icosphere(level, 25.0)
    mesh = pr.records_of(v, f)
    assert mesh.shape == (T, 12)
    gp._set_mesh(state, mesh)
    before = pt.getBvhInfo(state).device_bytes
    for P in P_SIZES:
        poses, motions = _pose_set(obj, P, 25.0, 5100 + P)
        rec = _poses_cast(state, poses, motions)
        want = tc.reduce_casts(_per_triangle(state, poses, motions, T), P)
        assert np.array_equal(rec, want), (scene, T, P) + gt._diff(rec, want)
        assert np.array_equal(rec, _poses_cast(state, poses, motions))                 # two calls give the same bits
        hit = rec[:, 1] != 0xFFFFFFFF
        if P >= 64:
            col = tc.columns(rec)
            assert 0.4 <= hit.mean() <= 0.99 and (col["t"][hit] == 0).mean() >= 0.05 and (col["t"][hit] > 0).mean() >= 0.4
            assert np.array_equal(rec[[11, 23, 31]], tc.miss_records(3, tc.MISS))
            assert (rec[~hit, 3] == 0xFFFFFFFF).all() and (rec[hit, 3] < T).all() and np.unique(rec[hit, 3]).size >= 8
        if P == 3 and T == 20:                                                          # and the statement itself
            ref = tc.poses_cast(poses, motions, mesh, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices())
            assert np.array_equal(rec, ref), gt._diff(rec, ref)
    assert pt.getBvhInfo(state).device_bytes == before


def test_ties_go_to_the_lowest_mesh_triangle(scenes):
    """every triangle of the mesh twice: the copy with the lower index answers"""
    state, obj = scenes("box")
    v, f = tc.icosphere(0, 25.0)
    mesh = pr.records_of(v, f)
    order = np.random.default_rng(5201).permutation(20)
    gp._set_mesh(state, np.concatenate([mesh[order], mesh]))
    poses, motions = _pose_set(obj, 64, 25.0, 5202)
    rec = _poses_cast(state, poses, motions)
    want = tc.reduce_casts(_per_triangle(state, poses, motions, 40), 64)
    assert np.array_equal(rec, want), gt._diff(rec, want)
    hit = rec[:, 1] != 0xFFFFFFFF
    assert hit.sum() >= 30 and (rec[hit, 3] < 20).all()
    gp._set_mesh(state, mesh)
    single = _poses_cast(state, poses, motions)
    # the same t as the mesh once (which of several mesh triangles with that t answers, and with it the scene triangle and the feature,
    # follows the order)
    assert np.array_equal(rec[:, 0], single[:, 0])


def test_debug_hook_flags_change_no_bit(scenes):
    for scene in ("box", "fp32"):
        state, obj = scenes(scene)
        v, f = tc.icosphere(2, 25.0)
        gp._set_mesh(state, pr.records_of(v, f))
        poses, motions = _pose_set(obj, 65, 25.0, 5301)
        want = _poses_cast(state, poses, motions)
        for flags in (0, _native.POSES_NO_EARLY, _native.POSES_POSE_MAJOR, _native.POSES_NO_EARLY | _native.POSES_POSE_MAJOR):
            assert np.array_equal(_poses_cast(state, poses, motions, flags), want), (scene, flags)
        d = gp._Device(state)
        try:
            assert _L().pt_debug_query_poses_cast(state.context, d.put(poses), d.put(motions), 65, d.out(65 * 32), 4) == 1 and "flags" in _err(state)
        finally:
            d.free()


def test_refusals_and_their_order(scenes):
    base, obj = scenes("box")
    L = _L()
    v, f = tc.icosphere(0, 25.0)
    poses_h, motions_h = _pose_set(obj, 8, 25.0, 5401)
    state = pt.PathTracerState()
    C.memmove(C.byref(state.params), C.byref(base.params), C.sizeof(state.params))
    state.params.accumulationBuffer = None
    pt.createDeviceContext(state)
    d = gp._Device(state)
    try:
        ctx = state.context
        poses, motions, out = d.put(poses_h), d.put(motions_h), d.out(8 * 32)
        name = "pt_query_poses_cast"

        def call(c, p, P, m=motions, o=out):
            return L.pt_query_poses_cast(c, p, m, P, o)

        def refused(rc, text):
            assert rc == 1 and _err(state).startswith(name + ": ") and text in _err(state), (text, rc, _err(state))
        assert call(None, poses, 8) == 1                                    # 1: a null context
        assert call(ctx, None, 0) == 0 and call(ctx, None, 0, None, None) == 0     # 2: no poses is success, before the null pointers
        refused(call(ctx, None, 8), "null argument")                         # 3
        refused(call(ctx, poses, 8, None), "null argument")
        refused(call(ctx, poses, 8, motions, None), "null argument")
        refused(call(ctx, poses + 4, 0x80000000), "too many poses")          # 4, before the alignment
        refused(call(ctx, poses + 4, 8), "16-byte aligned")                  # 6, before the missing mesh
        refused(call(ctx, poses, 8, motions + 4), "16-byte aligned")
        refused(call(ctx, poses, 8, motions, out + 8), "16-byte aligned")
        refused(call(ctx, poses, 8, motions, poses), "overlaps")             # 7, before the missing mesh
        refused(call(ctx, poses, 8, motions, motions), "overlaps")
        refused(call(ctx, poses, 8, poses), "overlaps")
        refused(call(ctx, poses, 8), "pt_set_query_mesh first")              # 8, before the missing scene
        gp._set_mesh(state, pr.records_of(v, f))
        refused(call(ctx, poses, 8, motions, poses), "overlaps")             # 7, before the missing scene
        refused(call(ctx, poses, 8), "no scene")                             # 9
        # 5: 20 triangles times 2^27 poses is past 2^31 - 1; judged before the alignment and the overlaps
        refused(call(ctx, poses + 4, 1 << 27), "too many posed triangles (2^31 - 1 per call): split the poses")
        # the context is left usable
        pt.buildTheAccelarationStructure(state, obj)
        rec = _poses_cast(state, poses_h, motions_h)
        assert np.array_equal(rec, tc.reduce_casts(_per_triangle(state, poses_h, motions_h, 20), 8)) and (rec[:, 1] != 0xFFFFFFFF).any()
        # nothing is written by a call with no poses
        g = d.out(32)
        assert L.pt_query_poses_cast(ctx, poses, motions, 0, g) == 0 and (d.get(g, 32, np.uint8) == 0xCD).all()
    finally:
        d.free()
        pt.CleanAllTheThings(state)


def test_render_state_matches_a_twin_that_never_called_it(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    v, f = tc.icosphere(2, 25.0)
    poses, motions = _pose_set(obj, 64, 25.0, 5501)
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        gp._set_mesh(state, pr.records_of(v, f))
        assert (_poses_cast(state, poses, motions)[:, 1] != 0xFFFFFFFF).any()
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        assert pt.getBvhInfo(state).device_bytes == before == pt.getBvhInfo(twin).device_bytes
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_a_motion_across_a_thin_wall_is_stopped_where_sampled_poses_tunnel():
    """A wall of two triangles in the plane x = 0 and a unit tetrahedron whose corner B leads at x = -3: both end poses of the motion
    (8, 0, 0) are free, and the cast stops it where B reaches the wall, at t = 3 / 8 in (0, 0.5, 0.25) — exact in fp32."""
    wall = np.array([[0, -8, -8, 0], [0, 8, -8, 0], [0, 8, 8, 0], [0, -8, 8, 0]], np.float32)
    c = qs._Ctx.from_arrays(wall, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.zeros(2, np.uint32), qs.box()[3])
    try:
        state = qs.state_of(c)
        tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
        faces = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
        assert pt.setQueryMesh(state, tet, faces) == 4
        start, end = pr._translations([[-4.0, 0.5, 0.25]])[0], pr._translations([[4.0, 0.5, 0.25]])[0]
        assert not pt.queryPosesAny(state, np.stack([start, end])).any()
        got = pt.queryPosesCast(state, start[None], [[8.0, 0.0, 0.0, 1.0]])
        assert got["t"][0] == F(0.375) and got["prim"][0] == 0 and got["feature"][0] == 1 and got["query_triangle"][0] == 0
        assert np.array_equal(got["point"][0], np.array([0.0, 0.5, 0.25], np.float32)) and got["material"][0] == 0
        # too short to reach the wall; from the wall's other side; along the wall
        miss = pt.queryPosesCast(state, np.stack([start, end, start]), [[8.0, 0.0, 0.0, 0.25], [8.0, 0.0, 0.0, np.inf], [0.0, 1.0, 0.0, np.inf]])
        assert (miss["t"] == -1).all() and (miss["query_triangle"] == 0xFFFFFFFF).all()
        assert pt.queryPosesCast(state, start[None], [[8.0, 0.0, 0.0, 0.375]])["t"][0] == F(0.375)      # tmax is closed
        path = pt.advanceUntilContact(state, np.stack([pr._translations([[-6.0, 0.5, 0.25]])[0], start, end]))
        assert path["leg"] == 1 and path["t"] == 0.375 and np.array_equal(path["pose"][:, 3], np.array([-1.0, 0.5, 0.25], np.float32))
        assert path["contact"]["prim"] == 0
        free = pt.advanceUntilContact(state, np.stack([start, pr._translations([[-4.0, 5.0, 0.25]])[0]]))
        assert free["leg"] == -1 and free["contact"] is None and free["t"] == 1.0
        normal, overlap = pt.castContacts(got, tc.posed_casts(pr.as_poses(start[None]), np.array([[8.0, 0.0, 0.0, 1.0]], np.float32), pr.records_of(tet, faces))[0:1], wall, [0, 1, 2, 0, 2, 3])
        assert np.array_equal(normal, np.array([[-1.0, 0.0, 0.0]], np.float32)) and not overlap.any()
    finally:
        c.close()


def test_wrappers_arrays_and_tensors(scenes):
    import torch
    state, obj = scenes("box")
    v, f = tc.icosphere(0, 25.0)
    assert pt.setQueryMesh(state, v, f) == 20
    poses, motions = _pose_set(obj, 65, 25.0, 5601)
    want = _poses_cast(state, poses, motions)
    col = tc.columns(want)
    got = pt.queryPosesCast(state, poses.reshape(-1, 3, 4), motions)
    via = pt.meshCast(state, v, f, poses.reshape(-1, 3, 4), motions)
    for k in col:
        assert np.array_equal(np.asarray(got[k]).view(np.uint32), col[k].view(np.uint32)), k
        assert np.array_equal(np.asarray(via[k]).view(np.uint32), col[k].view(np.uint32)), k
    # (P, 3) motions: tmax = +inf
    free = motions.copy(); free[:, 3] = np.inf
    assert np.array_equal(pt.queryPosesCast(state, poses, motions[:, :3])["t"].view(np.uint32), _poses_cast(state, poses, free)[:, 0])
    dev = torch.device("cuda", 0)
    tp, tm = torch.from_numpy(poses.copy()).to(dev), torch.from_numpy(motions.copy()).to(dev)
    tg = pt.queryPosesCast(state, tp, tm)
    assert all(x.device == dev for x in tg.values()) and tg["prim"].dtype == torch.int32 and tg["query_triangle"].dtype == torch.int32
    for k in col:
        assert np.array_equal(tg[k].cpu().numpy().view(np.uint32), col[k].view(np.uint32)), k
    with pytest.raises(pt.PathTracerError, match="tensor"):
        pt.queryPosesCast(state, tp, motions)
    with pytest.raises(pt.PathTracerError, match="poses and"):
        pt.queryPosesCast(state, tp, tm[:3].contiguous())
    assert pt.queryPosesCast(state, poses[:0], motions[:0])["t"].shape == (0,)


def test_cli_cast_and_cast_mesh_print_what_the_wrappers_say(scenes, tmp_path):
    import json
    import subprocess
    state, obj = scenes("box")
    exe = os.path.join(os.path.dirname(pt.__file__), "acgpt_main")
    names = [l.split()[1] for l in open(os.path.splitext(BOX)[0] + ".mtl") if l.startswith("newmtl")]
    common = [exe, "--obj", BOX, "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    # fp32 values, printed as the doubles they are: the app reads back the same fp32.  Straight down on the floor or a block, the same
    # with a tmax that ends in mid-air, a start overlap with the floor, away from the box
    tri = (250.0, 300.0, 250.0, 280.0, 305.0, 250.0, 250.0, 310.0, 285.0)
    queries = [tri + (0.0, -1.0, 0.0, None), tri + (0.0, -1.0, 0.0, 5.0), (250.0, -10.0, 250.0, 280.0, 30.0, 250.0, 250.0, 30.0, 285.0, 1.0, 0.0, 0.0, None),
               tuple(c + 2000.0 for c in tri) + (1.0, 0.0, 0.0, None)]
    cmd = list(common)
    for q in queries:
        cmd += ["--cast", ",".join("%r" % a for a in q if a is not None)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"cast"')]
    assert len(lines) == len(queries)
    casts = tc.pack(np.array([q[:9] for q in queries]).reshape(-1, 3, 3), np.array([q[9:12] for q in queries]), np.array([np.inf if q[12] is None else q[12] for q in queries]))
    got = pt.queryTriangleCast(state, casts)
    assert got["t"][0] > 0 and got["prim"][1] == 0xFFFFFFFF and got["feature"][2] == 15 and got["prim"][3] == 0xFFFFFFFF
    for i, line in enumerate(lines):
        assert np.array_equal(np.array(line["cast"], np.float32), casts[i, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]) and line["tmax"] == queries[i][12]
        if got["prim"][i] == 0xFFFFFFFF:
            assert line == {"cast": line["cast"], "tmax": line["tmax"], "hit": False}
            continue
        assert line["hit"] is True and line["triangle"] == int(got["prim"][i]) and line["feature"] == int(got["feature"][i])
        assert np.float32(line["t"]) == got["t"][i] and line["material"] == names[int(got["material"][i])]
        assert np.array_equal(np.array(line["point"], np.float32), got["point"][i])
    for arg in ("1,2,3,4,5,6,7,8,9,0,1", "1,2,3,4,5,6,7,8,9,0,1,nan", "1,2,3,4,5,6,7,8,9,0,1,0,-2", "1,2,inf,4,5,6,7,8,9,0,1,0"):
        bad = subprocess.run([exe, "--obj", BOX, "--cast", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--cast" in bad.stderr, (arg, bad.returncode, bad.stderr)
    # a mesh of its own: the icosphere above the floor
    v, f = tc.icosphere(0, 25.0)
    v = (v + np.array([250.0, 300.0, 250.0], np.float32)).astype(np.float32)
    path = tmp_path / "ball.obj"
    path.write_text("".join("v %r %r %r\n" % tuple(float(c) for c in p) for p in v) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in f))
    assert pt.setQueryMesh(state, v, f) == 20
    identity = np.eye(4, dtype=np.float32)[None, :3, :]
    for motion, tmax in (((0.0, -2.0, 0.0), None), ((0.0, -2.0, 0.0), 10.0), ((0.0, 3.0, 0.5), None)):
        arg = "%s,%r,%r,%r" % ((str(path),) + motion) + ("" if tmax is None else ",%r" % tmax)
        run = subprocess.run(common + ["--cast-mesh", arg], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"cast_mesh"')]
        assert len(lines) == 1, run.stdout
        line = lines[0]
        want = pt.queryPosesCast(state, identity, [list(motion) + [np.inf if tmax is None else tmax]])
        assert line["triangles"] == 20 and line["motion"] == list(motion) and line["tmax"] == tmax
        assert line["hit"] == bool(want["t"][0] >= 0)
        if line["hit"]:
            assert np.float32(line["t"]) == want["t"][0] and line["triangle"] == int(want["prim"][0]) and line["query_triangle"] == int(want["query_triangle"][0])
            assert line["feature"] == int(want["feature"][0]) and np.array_equal(np.array(line["point"], np.float32), want["point"][0])
    assert pt.queryPosesCast(state, identity, [[0.0, -2.0, 0.0, np.inf]])["t"][0] > 0 and pt.queryPosesCast(state, identity, [[0.0, -2.0, 0.0, 10.0]])["t"][0] == -1
    for arg in (str(path), "%s,1,2" % path, "%s,1,2,nan" % path, "%s,1,2,3,-1" % path):
        bad = subprocess.run([exe, "--obj", BOX, "--cast-mesh", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--cast-mesh" in bad.stderr, (arg, bad.returncode, bad.stderr)
