"""Temporal reprojection across vertex updates on the GPU: pt_temporal_blend_motion against tests/motion_ref.py on GPU-made features and
accumulations under three deformations, the static blend's bits where nothing moved, the gain the CPU calibration promises
(tests/test_motion_host.py), the state it must leave alone, the group context, the refusals, pathtracer.TemporalHistory(motion=True)
and acgpt_main --move-history."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import motion_ref as mr
import temporal_ref as tr
from scene_utils import image_mse
from test_gpu_temporal import KW, _Dev, _view
from test_motion_host import F_MOTION

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")


def _deformed(path, kind):
    v = np.ascontiguousarray(pt.TinyObjWrapper(path).getVerticesFloat(), np.float32).reshape(-1, 4)
    if kind == "sphere":
        return v, mr.translated(v, mr.object_vertices(path, "glass_sphere"), mr.SPHERE_MOVE)
    if kind == "blob":
        return v, mr.rotated_about_y(v, mr.object_vertices(path, "blob"), 35.0)
    return v, mr.jittered(v, 9, 0.4)


def _motion(state, q, n, feats, prev, prev_hist, prev_feats, verts, prev_verts, n_verts, cap, gamma, out):
    return _native.hip().pt_temporal_blend_motion(state.context, C.byref(q), n, feats[0], feats[1], C.byref(prev) if prev is not None else None,
                                                  prev_hist, prev_feats[0] if prev_feats else None, prev_feats[1] if prev_feats else None,
                                                  verts, prev_verts, n_verts, cap, gamma, out)


def _static(state, q, n, feats, prev, prev_hist, prev_feats, cap, out):
    return _native.hip().pt_temporal_blend(state.context, C.byref(q), n, feats[0], feats[1], C.byref(prev), prev_hist, prev_feats[0],
                                           prev_feats[1], cap, out)


def _moved_views(state, dev, path, kind, size, prev_size, orbit=(20, 0)):
    """History (32 spp) and features of the unmoved scene at the reference camera, then the scene deformed (pt_update_vertices) and
    one 8-spp launch with features at `orbit`; the two position arrays on the device."""
    (w, h), (wp, hp) = size, prev_size
    v0, v1 = _deformed(path, kind)
    pq, hist, _, pf = _view(state, dev, wp, hp, (0, 0), 32)
    hist[..., 3] = 32.0
    pt.updateVertices(state, v1)
    q, acc, acc_d, f = _view(state, dev, w, h, orbit, 8)
    return dict(v0=v0, v1=v1, pq=pq, hist=hist, hist_d=dev.put(hist), pf=pf, q=q, acc=acc, acc_d=acc_d, f=f, vd=dev.put(v1), vd0=dev.put(v0))


@pytest.mark.parametrize("scene", [BOX, BOX_DIFFUSE])
@pytest.mark.parametrize("kind", ["sphere", "blob", "jitter"])
@pytest.mark.parametrize("size,prev_size", [((256, 192), (256, 192)), ((97, 61), (128, 80))])
def test_motion_blend_equals_the_numpy_reference(gpu_state_factory, scene, kind, size, prev_size):
    (w, h), (wp, hp) = size, prev_size
    state, obj = gpu_state_factory(scene, width=w, height=h, spp=8, **KW)
    dev = _Dev(state)
    try:
        m = _moved_views(state, dev, scene, kind, size, prev_size)
        out_d = dev.alloc(w * h * 16)
        prev_feat = [dev.get(p, hp, wp) for p in m["pf"]]
        feat = [dev.get(p, h, w) for p in m["f"]]
        idx = np.asarray(obj.getIndexBuffer(), np.uint32)
        n_verts = m["v0"].shape[0]
        for cap in (256.0, 12.0):
            for gamma in (0.0, pt.TEMPORAL_CLIP_GAMMA):
                assert _motion(state, m["q"], 8, m["f"], m["pq"], m["hist_d"], m["pf"], m["vd"], m["vd0"], n_verts, cap, gamma, out_d) == 0, \
                    _native.hip().pt_last_error(state.context)
                got = dev.get(out_d, h, w)
                ref, took = mr.blend(m["acc"], feat[0], feat[1], tr.camera_of(m["q"]), 8, tr.tri_bsdf(obj), cap,
                                     (tr.camera_of(m["pq"]), m["hist"], *prev_feat), idx, m["v1"], m["v0"], gamma)
                assert np.array_equal(got[..., 3].view(np.uint32), ref[..., 3].view(np.uint32))
                assert np.array_equal(got[..., 3] != 8.0, took)
                bad = ~(np.abs(got[..., :3] - ref[..., :3]) <= 1e-6 * np.abs(ref[..., :3]))
                assert not bad.any(), "%d channels off, worst %s vs %s" % (bad.sum(), got[..., :3][bad][:4], ref[..., :3][bad][:4])
                print("%s %s %s <- %s cap %g gamma %g: %.3f take history, %.4f bit-identical" % (os.path.basename(scene), kind, size, prev_size,
                      cap, gamma, took.mean(), (got.view(np.uint32) == ref.view(np.uint32)).mean()))
                assert took.mean() > 0.3
    finally:
        dev.close()


def test_unmoved_vertices_give_the_static_blend(gpu_state_factory):
    state, obj = gpu_state_factory(BOX_DIFFUSE, width=97, height=61, spp=8, **KW)
    dev = _Dev(state)
    try:
        pq, hist, _, pf = _view(state, dev, 128, 80, (0, 0), 32)
        hist[..., 3] = 32.0
        hd = dev.put(hist)
        q, _, _, f = _view(state, dev, 97, 61, (20, 0), 8)
        v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
        a, b = dev.put(v), dev.put(v)
        want_d, got_d = dev.alloc(97 * 61 * 16), dev.alloc(97 * 61 * 16)
        for cap in (256.0, 12.0):
            assert _static(state, q, 8, f, pq, hd, pf, cap, want_d) == 0
            want = dev.get(want_d, 61, 97)
            for verts in ((a, b), (None, None)):
                assert _motion(state, q, 8, f, pq, hd, pf, *verts, v.shape[0], cap, 0.0, got_d) == 0, _native.hip().pt_last_error(state.context)
                assert np.array_equal(dev.get(got_d, 61, 97).view(np.uint32), want.view(np.uint32))
    finally:
        dev.close()


def test_gains_what_the_cpu_calibration_says(gpu_state_factory):
    state, obj = gpu_state_factory(BOX_DIFFUSE, width=256, height=256, spp=8, **KW)
    dev = _Dev(state)
    try:
        v0, v1 = _deformed(BOX_DIFFUSE, "sphere")
        pq, hist, _, pf = _view(state, dev, 256, 256, (0, 0), 256)                 # 256 spp of the unmoved scene
        hist[..., 3] = 256.0
        hist_d = dev.put(hist)
        pt.updateVertices(state, v1)
        q, noisy, _, f = _view(state, dev, 256, 256, (0, 0), 8)                      # one 8-spp launch of the moved scene
        _, truth, _, _ = _view(state, dev, 256, 256, (0, 0), 256, frames=32)         # 8192 spp of the moved scene
        out_d = dev.alloc(256 * 256 * 16)
        vd, vd0 = dev.put(v1), dev.put(v0)
        res = {}
        for name, gamma in (("g0", 0.0), ("default", pt.TEMPORAL_CLIP_GAMMA)):
            assert _motion(state, q, 8, f, pq, hist_d, pf, vd, vd0, v0.shape[0], pt.TEMPORAL_HISTORY_CAP, gamma, out_d) == 0
            res[name] = image_mse(dev.get(out_d, 256, 256), truth)
        assert _static(state, q, 8, f, pq, hist_d, pf, pt.TEMPORAL_HISTORY_CAP, out_d) == 0
        res["static"] = image_mse(dev.get(out_d, 256, 256), truth)
        mse_noisy = image_mse(noisy, truth)
        print("MSE 8 spp %.3e static %.3e motion gamma 0 %.3e default %.3e (F %.2f)" % (mse_noisy, res["static"], res["g0"], res["default"],
              mse_noisy / res["default"]))
        assert mse_noisy / res["default"] >= 0.9 * F_MOTION
        assert res["default"] <= res["g0"] < res["static"]
    finally:
        dev.close()


def test_leaves_the_render_state_alone_and_repeats(gpu_state_factory):
    kw = dict(width=96, height=64, spp=8, **KW)
    state, obj = gpu_state_factory(BOX_DIFFUSE, **kw)
    fast, _ = gpu_state_factory(BOX_DIFFUSE, math_mode="fast", **kw)
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    dev, dev_fast = _Dev(state), _Dev(fast)
    L = _native.hip()
    try:
        v0, v1 = _deformed(BOX_DIFFUSE, "sphere")
        pq, hist, _, pf = _view(state, dev, 80, 72, (0, 0), 16)
        hist[..., 3] = 16.0
        hist_d = dev.put(hist)
        n_tris = obj.getIndexBuffer().size // 3
        state.params.currentFrameIdx = 0
        pt.LaunchCurrentFrame(ob, state)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        f = (dev.alloc(96 * 64 * 16), dev.alloc(96 * 64 * 16))
        assert L.pt_render_features(state.context, C.byref(state.params), f[0], f[1]) == 0
        vd, vd0 = dev.put(v0), dev.put(v1)         # the scene as it is now, and the sphere elsewhere in the previous view
        out_d = dev.alloc(96 * 64 * 16)
        g = pt.TEMPORAL_CLIP_GAMMA
        assert _motion(state, state.params, 8, f, pq, hist_d, pf, vd, vd0, v0.shape[0], 256.0, g, out_d) == 0, L.pt_last_error(state.context)
        first = dev.get(out_d, 64, 96)
        grown = pt.getBvhInfo(state).device_bytes
        assert grown == before + n_tris + 12 * n_tris               # the bsdfType array and the index buffer, once
        for _ in range(2):
            assert _motion(state, state.params, 8, f, pq, hist_d, pf, vd, vd0, v0.shape[0], 256.0, g, out_d) == 0
            assert np.array_equal(dev.get(out_d, 64, 96).view(np.uint32), first.view(np.uint32))
        assert pt.getBvhInfo(state).device_bytes == grown
        pt.updateVertices(state, v0)                                # an update reuses the same index buffer
        assert pt.getBvhInfo(state).device_bytes == grown
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        # the other math mode: same inputs, same bits
        fq = pt.PathTraceParams()
        C.memmove(C.byref(fq), C.byref(state.params), C.sizeof(fq))
        fq.accumulationBuffer = dev_fast.put(acc)
        ff = (dev_fast.put(dev.get(f[0], 64, 96)), dev_fast.put(dev.get(f[1], 64, 96)))
        fpf = (dev_fast.put(dev.get(pf[0], 72, 80)), dev_fast.put(dev.get(pf[1], 72, 80)))
        fout = dev_fast.alloc(96 * 64 * 16)
        assert _motion(fast, fq, 8, ff, pq, dev_fast.put(hist), fpf, dev_fast.put(v0), dev_fast.put(v1), v0.shape[0], 256.0, g, fout) == 0
        assert np.array_equal(dev_fast.get(fout, 64, 96).view(np.uint32), first.view(np.uint32))
    finally:
        ob.free()
        dev.close()
        dev_fast.close()


def _history_run(s, motion):
    """TemporalHistory over: one frame, updateVertices (the sphere moved), one frame; returns (update, denoise) of the second view."""
    v0, v1 = _deformed(BOX_DIFFUSE, "sphere")
    hist = pt.TemporalHistory(motion=motion)
    try:
        s.params.currentFrameIdx = 0
        pt.LaunchCurrentFrame(None, s)
        s.params.currentFrameIdx = 1
        hist.update(s)
        pt.updateVertices(s, v1)
        s.refreshAccumulationBuffer = True
        pt.updateState(None, s)
        pt.LaunchCurrentFrame(None, s)
        s.params.currentFrameIdx = 1
        return hist.update(s), hist.denoise(s, 5)
    finally:
        hist.close()


def test_group_context_acts_on_rank0(gpu_state_factory, monkeypatch):
    kw = dict(width=96, height=64, spp=8, **KW)
    single, _ = gpu_state_factory(BOX_DIFFUSE, **kw)
    monkeypatch.setenv("ACGPT_REHEARSE_SAME_GPU", "1")
    group, _ = gpu_state_factory(BOX_DIFFUSE, device_ids=[0, 0], **kw)
    results = [_history_run(s, True) for s in (single, group)]
    for a, b in zip(*results):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (results[0][0][..., 3] > 8).mean() > 0.5


def test_refusals_leave_the_context_usable(gpu_state_factory):
    state, obj = gpu_state_factory(BOX_DIFFUSE, width=64, height=48, spp=8, **KW)
    dev = _Dev(state)
    L = _native.hip()
    try:
        m = _moved_views(state, dev, BOX_DIFFUSE, "sphere", (64, 48), (64, 48))
        q, pq, f, pf, hd, vd, vd0 = m["q"], m["pq"], m["f"], m["pf"], m["hist_d"], m["vd"], m["vd0"]
        nv = m["v0"].shape[0]
        out = dev.alloc(64 * 48 * 16)
        g = pt.TEMPORAL_CLIP_GAMMA
        assert _motion(state, q, 8, f, pq, hd, pf, vd, vd0, nv, 256.0, g, out) == 0
        expected = dev.get(out, 48, 64)
        noacc = pt.PathTraceParams()
        C.memmove(C.byref(noacc), C.byref(q), C.sizeof(q))
        noacc.accumulationBuffer = None
        B = L.pt_temporal_blend_motion
        ctx = state.context
        refused = [
            B(ctx, None, 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, g, out),                    # pt_temporal_blend's
            B(ctx, C.byref(noacc), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, g, out),
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), None, pf[0], pf[1], vd, vd0, nv, 256.0, g, out),
            B(ctx, C.byref(q), 0, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, g, out),
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, float("nan"), g, out),
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, g, f[0]),
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, None, nv, 256.0, g, out),            # one array only
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], None, vd0, nv, 256.0, g, out),
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv - 1, 256.0, g, out),         # n_verts
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv + 1, 256.0, g, out),
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, -1.0, out),          # gamma
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, float("inf"), out),
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, float("nan"), out),
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, g, vd),              # overlaps a vertex array
            B(ctx, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, g, vd0 + 16),
        ]
        assert all(rc != 0 for rc in refused), refused
        assert b"pt_temporal_blend_motion" in L.pt_last_error(state.context)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert B(bare, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], vd, vd0, nv, 256.0, g, out) != 0
            assert b"no scene" in L.pt_last_error(bare)
        finally:
            L.pt_destroy(bare)
        assert _motion(state, q, 8, f, pq, hd, pf, vd, vd0, nv, 256.0, g, out) == 0
        assert np.array_equal(dev.get(out, 48, 64).view(np.uint32), expected.view(np.uint32))
    finally:
        dev.close()


def test_temporal_history_keeps_the_history_across_updates(gpu_state_factory):
    kw = dict(width=96, height=64, spp=8, **KW)
    kept = _history_run(gpu_state_factory(BOX_DIFFUSE, **kw)[0], True)[0]
    dropped = _history_run(gpu_state_factory(BOX_DIFFUSE, **kw)[0], False)[0]
    assert (kept[..., 3] > 8).mean() > 0.5                  # motion=True: the history carried over the vertex update ...
    assert np.all(dropped[..., 3] == 8)                     # ... the default object still drops it
    # a new scene drops it with motion=True too
    state, obj = gpu_state_factory(BOX_DIFFUSE, **kw)
    hist = pt.TemporalHistory(motion=True)
    try:
        state.params.currentFrameIdx = 0
        pt.LaunchCurrentFrame(None, state)
        state.params.currentFrameIdx = 1
        hist.update(state)
        pt.buildTheAccelarationStructure(state, obj)
        tr.set_camera(state.params, *tr.orbit_camera(96, 64, 20, 0))
        state.refreshAccumulationBuffer = True
        pt.updateState(None, state)
        pt.LaunchCurrentFrame(None, state)
        state.params.currentFrameIdx = 1
        assert np.all(hist.update(state)[..., 3] == 8)
    finally:
        hist.close()


def _read_ppm(path):
    blob = open(path, "rb").read()
    parts = blob.split(b"\n", 3)
    assert parts[0] == b"P6"
    w, h = (int(x) for x in parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3).astype(np.float64) / 255.0


def test_cli_move_history(built, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    base = [exe, "--obj", BOX_DIFFUSE, "--width", "128", "--height", "128", "--max-depth", "8", "--direct-lighting", "--importance-sampling",
            "--move", "glass:%g,%g,%g" % mr.SPHERE_MOVE]

    def run(name, extra, code=0):
        r = subprocess.run(base + ["--out", str(tmp_path / (name + ".ppm"))] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == code, r.stdout + r.stderr
        return r

    run("a", ["--spp-per-launch", "8", "--frames", "2", "--move-history", "--denoise", "5"])
    run("b", ["--spp-per-launch", "8", "--frames", "2"])
    run("c", ["--spp-per-launch", "8", "--frames", "1", "--move-history"])
    run("truth", ["--spp-per-launch", "256", "--frames", "16"])
    # the flag adds files and changes none
    for n in ("", "_moved"):
        assert (tmp_path / ("a%s.ppm" % n)).read_bytes() == (tmp_path / ("b%s.ppm" % n)).read_bytes()
    assert (tmp_path / "a_moved_temporal.ppm").exists() and (tmp_path / "a_moved_temporal_denoised.ppm").exists()
    assert not (tmp_path / "b_moved_temporal.ppm").exists() and not (tmp_path / "c_moved_temporal_denoised.ppm").exists()
    truth = _read_ppm(str(tmp_path / "truth_moved.ppm"))
    for name in ("a", "c"):
        moved, carried = (_read_ppm(str(tmp_path / ("%s%s.ppm" % (name, n)))) for n in ("_moved", "_moved_temporal"))
        mse_moved, mse_carried = float(np.mean((moved - truth) ** 2)), float(np.mean((carried - truth) ** 2))
        print("CLI %s: MSE _moved %.3e, _moved_temporal %.3e" % (name, mse_moved, mse_carried))
        assert mse_carried < mse_moved
    r = subprocess.run([exe, "--obj", BOX_DIFFUSE, "--out", str(tmp_path / "d.ppm"), "--move-history"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--move" in r.stderr
