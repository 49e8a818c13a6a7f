"""Temporal reprojection on the GPU: pt_temporal_blend against tests/temporal_ref.py on GPU-made features and accumulations, how much
it gains (thresholds from the CPU calibration in tests/test_temporal_host.py), the state it must leave alone, the group context,
the refusals, pathtracer.TemporalHistory and acgpt_main --history-out / --history-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import temporal_ref as tr
from scene_utils import image_mse
from test_temporal_host import F_BLEND

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
KW = dict(max_depth=8, direct_lighting=True, importance_sampling=True)


class _Dev:
    """Device buffers of one context, freed on close."""

    def __init__(self, state):
        self.state, self.ptrs = state, []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert _native.hip().pt_device_malloc(self.state.context, C.byref(p), nbytes) == 0
        self.ptrs.append(p.value)
        return p.value

    def put(self, a):
        a = np.ascontiguousarray(a, np.float32)
        p = self.alloc(a.nbytes)
        assert _native.hip().pt_copy_to_device(self.state.context, p, a.ctypes.data, a.nbytes) == 0
        return p

    def get(self, p, h, w):
        out = np.zeros((h, w, 4), np.float32)
        assert _native.hip().pt_copy_to_host(self.state.context, out.ctypes.data, p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.ptrs:
            _native.hip().pt_device_free(self.state.context, p)
        self.ptrs = []


def _view(state, dev, w, h, orbit, spp, frames=1):
    """Render `frames` launches of `spp` at the camera of --orbit `orbit` into a buffer of its own (the state's accumulation is not
    touched); returns (params of the view, accumulation [h, w, 4] on the host, its device pointer, features on the device)."""
    L = _native.hip()
    q = pt.PathTraceParams()
    C.memmove(C.byref(q), C.byref(state.params), C.sizeof(q))
    q.width, q.height, q.samplesPerPixel = w, h, spp
    tr.set_camera(q, *tr.orbit_camera(w, h, *orbit))
    q.frameBuffer = None
    q.accumulationBuffer = dev.alloc(w * h * 16)
    q.currentFrameIdx = 0
    assert L.pt_launch_frames(state.context, C.byref(q), frames) == 0, L.pt_last_error(state.context)
    alb, nd = dev.alloc(w * h * 16), dev.alloc(w * h * 16)
    assert L.pt_render_features(state.context, C.byref(q), alb, nd) == 0
    return q, dev.get(q.accumulationBuffer, h, w), q.accumulationBuffer, (alb, nd)


def _blend(state, q, n, feats, prev, prev_hist, prev_feats, cap, out):
    return _native.hip().pt_temporal_blend(state.context, C.byref(q), n, feats[0], feats[1], C.byref(prev) if prev is not None else None,
                                           prev_hist, prev_feats[0] if prev_feats else None, prev_feats[1] if prev_feats else None, cap, out)


@pytest.mark.parametrize("scene", [BOX, BOX_DIFFUSE])
@pytest.mark.parametrize("size,prev_size", [((256, 192), (256, 192)), ((256, 192), (200, 240)), ((97, 61), (97, 61)), ((97, 61), (128, 80))])
def test_blend_equals_the_numpy_reference(gpu_state_factory, scene, size, prev_size):
    (w, h), (wp, hp) = size, prev_size
    state, obj = gpu_state_factory(scene, width=w, height=h, spp=8, **KW)
    dev = _Dev(state)
    try:
        pq, hist, _, pf = _view(state, dev, wp, hp, (0, 0), 32)
        hist[..., 3] = 32.0
        hist_d = dev.put(hist)
        q, acc, _, f = _view(state, dev, w, h, (20, 0), 8)
        out_d = dev.alloc(w * h * 16)
        prev_feat = [dev.get(p, hp, wp) for p in pf]
        feat = [dev.get(p, h, w) for p in f]
        for cap in (256.0, 12.0):
            assert _blend(state, q, 8, f, pq, hist_d, pf, cap, out_d) == 0, _native.hip().pt_last_error(state.context)
            got = dev.get(out_d, h, w)
            ref, took = tr.blend(acc, feat[0], feat[1], tr.camera_of(q), 8, tr.tri_bsdf(obj), cap, (tr.camera_of(pq), hist, *prev_feat))
            assert np.array_equal(got[..., 3].view(np.uint32), ref[..., 3].view(np.uint32))
            assert np.array_equal(got[..., 3] != 8.0, took)
            bad = ~(np.abs(got[..., :3] - ref[..., :3]) <= 1e-6 * np.abs(ref[..., :3]))
            assert not bad.any(), "%d channels off, worst %s vs %s" % (bad.sum(), got[..., :3][bad][:4], ref[..., :3][bad][:4])
            print("%s %s <- %s cap %g: %.3f take history, %.4f of the channels bit-identical" % (os.path.basename(scene), size, prev_size, cap,
                  took.mean(), (got.view(np.uint32) == ref.view(np.uint32)).mean()))
            assert took.mean() > 0.4
        # no history: the pass-through, exactly
        assert _blend(state, q, 8, f, None, None, None, 256.0, out_d) == 0
        got = dev.get(out_d, h, w)
        assert np.array_equal(got[..., :3].view(np.uint32), acc[..., :3].view(np.uint32)) and np.all(got[..., 3] == 8.0)
    finally:
        dev.close()


def test_gains_what_the_cpu_calibration_says(gpu_state_factory):
    state, obj = gpu_state_factory(BOX, width=256, height=256, spp=8, **KW)
    dev = _Dev(state)
    try:
        pq, hist, _, pf = _view(state, dev, 256, 256, (0, 0), 256, frames=4)          # 1024 spp at the reference camera
        hist[..., 3] = 1024.0
        hist_d = dev.put(hist)
        q, noisy, noisy_d, f = _view(state, dev, 256, 256, (20, 0), 8)             # one 8-spp launch, orbited
        _, truth, _, _ = _view(state, dev, 256, 256, (20, 0), 256, frames=32)      # 8192 spp, orbited
        out_d = dev.alloc(256 * 256 * 16)
        assert _blend(state, q, 8, f, pq, hist_d, pf, pt.TEMPORAL_HISTORY_CAP, out_d) == 0
        blended = dev.get(out_d, 256, 256)
        dn_d = dev.alloc(256 * 256 * 16)
        L = _native.hip()

        def denoise(src):
            d = pt.PathTraceParams()
            C.memmove(C.byref(d), C.byref(q), C.sizeof(d))
            d.accumulationBuffer = src
            assert L.pt_denoise(state.context, C.byref(d), f[0], f[1], dn_d, 5) == 0
            return dev.get(dn_d, 256, 256)

        mse_noisy, mse_blend = image_mse(noisy, truth), image_mse(blended, truth)
        mse_dn_blend, mse_dn_noisy = image_mse(denoise(out_d), truth), image_mse(denoise(noisy_d), truth)
        print("MSE 8 spp %.3e blend %.3e (F %.2f) denoise(blend) %.3e (%.2f) denoise(8 spp) %.3e (%.2f); %.3f take history"
              % (mse_noisy, mse_blend, mse_noisy / mse_blend, mse_dn_blend, mse_noisy / mse_dn_blend, mse_dn_noisy, mse_noisy / mse_dn_noisy,
                 (blended[..., 3] != 8.0).mean()))
        assert mse_noisy / mse_blend >= 0.9 * F_BLEND
        assert mse_dn_blend < mse_dn_noisy
    finally:
        dev.close()


def test_leaves_the_render_state_alone_and_repeats(gpu_state_factory):
    kw = dict(width=96, height=64, spp=8, **KW)
    state, obj = gpu_state_factory(BOX, **kw)
    fast, _ = gpu_state_factory(BOX, math_mode="fast", **kw)
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    dev, dev_fast = _Dev(state), _Dev(fast)
    L = _native.hip()
    try:
        pq, hist, _, pf = _view(state, dev, 80, 72, (0, 0), 16)
        hist[..., 3] = 16.0
        hist_d = dev.put(hist)
        state.params.currentFrameIdx = 0
        pt.LaunchCurrentFrame(ob, state)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        before = pt.getBvhInfo(state).device_bytes
        f = (dev.alloc(96 * 64 * 16), dev.alloc(96 * 64 * 16))
        assert L.pt_render_features(state.context, C.byref(state.params), f[0], f[1]) == 0
        out_d = dev.alloc(96 * 64 * 16)
        assert _blend(state, state.params, 8, f, pq, hist_d, pf, 256.0, out_d) == 0
        first = dev.get(out_d, 64, 96)
        grown = pt.getBvhInfo(state).device_bytes
        assert grown == before + obj.getIndexBuffer().size // 3          # one byte per triangle, once
        for _ in range(2):
            assert _blend(state, state.params, 8, f, pq, hist_d, pf, 256.0, out_d) == 0
            assert np.array_equal(dev.get(out_d, 64, 96).view(np.uint32), first.view(np.uint32))
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
        assert _blend(fast, fq, 8, ff, pq, dev_fast.put(hist), fpf, 256.0, fout) == 0
        assert np.array_equal(dev_fast.get(fout, 64, 96).view(np.uint32), first.view(np.uint32))
        # a new scene frees the array; the next blend builds it again
        pt.buildTheAccelarationStructure(state, obj)
        rebuilt = pt.getBvhInfo(state).device_bytes
        assert _blend(state, state.params, 8, f, pq, hist_d, pf, 256.0, out_d) == 0
        assert pt.getBvhInfo(state).device_bytes == rebuilt + obj.getIndexBuffer().size // 3
        assert np.array_equal(dev.get(out_d, 64, 96).view(np.uint32), first.view(np.uint32))
    finally:
        ob.free()
        dev.close()
        dev_fast.close()


def test_group_context_acts_on_rank0(gpu_state_factory, monkeypatch):
    kw = dict(width=96, height=64, spp=8, **KW)
    single, _ = gpu_state_factory(BOX, **kw)
    monkeypatch.setenv("ACGPT_REHEARSE_SAME_GPU", "1")
    group, _ = gpu_state_factory(BOX, device_ids=[0, 0], **kw)
    results = []
    for s in (single, group):
        hist = pt.TemporalHistory()
        try:
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(None, s)
            s.params.currentFrameIdx = 1
            hist.update(s)
            tr.set_camera(s.params, *tr.orbit_camera(96, 64, 20, 0))
            s.refreshAccumulationBuffer = True
            pt.updateState(None, s)
            pt.LaunchCurrentFrame(None, s)
            s.params.currentFrameIdx = 1
            results.append((hist.update(s), hist.denoise(s, 5)))
        finally:
            hist.close()
    for a, b in zip(*results):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (results[0][0][..., 3] > 8).mean() > 0.5


def test_refusals_leave_the_context_usable(gpu_state_factory):
    state, _ = gpu_state_factory(BOX, width=64, height=48, spp=8, **KW)
    dev = _Dev(state)
    L = _native.hip()
    try:
        pq, hist, _, pf = _view(state, dev, 64, 48, (0, 0), 8)
        hist[..., 3] = 8.0
        hd = dev.put(hist)
        q, _, _, f = _view(state, dev, 64, 48, (20, 0), 8)
        out = dev.alloc(64 * 48 * 16)
        assert _blend(state, q, 8, f, pq, hd, pf, 256.0, out) == 0
        expected = dev.get(out, 48, 64)
        empty = pt.PathTraceParams()
        C.memmove(C.byref(empty), C.byref(q), C.sizeof(q))
        empty.width = 0
        big = pt.PathTraceParams()
        C.memmove(C.byref(big), C.byref(pq), C.sizeof(pq))
        big.width = 70000
        noacc = pt.PathTraceParams()
        C.memmove(C.byref(noacc), C.byref(q), C.sizeof(q))
        noacc.accumulationBuffer = None
        refused = [
            L.pt_temporal_blend(state.context, None, 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, out),
            L.pt_temporal_blend(state.context, C.byref(noacc), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, out),
            L.pt_temporal_blend(state.context, C.byref(q), 8, None, f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, out),
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], None, C.byref(pq), hd, pf[0], pf[1], 256.0, out),
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, None),
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), None, pf[0], pf[1], 256.0, out),      # a partial set
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], None, hd, pf[0], pf[1], 256.0, out),
            L.pt_temporal_blend(state.context, C.byref(q), 0, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, out),         # N = 0
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], -1.0, out),          # caps
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], float("inf"), out),
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], float("nan"), out),
            L.pt_temporal_blend(state.context, C.byref(empty), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, out),     # sizes
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(big), hd, pf[0], pf[1], 256.0, out),
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, q.accumulationBuffer),   # overlaps
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, f[1]),
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, hd),
            L.pt_temporal_blend(state.context, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, pf[0] + 16),
        ]
        assert all(rc != 0 for rc in refused), refused
        assert b"pt_temporal_blend" in L.pt_last_error(state.context)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_temporal_blend(bare, C.byref(q), 8, f[0], f[1], C.byref(pq), hd, pf[0], pf[1], 256.0, out) != 0
            assert b"no scene" in L.pt_last_error(bare)
        finally:
            L.pt_destroy(bare)
        assert _blend(state, q, 8, f, pq, hd, pf, 256.0, out) == 0
        assert np.array_equal(dev.get(out, 48, 64).view(np.uint32), expected.view(np.uint32))
    finally:
        dev.close()


def test_temporal_history_object(gpu_state_factory):
    state, _ = gpu_state_factory(BOX, width=96, height=64, spp=16, **KW)
    hist = pt.TemporalHistory()

    def frames(n):
        for _ in range(n):
            pt.LaunchCurrentFrame(None, state)
            state.params.currentFrameIdx += 1

    state.params.currentFrameIdx = 0
    frames(4)
    first = hist.update(state)                                   # nothing to reproject yet: the accumulation, N = 64
    assert np.all(first[..., 3] == 64.0)
    assert np.array_equal(first[..., :3], pt.readAccumulation(state)[..., :3])
    tr.set_camera(state.params, *tr.orbit_camera(96, 64, 20, 0))
    state.refreshAccumulationBuffer = True
    pt.updateState(None, state)
    frames(1)
    moved = hist.update(state)
    took = moved[..., 3] > 16.0
    assert took.mean() > 0.5 and np.all(moved[took, 3] <= 16.0 + 64.0)
    frames(1)
    again = hist.update(state)                                  # same camera: the same source, the newer accumulation
    assert np.all(again[took, 3] <= 32.0 + 64.0) and np.all(again[~took, 3] == 32.0)
    assert np.allclose(again[took, 3] - 32.0, moved[took, 3] - 16.0, rtol=1e-5, atol=1e-5)
    dn = hist.denoise(state, 5)
    assert dn.shape == (64, 96, 4) and np.all(dn[..., 3] == 1.0)
    pt.keyCallback(state, "UP")                                 # another maxDepth: the history goes
    pt.updateState(None, state)
    frames(1)
    dropped = hist.update(state)
    assert np.all(dropped[..., 3] == 16.0)
    hist.close()
    assert hist not in state._temporal
    hist2 = pt.TemporalHistory()
    hist2.update(state)
    assert state._temporal == [hist2]                           # CleanAllTheThings (the fixture's teardown) closes it


def _read_history(path):
    blob = open(path, "rb").read()
    assert blob[:8] == b"ACGPTHST"
    hdr = np.frombuffer(blob[8:40], np.uint32)
    w, h = int(hdr[0]), int(hdr[1])
    data = np.frombuffer(blob[88:], np.float32)
    assert data.size == w * h * 4
    return hdr, np.frombuffer(blob[40:88], np.float32), data.reshape(h, w, 4)


def test_cli_carries_the_history_across_an_orbit(built, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    base = [exe, "--obj", BOX, "--width", "128", "--height", "128", "--max-depth", "8", "--direct-lighting", "--importance-sampling"]

    def run(name, extra, ok=True):
        r = subprocess.run(base + ["--out", str(tmp_path / (name + ".png"))] + extra, capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stdout + r.stderr
        return r

    a = str(tmp_path / "a.hist")
    run("a", ["--spp-per-launch", "64", "--frames", "4", "--history-out", a])
    hdr, cam, hist_a = _read_history(a)
    n_tris = pt.TinyObjWrapper(BOX).getIndexBuffer().size // 3
    assert list(hdr) == [128, 128, 8, 1, 1, 0, _native.MATH_FAST, n_tris] and np.all(hist_a[..., 3] == 256.0)
    orbit = ["--orbit", "20,0", "--spp-per-launch", "8", "--frames", "1"]
    run("b", orbit + ["--history-in", a, "--denoise", "5", "--history-out", str(tmp_path / "b.hist")])
    run("c", orbit + ["--history-out", str(tmp_path / "c.hist")])
    run("truth", ["--orbit", "20,0", "--spp-per-launch", "256", "--frames", "16", "--history-out", str(tmp_path / "t.hist")])
    assert (tmp_path / "b.png").read_bytes() == (tmp_path / "c.png").read_bytes()          # the frame itself is the same
    for name in ("b_temporal.png", "b_temporal_denoised.png"):
        assert (tmp_path / name).read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    assert not (tmp_path / "c_temporal.png").exists()
    _, cam_b, blended = _read_history(str(tmp_path / "b.hist"))
    _, _, plain = _read_history(str(tmp_path / "c.hist"))
    _, _, truth = _read_history(str(tmp_path / "t.hist"))
    assert not np.array_equal(cam_b, cam)
    mse_plain, mse_blend = image_mse(plain, truth), image_mse(blended, truth)
    print("CLI: MSE 8 spp %.3e, _temporal %.3e" % (mse_plain, mse_blend))
    assert mse_blend < mse_plain / 2
    r = run("d", orbit + ["--max-depth", "6", "--history-in", a], ok=False)
    assert "maxDepth" in r.stdout + r.stderr and not (tmp_path / "d_temporal.png").exists()
