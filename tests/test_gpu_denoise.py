"""The denoised preview on the GPU: pt_render_features against the ray queries, pt_denoise against tests/denoise_ref.py, how much it
denoises (thresholds from the CPU calibration in tests/test_denoise_host.py), the state it must leave alone, the group context,
the refusals and acgpt_main --denoise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import denoise_ref as dr
from scene_utils import image_mse
from test_denoise_host import EDGE_MEASURED, F_MEASURED

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")


def _camera(state):
    p = state.params
    return p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple()


def _trace_closest(state, rays):
    n = rays.shape[0]
    t = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32)
    assert _native.hip().pt_trace_closest(state.context, rays.ctypes.data, n, t.ctypes.data, prim.ctypes.data) == 0
    return t, prim


def _launch(state, frame=0, sub_frames=1, output_buffer=None):
    state.params.currentFrameIdx = frame
    pt.LaunchCurrentFrame(output_buffer, state, sub_frames)


def _diffuse(obj):
    return np.array([[m.diffuse.x, m.diffuse.y, m.diffuse.z] for m in obj.getMaterials()], np.float32)


def _check_features(state, obj, alb, nd):
    w, h = int(state.params.width), int(state.params.height)
    rays = dr.pixel_rays(w, h, *_camera(state))
    t, prim = _trace_closest(state, rays)
    assert np.array_equal(alb[..., 3].reshape(-1).view(np.uint32), prim)
    assert np.array_equal(nd[..., 3].reshape(-1).view(np.uint32), t.view(np.uint32))
    ref_alb, ref_nd = dr.features_from_hits(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), _diffuse(obj))
    assert np.abs(nd.reshape(-1, 4)[:, :3] - ref_nd[:, :3]).max() <= 1e-5
    assert np.array_equal(alb.reshape(-1, 4)[:, :3], ref_alb[:, :3])
    assert 0.5 < (prim != 0xFFFFFFFF).mean() < 1.0


@pytest.mark.parametrize("scene", [BOX, BOX_DIFFUSE])
@pytest.mark.parametrize("size", [(256, 192), (97, 61)])
def test_features_equal_the_queries(gpu_state_factory, scene, size):
    state, obj = gpu_state_factory(scene, width=size[0], height=size[1], max_depth=4, spp=8)
    before = pt.getBvhInfo(state).device_bytes
    alb, nd = pt.renderFeatures(state)
    assert pt.getBvhInfo(state).device_bytes == before         # the scene keeps its one node array
    _check_features(state, obj, alb, nd)


def test_features_on_an_fp32_node_scene(gpu_state_factory):
    """A scene set up under an fp32-node variant keeps the fp32 nodes only: the features walk them (traverse<false>), same bits."""
    base, obj = gpu_state_factory(BOX, width=97, height=61, max_depth=4, spp=8)
    alb0, nd0 = pt.renderFeatures(base)
    state = pt.PathTracerState()
    C.memmove(C.byref(state.params), C.byref(base.params), C.sizeof(state.params))
    state.params.accumulationBuffer = None
    pt.createDeviceContext(state)
    try:
        assert _native.hip().pt_set_tuning(state.context, 0, 1) == 0            # variant 1: fp32 nodes
        pt.buildTheAccelarationStructure(state, obj)
        before = pt.getBvhInfo(state).device_bytes
        alb, nd = pt.renderFeatures(state)
        assert pt.getBvhInfo(state).device_bytes == before
        assert np.array_equal(alb.view(np.uint32), alb0.view(np.uint32)) and np.array_equal(nd.view(np.uint32), nd0.view(np.uint32))
        _check_features(state, obj, alb, nd)
    finally:
        pt.CleanAllTheThings(state)


@pytest.mark.parametrize("size", [(96, 64), (97, 61)])
def test_filter_equals_the_numpy_reference(gpu_state_factory, size):
    state, _ = gpu_state_factory(BOX, width=size[0], height=size[1], max_depth=8, direct_lighting=True, importance_sampling=True, spp=8)
    _launch(state)
    acc = pt.readAccumulation(state)
    alb, nd = pt.renderFeatures(state)
    fast, _ = gpu_state_factory(BOX, math_mode="fast", width=size[0], height=size[1], max_depth=8, direct_lighting=True, importance_sampling=True, spp=8)
    assert _native.hip().pt_copy_to_device(fast.context, fast.params.accumulationBuffer, acc.ctypes.data, acc.nbytes) == 0
    for it in (1, 3, 5):
        got = pt.denoise(state, it)
        ref = dr.denoise(acc, alb, nd, it)
        bad = ~(np.abs(got - ref) <= np.maximum(1e-4 * np.abs(ref), 1e-5))
        assert not bad.any(), "iterations %d: %d channels off, worst %s vs %s" % (it, bad.sum(), got[bad][:4], ref[bad][:4])
        assert np.array_equal(pt.denoise(state, it).view(np.uint32), got.view(np.uint32))           # deterministic
        assert np.array_equal(pt.denoise(fast, it).view(np.uint32), got.view(np.uint32))            # math mode does not matter


def test_denoises_and_keeps_edges(gpu_state_factory):
    state, _ = gpu_state_factory(BOX, width=256, height=256, max_depth=8, direct_lighting=True, importance_sampling=True, spp=8)
    _launch(state)
    noisy = pt.readAccumulation(state)
    denoised = pt.denoise(state, 5)
    state.params.samplesPerPixel = 256
    _launch(state, 0, 32)                               # 8192 samples per pixel
    ref = pt.readAccumulation(state)
    mse_noisy, mse_dn = image_mse(noisy, ref), image_mse(denoised, ref)
    mse_edge = image_mse(pt.denoise(state, 5), ref)
    print("MSE noisy %.3e denoised %.3e (F %.2f) denoise(ref) %.3e (%.3f of noisy)" % (mse_noisy, mse_dn, mse_noisy / mse_dn, mse_edge, mse_edge / mse_noisy))
    assert mse_dn <= mse_noisy / (F_MEASURED / 2)
    assert mse_edge <= 2.5 * EDGE_MEASURED * mse_noisy


def test_leaves_the_render_state_alone(gpu_state_factory):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, _ = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        _launch(state, 0, output_buffer=ob)
        _launch(twin, 0)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        pt.renderFeatures(state)
        pt.denoise(state, 5)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        _launch(state, 1, output_buffer=ob)
        _launch(twin, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_group_context_acts_on_rank0(gpu_state_factory, monkeypatch):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    single, _ = gpu_state_factory(BOX, **kw)
    monkeypatch.setenv("ACGPT_REHEARSE_SAME_GPU", "1")
    group, _ = gpu_state_factory(BOX, device_ids=[0, 0], **kw)
    for s in (single, group):
        _launch(s)
    assert np.array_equal(pt.readAccumulation(group).view(np.uint32), pt.readAccumulation(single).view(np.uint32))
    for a, b in zip(pt.renderFeatures(group), pt.renderFeatures(single)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(pt.denoise(group, 5).view(np.uint32), pt.denoise(single, 5).view(np.uint32))


def test_refusals_leave_the_context_usable(gpu_state_factory):
    state, _ = gpu_state_factory(BOX, width=64, height=48, max_depth=4, spp=8)
    _launch(state)
    expected = pt.denoise(state, 5)
    L = _native.hip()
    n = 64 * 48 * 16
    bufs = [C.c_void_p() for _ in range(3)]
    for b in bufs:
        assert L.pt_device_malloc(state.context, C.byref(b), n) == 0
    alb, nd, out = (b.value for b in bufs)
    try:
        assert L.pt_render_features(state.context, C.byref(state.params), alb, nd) == 0
        p = state.params
        refused = [
            L.pt_render_features(state.context, None, alb, nd),
            L.pt_render_features(state.context, C.byref(p), None, nd),
            L.pt_render_features(state.context, C.byref(p), alb, None),
            L.pt_denoise(state.context, None, alb, nd, out, 5),
            L.pt_denoise(state.context, C.byref(p), None, nd, out, 5),
            L.pt_denoise(state.context, C.byref(p), alb, None, out, 5),
            L.pt_denoise(state.context, C.byref(p), alb, nd, None, 5),
            L.pt_denoise(state.context, C.byref(p), alb, nd, out, 0),
            L.pt_denoise(state.context, C.byref(p), alb, nd, out, 9),
            L.pt_denoise(state.context, C.byref(p), alb, nd, p.accumulationBuffer, 5),
            L.pt_denoise(state.context, C.byref(p), alb, nd, nd, 5),
        ]
        assert all(rc != 0 for rc in refused), refused
        assert L.pt_last_error(state.context)
        empty = pt.PathTraceParams()
        C.memmove(C.byref(empty), C.byref(p), C.sizeof(p))
        empty.width = 0
        assert L.pt_render_features(state.context, C.byref(empty), alb, nd) != 0
        assert L.pt_denoise(state.context, C.byref(empty), alb, nd, out, 5) != 0
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_render_features(bare, C.byref(p), alb, nd) != 0
            assert b"no scene" in L.pt_last_error(bare)
        finally:
            L.pt_destroy(bare)
    finally:
        for b in (alb, nd, out):
            L.pt_device_free(state.context, b)
    assert np.array_equal(pt.denoise(state, 5).view(np.uint32), expected.view(np.uint32))


def test_cli_writes_a_denoised_image_beside_the_frame(built, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    runs = {}
    for name, extra in (("plain", []), ("denoised", ["--denoise", "5"])):
        d = tmp_path / name
        d.mkdir()
        cmd = [exe, "--obj", BOX, "--width", "128", "--height", "96", "--spp-per-launch", "8", "--frames", "2", "--max-depth", "6",
               "--direct-lighting", "--importance-sampling", "--out", str(d / "f.png")] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = d
    assert (runs["plain"] / "f.png").read_bytes() == (runs["denoised"] / "f.png").read_bytes()
    assert not (runs["plain"] / "f_denoised.png").exists()
    den = (runs["denoised"] / "f_denoised.png").read_bytes()
    assert den[:8] == b"\x89PNG\r\n\x1a\n" and den != (runs["denoised"] / "f.png").read_bytes()
