"""pt_denoise, pt_temporal_blend and pt_temporal_blend_motion on inputs no render produces (tests/image_cases.py): every valid case
against the fp32 mirror at the bars of test_gpu_denoise.py / test_gpu_temporal.py, against the float64 evaluation and the closed-form
plane answers; every hostile kind at every position against the mirror under the rules of include/acgpt.h, with the three properties
asserted on the device output itself; a poisoned history through two chained blends.  Nothing renders: every buffer is uploaded.

Every call is made twice in PT_MATH_IEEE and once in PT_MATH_FAST and must give the same bits; every output has 64 bytes of 0xCD
behind it, checked after each call."""
import ctypes as C
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import denoise_ref as dr
import image_cases as ic
from test_gpu_temporal import _Dev
from test_image_cases_host import F64_BOUND, check_closed_form

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
MAX_PIXELS = 64 * 64
GUARD = 64


class _Stages:
    """One context and one set of device buffers, each large enough for 64 x 64, for every case of this module."""

    def __init__(self, state):
        self.state, self.dev, self.L = state, _Dev(state), _native.hip()
        self.buf = {k: self.dev.alloc(MAX_PIXELS * 16 + GUARD) for k in ("accum", "albedo", "nd", "hist", "prev_albedo", "prev_nd", "out", "out2")}
        n_verts = ic.scene()["verts"].shape[0]
        self.verts = [self.dev.alloc(n_verts * 16), self.dev.alloc(n_verts * 16)]
        self.calls = 0

    def put(self, name, a):
        a = np.ascontiguousarray(a, np.float32)
        assert a.nbytes <= MAX_PIXELS * 16
        assert self.L.pt_copy_to_device(self.state.context, self.buf[name], a.ctypes.data, a.nbytes) == 0

    def params(self, w, h, camera=None):
        q = pt.PathTraceParams()
        C.memmove(C.byref(q), C.byref(self.state.params), C.sizeof(q))
        q.width, q.height = w, h
        q.frameBuffer = None
        q.accumulationBuffer = self.buf["accum"]
        if camera is not None:
            f = lambda v: pt.Float3(float(v[0]), float(v[1]), float(v[2]))
            q.cameraEye, q.cameraU, q.cameraV, q.cameraW = (f(v) for v in camera)
        return q

    def _thrice(self, call, w, h, out="out"):
        """call() twice in PT_MATH_IEEE and once in PT_MATH_FAST: the same bits, and the guard behind the output intact each time."""
        ctx, n = self.state.context, w * h
        res = []
        for mode in (_native.MATH_IEEE, _native.MATH_IEEE, _native.MATH_FAST):
            assert self.L.pt_set_math_mode(ctx, mode) == 0
            assert self.L.pt_device_memset(ctx, self.buf[out], 0xCD, n * 16 + GUARD) == 0
            assert call() == 0, self.L.pt_last_error(ctx)
            raw = np.zeros(n * 4 + GUARD // 4, np.uint32)
            assert self.L.pt_copy_to_host(ctx, raw.ctypes.data, self.buf[out], raw.nbytes) == 0
            assert (raw[n * 4:] == 0xCDCDCDCD).all(), "written past pixel %d" % n
            res.append(raw[:n * 4].copy())
            self.calls += 1
        assert self.L.pt_set_math_mode(ctx, _native.MATH_IEEE) == 0
        assert np.array_equal(res[0], res[1]), "two calls differ"
        assert np.array_equal(res[0], res[2]), "the math modes differ"
        return res[0].view(np.float32).reshape(h, w, 4)

    def denoise(self, accum, albedo, nd, iterations):
        h, w = accum.shape[:2]
        for name, a in (("accum", accum), ("albedo", albedo), ("nd", nd)):
            self.put(name, a)
        q = self.params(w, h)
        return self._thrice(lambda: self.L.pt_denoise(self.state.context, C.byref(q), self.buf["albedo"], self.buf["nd"], self.buf["out"], iterations), w, h)

    def upload_blend(self, case):
        for name in ("accum", "albedo", "nd", "hist", "prev_albedo", "prev_nd"):
            self.put(name, case[name])
        if case["verts"] is not None:
            for p, v in zip(self.verts, (case["verts"], case["prev_verts"])):
                assert self.L.pt_copy_to_device(self.state.context, p, v.ctypes.data, v.nbytes) == 0

    def blend(self, case, cap, form, gamma, hist="hist", out="out"):
        """The uploaded case through pt_temporal_blend (form "static") or pt_temporal_blend_motion."""
        b, ctx = self.buf, self.state.context
        q, pq = self.params(case["w"], case["h"], case["camera"]), self.params(case["wp"], case["hp"], case["prev_camera"])
        if form == "static":
            call = lambda: self.L.pt_temporal_blend(ctx, C.byref(q), case["N"], b["albedo"], b["nd"], C.byref(pq), b[hist], b["prev_albedo"],
                                                    b["prev_nd"], cap, b[out])
        else:
            v = self.verts if case["verts"] is not None else (None, None)
            call = lambda: self.L.pt_temporal_blend_motion(ctx, C.byref(q), case["N"], b["albedo"], b["nd"], C.byref(pq), b[hist], b["prev_albedo"],
                                                           b["prev_nd"], v[0], v[1], ic.scene()["verts"].shape[0], cap, gamma, b[out])
        return self._thrice(call, case["w"], case["h"], out)

    def close(self):
        self.dev.close()


@pytest.fixture(scope="module")
def stages(gpu_state_factory):
    state, _ = gpu_state_factory(BOX, width=64, height=64, spp=1)
    s = _Stages(state)
    yield s
    s.close()


def _denoise_bar(got, ref, what):
    bad = ~(np.abs(got - ref) <= np.maximum(1e-4 * np.abs(ref), 1e-5))
    assert not bad.any(), "%s: %d channels off, worst %s vs %s" % (what, bad.sum(), got[bad][:4], ref[bad][:4])


def _blend_bar(got, ref, took, n, what):
    assert np.array_equal(got[..., 3].view(np.uint32), ref[..., 3].view(np.uint32)), what
    assert np.array_equal(got[..., 3] != n, took), what
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got[..., :3] - ref[..., :3]) <= 1e-6 * np.abs(ref[..., :3]))
    bad &= got[..., :3].view(np.uint32) != ref[..., :3].view(np.uint32)         # a non-finite pass-through is equal as bits
    assert not bad.any(), "%s: %d channels off, worst %s vs %s" % (what, bad.sum(), got[..., :3][bad][:4], ref[..., :3][bad][:4])


# ---- valid cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,w,h", ic.denoise_cases())
def test_denoiser_on_valid_cases(stages, kind, w, h):
    c = ic.denoise_case(kind, w, h)
    r32, r64 = ic.denoise_reference(kind, w, h), ic.denoise_reference(kind, w, h, np.float64)
    for it in ic.ITERATIONS:
        got = stages.denoise(c["accum"], c["albedo"], c["nd"], it)
        what = "%s %dx%d, %d iterations" % (kind, w, h, it)
        err = np.abs(got - r32[it])
        print("%s: worst |gpu - mirror| / max(1e-4 |ref|, 1e-5) = %.3f, %.4f bit-identical" % (
            what, (err / np.maximum(1e-4 * np.abs(r32[it]), 1e-5)).max(), (got.view(np.uint32) == r32[it].view(np.uint32)).mean()))
        _denoise_bar(got, r32[it], what)
        bound = np.maximum(F64_BOUND["denoise"] * np.abs(r64[it]), 1e-5) + np.maximum(1e-4 * np.abs(r64[it]), 1e-5)
        assert np.all(np.abs(got - r64[it]) <= bound), what + " against float64"


@pytest.mark.parametrize("kind", ic.BLEND_KINDS + ic.MOTION_KINDS)
def test_blends_on_valid_cases(stages, kind):
    case = ic.blend_case(kind)
    stages.upload_blend(case)
    for cap in ic.CAPS:
        for form, gamma in ic.blend_forms(kind):
            what = "%s cap %g %s gamma %g" % (kind, cap, form, gamma)
            got = stages.blend(case, cap, form, gamma)
            ref, took = ic.blend_reference(kind, cap, form, gamma)
            print("%s: %.2f take history, %.4f bit-identical" % (what, took.mean(), (got.view(np.uint32) == ref.view(np.uint32)).mean()))
            _blend_bar(got, ref, took, case["N"], what)
            r64, _ = ic.blend_reference(kind, cap, form, gamma, np.float64)
            assert np.all(np.abs(got - r64) <= (F64_BOUND[form] + 1e-6) * np.abs(r64)), what + " against float64"
            if case["shift"] is not None and gamma == 0.0:
                check_closed_form(got, case, cap, what + " against the closed form")
            if kind in ic.PASS_THROUGH or cap == 0.0:
                assert np.array_equal(got[..., :3].view(np.uint32), case["accum"][..., :3].view(np.uint32)) and np.all(got[..., 3] == case["N"]), what


# ---- hostile pixels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ic.DENOISE_HOSTILE_KINDS)
def test_denoiser_on_hostile_pixels(stages, kind):
    clean = {}
    for position in ic.POSITIONS:
        for (size, its) in ic.DENOISE_HOSTILE_RUNS:
            accum, alb, nd, px = ic.denoise_hostile(kind, position, size)
            ref = ic.denoise_all(accum, alb, nd, its)
            c = ic.denoise_case("mixed", *size)
            for it in its:
                what = "%s at %s, %dx%d, %d iterations" % (kind, position, *size, it)
                if (size, it) not in clean:
                    clean[size, it] = stages.denoise(c["accum"], c["albedo"], c["nd"], it)
                got = stages.denoise(accum, alb, nd, it)
                bad = ~dr.usable(accum, alb, nd)
                assert np.array_equal(got[bad].view(np.uint32), ref[it][bad].view(np.uint32)), what       # the pass-through: exact bits
                _denoise_bar(got[~bad], ref[it][~bad], what)
                ic.check_denoise_hostile(got, clean[size, it], accum, alb, nd, px, it, what)


@pytest.mark.parametrize("base,form,gamma", ic.BLEND_HOSTILE_BASES)
def test_blends_on_hostile_pixels(stages, base, form, gamma):
    valid = ic.blend_case(base)
    stages.upload_blend(valid)
    clean = stages.blend(valid, ic.HOSTILE_CAP, form, gamma)
    for (b, f, g, kind, target, position) in ic.blend_hostile_runs():
        if (b, f, g) != (base, form, gamma):
            continue
        what = "%s %s gamma %g: %s in %s at %s" % (base, form, gamma, kind, target, position)
        case, cur, prv = ic.blend_hostile(base, kind, target, position)
        stages.upload_blend(case)
        got = stages.blend(case, ic.HOSTILE_CAP, form, gamma)
        ref, took = ic.blend_mirror(case, ic.HOSTILE_CAP, form, gamma)
        _blend_bar(got, ref, took, case["N"], what)
        through = ~np.isfinite(case["accum"][..., :3]).all(axis=-1)
        assert np.array_equal(got[through].view(np.uint32), ref[through].view(np.uint32)), what
        ic.check_blend_hostile(got, clean, case, cur, prv, gamma, what)


def test_a_poisoned_history_heals(stages):
    """A history with one NaN pixel through pt_temporal_blend twice (ping-pong, identity camera): after the first call the NaN is gone,
    and no pixel but that one differs from the clean chain."""
    case = ic.blend_case("identity")
    (y, x), = ic.hostile_pixels(case["w"], case["h"], "interior")
    chains = []
    for poison in (False, True):
        c = dict(case)
        if poison:
            c["hist"] = ic.plant({"rgb": case["hist"]}, "rgb_nan", "interior")[0]["rgb"]
            assert np.isnan(c["hist"][y, x, :3]).all() and np.isnan(c["hist"]).sum() == 3
        stages.upload_blend(c)
        first = stages.blend(c, 256.0, "static", 0.0, hist="hist", out="out")
        second = stages.blend(c, 256.0, "static", 0.0, hist="out", out="out2")
        chains.append((first, second))
    for clean, got in zip(*chains):
        assert np.isfinite(got).all()
        differs = (clean.view(np.uint32) != got.view(np.uint32)).any(axis=-1)
        assert differs[y, x]
        differs[y, x] = False
        assert not differs.any()
    ref2, took = ic.blend_mirror(dict(case, hist=chains[1][0]), 256.0, "static", 0.0)          # the mirror on the device's own first output
    _blend_bar(chains[1][1], ref2, took, case["N"], "the second blend of the poisoned chain")
