"""pt_convergence_update on the GPU against tests/convergence_ref.py, bit for bit: the state, out_error, out_tiles and the whole info
record as uint32 bits with no tolerance, on synthetic accumulations and on rendered ones; then the calibration of the estimate on the
GPU's own noise, pathtracer.Convergence / renderUntil and acgpt_main --until-error.  Every device buffer lies between the sentinel
guard bands of test_gpu_shapes.Guarded."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import convergence_ref as cr
from test_convergence_host import CAL_BAND, CAL_EXPECTED, CAL_FRAMES, CAL_MEAN
from test_gpu_shapes import SENT, Guarded

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
F = np.float32
# (w, h): one pixel, one partial tile in each direction, a tile less one, a full tile, tiles plus one, narrow images over many tiles,
# more than 65 535 tile rows, and a full-size frame (8160 tiles: more than the grid, so every workgroup strides)
SHAPES = [(1, 1), (1, 17), (17, 1), (15, 15), (16, 16), (17, 33), (4099, 3), (3, 4099), (1, 1048577), (1920, 1080)]
FRAMES = (2, 5, 6)


def _L():
    return _native.hip()


@pytest.fixture(scope="module")
def ctx():
    c = C.c_void_p()
    assert _L().pt_create(C.byref(c), 0) == 0, _L().pt_last_error(None)
    yield c
    _L().pt_destroy(c)


def accumulation(n, seed):
    """float32 [n, 4]: positives log-uniform over 2^-30 .. 2^10; about 6 % of the pixels hold an exact zero, a NaN, an infinity or a
    negative in one channel or in all three; .w is a sentinel that must not be read"""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-30, 10, (n, 4))).astype(F)
    img[:, 3] = np.nan
    special = np.array([0.0, 0.0, np.nan, np.inf, -np.inf, -1.0, -1e-3, -300.0], F)
    pick = rng.random(n) < 0.06
    if n <= 64:
        pick[::3] = True
    m = int(pick.sum())
    vals = special[rng.integers(0, len(special), m)]
    grey = rng.random(m) < 0.5
    px = img[pick]
    px[grey, :3] = vals[grey, None]
    one = ~grey
    px[one, rng.integers(0, 3, int(one.sum()))] = vals[one]
    img[pick] = px
    return img


def c_params(cp):
    return _native.ConvergenceParams(cp["lum_floor"], cp["threshold"], int(cp["quantile_permille"]), int(cp.get("reserved", 0)))


def info_dict(i):
    return dict(frames=int(i.frames), measured_pixels=int(i.measured_pixels), unmeasured_pixels=int(i.unmeasured_pixels), invalid_pixels=int(i.invalid_pixels),
                converged_pixels=int(i.converged_pixels), max_error=F(i.max_error), quantile_error=F(i.quantile_error), reserved=int(i.reserved),
                histogram=np.array(i.histogram, np.uint32))


def n_tiles(w, h):
    return ((w + cr.TILE - 1) // cr.TILE) * ((h + cr.TILE - 1) // cr.TILE)


class Buffers:
    """accumulation, state, out_error and out_tiles of one image size, guarded"""

    def __init__(self, ctx, w, h):
        self.ctx, self.w, self.h, self.n = ctx, w, h, w * h
        self.acc, self.state, self.err, self.tiles = (Guarded(ctx, self.n * 16), Guarded(ctx, self.n * 16), Guarded(ctx, self.n * 4), Guarded(ctx, n_tiles(w, h) * 4))
        self.state.zero()
        self.p = pt.PathTraceParams()
        self.p.width, self.p.height, self.p.accumulationBuffer = w, h, self.acc.ptr

    def call(self, frames, cp, err=True, tiles=True, info=True):
        """(state [n, 4], out_error [n] or None, out_tiles or None, info dict or None) after one update"""
        self.err.fill(); self.tiles.fill()
        inf = _native.ConvergenceInfo()
        rc = _L().pt_convergence_update(self.ctx, C.byref(self.p), frames, C.byref(c_params(cp)), self.state.ptr, self.err.ptr if err else None,
                                        self.tiles.ptr if tiles else None, C.byref(inf) if info else None)
        assert rc == 0, _L().pt_last_error(self.ctx)
        e, t = self.err.read(), self.tiles.read()
        self.acc.check_guards()
        if not err:
            assert np.all(e == SENT)
        if not tiles:
            assert np.all(t == SENT)
        return (self.state.read().view(F).reshape(-1, 4).copy(), e.view(F).copy() if err else None, t.view(F).copy() if tiles else None,
                info_dict(inf) if info else None)

    def free(self):
        for b in (self.acc, self.state, self.err, self.tiles):
            b.free()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    diff = g != w
    assert not diff.any(), "%s: %d values differ, first at %s: %s vs %s" % (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), np.asarray(got)[diff][:4], np.asarray(want)[diff][:4])


def assert_info(got, want, what=""):
    assert np.array_equal(got["histogram"], want["histogram"]), (what, np.flatnonzero(got["histogram"] != want["histogram"])[:8])
    for k in ("frames", "measured_pixels", "unmeasured_pixels", "invalid_pixels", "converged_pixels"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("max_error", "quantile_error"):
        assert F(got[k]).view(np.uint32) == F(want[k]).view(np.uint32), (what, k, got[k], want[k])
    assert got.get("reserved", 0) == 0, what


def assert_call(b, acc, state_before, frames, cp, what):
    """one call on b against the reference; returns the new state"""
    b.acc.put(acc)
    state, err, tiles, info = b.call(frames, cp)
    rs, re_, rt, ri = cr.update(acc, state_before, b.w, b.h, frames, cp)
    assert_bits(state, rs, what + " state")
    assert_bits(err, re_, what + " out_error")
    assert_bits(tiles, rt, what + " out_tiles")
    assert_info(info, ri, what)
    assert info["measured_pixels"] + info["unmeasured_pixels"] + info["invalid_pixels"] == b.n, what
    assert_bits(b.acc.read().view(F).reshape(-1, 4), acc, what + " accumulation")
    return state


# ---- bit identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_bits_equal_the_reference(ctx, w, h):
    b = Buffers(ctx, w, h)
    cp = cr.params(threshold=0.3, quantile_permille=900)
    try:
        state = np.zeros((w * h, 4), F)
        for i, frames in enumerate(FRAMES):
            state = assert_call(b, accumulation(w * h, 7000 + 10 * w + h + i), state, frames, cp, "%dx%d frames %d" % (w, h, frames))
        assert np.all(state[:, 3] <= len(FRAMES))
    finally:
        b.free()


def test_a_flat_image_counts_exactly(ctx):
    """every lane of every wave in one histogram bin (the shared add), then in two, then in three and the other slots"""
    w, h = 500, 300
    b = Buffers(ctx, w, h)
    try:
        flat0, flat1 = np.full((w * h, 4), 0.5, F), np.full((w * h, 4), 0.75, F)
        two = flat1.copy(); two[1::2, :3] = 37.0
        three = two.copy(); three[2::7, :3] = 0.51; three[5::11, 0] = np.nan
        for name, second, bins in (("flat", flat1, 1), ("two bins", two, 2), ("three bins and invalid pixels", three, 3)):
            b.state.zero()
            s = assert_call(b, flat0, np.zeros((w * h, 4), F), 1, cr.params(), name + " first")
            b.acc.put(second)
            _, _, _, info = b.call(3, cr.params())
            assert_info(info, cr.update(second, s, w, h, 3)[3], name)
            assert np.count_nonzero(info["histogram"]) == bins, name
        assert info["invalid_pixels"] == len(range(5, w * h, 11))
    finally:
        b.free()


def test_an_image_without_a_measured_pixel(ctx):
    w, h = 40, 33
    b = Buffers(ctx, w, h)
    try:
        acc = accumulation(w * h, 5)
        b.acc.put(acc)
        state, err, tiles, info = b.call(4, cr.params())
        assert info["measured_pixels"] == 0 and info["max_error"] == 0 and info["quantile_error"] == 0 and not info["histogram"].any()
        assert np.all(tiles == -1) and np.all(err == -1) and tiles.size == 9
        assert_info(info, cr.update(acc, np.zeros((w * h, 4), F), w, h, 4)[3])
    finally:
        b.free()


def test_each_output_may_be_null(ctx):
    w, h = 67, 35
    b = Buffers(ctx, w, h)
    cp = cr.params(threshold=0.5)
    try:
        a0, a1 = accumulation(w * h, 11), accumulation(w * h, 12)
        want = None
        for combo in range(8):
            e, t, i = bool(combo & 1), bool(combo & 2), bool(combo & 4)
            b.state.zero()
            b.acc.put(a0)
            b.call(2, cp, e, t, i)
            b.acc.put(a1)
            state, err, tiles, info = b.call(3, cp, e, t, i)
            if want is None:
                want = cr.update(a1, cr.update(a0, np.zeros((w * h, 4), F), w, h, 2, cp)[0], w, h, 3, cp)
            assert_bits(state, want[0], "state, outputs %d" % combo)
            if e:
                assert_bits(err, want[1], "out_error, outputs %d" % combo)
            if t:
                assert_bits(tiles, want[2], "out_tiles, outputs %d" % combo)
            if i:
                assert_info(info, want[3], "outputs %d" % combo)
    finally:
        b.free()


def test_the_record_is_left_clean_between_two_images(ctx):
    big, small = Buffers(ctx, 300, 200), Buffers(ctx, 33, 17)
    try:
        s = assert_call(big, accumulation(60000, 21), np.zeros((60000, 4), F), 1, cr.params(), "big first")
        assert_call(big, accumulation(60000, 22), s, 2, cr.params(), "big second")
        s = assert_call(small, accumulation(33 * 17, 23), np.zeros((33 * 17, 4), F), 3, cr.params(), "small first")
        assert_call(small, accumulation(33 * 17, 24), s, 7, cr.params(quantile_permille=1), "small second")
    finally:
        big.free(); small.free()


def test_a_restart_in_the_middle_of_a_sequence(ctx):
    w, h = 50, 20
    b = Buffers(ctx, w, h)
    try:
        state = np.zeros((w * h, 4), F)
        for i, frames in enumerate((2, 6, 1, 3, 3, 1 << 24)):
            state = assert_call(b, accumulation(w * h, 30 + i), state, frames, cr.params(), "call %d frames %d" % (i, frames))
            if frames in (1, 3) and i != 3:
                assert np.all(state[:, 3] <= 1)             # started over: one observation, or an invalid pixel's zero
    finally:
        b.free()


# ---- invariance and isolation -------------------------------------------------------------------------------------------------
def test_two_calls_both_math_modes_and_a_group_context_give_the_same_bits(ctx):
    w, h = 200, 150
    accs = [accumulation(w * h, 40 + i) for i in range(3)]
    cp = cr.params(threshold=0.4)
    results = {}
    group = pt.PathTracerState()
    pt.createDeviceContext(group, device_ids=[0])
    try:
        for name, c, mode in (("first", ctx, _native.MATH_IEEE), ("second", ctx, _native.MATH_IEEE), ("fast", ctx, _native.MATH_FAST), ("group", group.context, None)):
            if mode is not None:
                assert _L().pt_set_math_mode(c, mode) == 0
            b = Buffers(c, w, h)
            try:
                out = []
                for a, frames in zip(accs, FRAMES):
                    b.acc.put(a)
                    out.append(b.call(frames, cp))
                results[name] = out
            finally:
                b.free()
    finally:
        assert _L().pt_set_math_mode(ctx, _native.MATH_FAST) == 0
        _L().pt_destroy(group.context)
    for name in ("second", "fast", "group"):
        for (s, e, t, i), (s0, e0, t0, i0) in zip(results[name], results["first"]):
            assert_bits(s, s0, name); assert_bits(e, e0, name); assert_bits(t, t0, name)
            assert_info(i, i0, name)
    state = np.zeros((w * h, 4), F)
    for a, frames, got in zip(accs, FRAMES, results["first"]):
        state = cr.update(a, state, w, h, frames, cp)[0]
        assert_bits(got[0], state, "against the reference")


def _frame(state, ob, index):
    state.params.currentFrameIdx = index
    pt.LaunchCurrentFrame(ob, state)
    st = pt.getStats(state)
    return pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(st)[:24] + bytes(st)[32:]      # the counters without the two timings


def test_the_call_leaves_the_render_state_alone(gpu_state_factory):
    kw = dict(width=64, height=64, max_depth=4, spp=4, direct_lighting=True, importance_sampling=True)
    a, _ = gpu_state_factory(BOX, **kw)
    twin, _ = gpu_state_factory(BOX, **kw)
    oa, ot = (pt.OutputBuffer(pt.OutputBufferType.DEVICE, 64, 64, s) for s in (a, twin))
    conv = pt.Convergence()
    try:
        source_hash = _L().pt_kernel_source_hash()
        acc, fb, st = _frame(a, oa, 0)
        acc_t, fb_t, st_t = _frame(twin, ot, 0)
        assert np.array_equal(bits(acc), bits(acc_t)) and np.array_equal(fb, fb_t) and st == st_t
        stats_before = bytes(pt.getStats(a))
        info = conv.update(a, accum_frames=1)
        assert info["unmeasured_pixels"] == 64 * 64 and not conv.converged
        assert np.array_equal(bits(pt.readAccumulation(a)), bits(acc)) and np.array_equal(oa.getHostPointer(), fb) and bytes(pt.getStats(a)) == stats_before
        acc1, fb1, st1 = _frame(a, oa, 1)
        acc1_t, fb1_t, st1_t = _frame(twin, ot, 1)
        assert np.array_equal(bits(acc1), bits(acc1_t)) and np.array_equal(fb1, fb1_t) and st1 == st1_t
        stats_before = bytes(pt.getStats(a))
        info = conv.update(a, accum_frames=2)
        assert info["measured_pixels"] == 64 * 64 and info["max_error"] > 0
        assert np.array_equal(bits(pt.readAccumulation(a)), bits(acc1)) and np.array_equal(oa.getHostPointer(), fb1) and bytes(pt.getStats(a)) == stats_before
        assert _L().pt_kernel_source_hash() == source_hash
        want = cr.update(acc1.reshape(-1, 4), cr.update(acc.reshape(-1, 4), np.zeros((4096, 4), F), 64, 64, 1)[0], 64, 64, 2)
        assert_bits(conv.stateImage().reshape(-1, 4), want[0], "state")
        assert_bits(conv.errorImage().ravel(), want[1], "errorImage")
        assert_bits(conv.tiles().ravel(), want[2], "tiles")
        assert conv.errorImage().shape == (64, 64) and conv.tiles().shape == (4, 4)
    finally:
        conv.close()
        oa.free(); ot.free()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_context_usable(ctx):
    w, h = 37, 19
    n = w * h
    b = Buffers(ctx, w, h)
    L = _L()
    try:
        a0, a1 = accumulation(n, 50), accumulation(n, 51)
        good = cr.params()
        s0 = assert_call(b, a0, np.zeros((n, 4), F), 2, good, "before")
        b.acc.put(a1)
        nan, inf = float("nan"), float("inf")

        def params(width=w, height=h, acc=b.acc.ptr):
            p = pt.PathTraceParams()
            p.width, p.height, p.accumulationBuffer = width, height, acc
            return p

        ok, okp = c_params(good), params()
        calls = [("null params", "null argument", (None, 3, ok, b.state.ptr, b.err.ptr, b.tiles.ptr)),
                 ("null cp", "null argument", (okp, 3, None, b.state.ptr, b.err.ptr, b.tiles.ptr)),
                 ("null state", "null argument", (okp, 3, ok, None, b.err.ptr, b.tiles.ptr)),
                 ("null accumulation", "null argument", (params(acc=None), 3, ok, b.state.ptr, b.err.ptr, b.tiles.ptr)),
                 ("zero width", "width and height", (params(width=0), 3, ok, b.state.ptr, b.err.ptr, b.tiles.ptr)),
                 ("zero height", "width and height", (params(height=0), 3, ok, b.state.ptr, b.err.ptr, b.tiles.ptr)),
                 ("too many pixels", "too large", (params(width=65536, height=32769), 3, ok, b.state.ptr, b.err.ptr, b.tiles.ptr)),
                 ("no frames", "accum_frames", (okp, 0, ok, b.state.ptr, b.err.ptr, b.tiles.ptr)),
                 ("too many frames", "accum_frames", (okp, (1 << 24) + 1, ok, b.state.ptr, b.err.ptr, b.tiles.ptr))]
        for what, kws in (("lum_floor", [dict(lum_floor=v) for v in (0.0, -0.01, nan, inf)]), ("threshold", [dict(threshold=v) for v in (0.0, -1.0, nan, inf)]),
                          ("quantile_permille", [dict(quantile_permille=v) for v in (0, 1001, 0xFFFFFFFF)]), ("reserved", [dict(reserved=1)])):
            calls += [("bad params %s" % kw, what, (okp, 3, c_params(dict(good, **kw)), b.state.ptr, b.err.ptr, b.tiles.ptr)) for kw in kws]
        calls += [("state is the accumulation", "state overlaps", (okp, 3, ok, b.acc.ptr, b.err.ptr, b.tiles.ptr)),
                  ("state overlaps the accumulation from above", "state overlaps", (okp, 3, ok, b.acc.ptr + 16 * (n - 1), b.err.ptr, b.tiles.ptr)),
                  ("out_error inside the accumulation", "out_error overlaps the accumulation", (okp, 3, ok, b.state.ptr, b.acc.ptr + 64, b.tiles.ptr)),
                  ("out_error inside the state", "out_error overlaps state", (okp, 3, ok, b.state.ptr, b.state.ptr + 16 * n - 4, b.tiles.ptr)),
                  ("out_tiles inside the accumulation", "out_tiles overlaps the accumulation", (okp, 3, ok, b.state.ptr, b.err.ptr, b.acc.ptr)),
                  ("out_tiles inside the state", "out_tiles overlaps state", (okp, 3, ok, b.state.ptr, b.err.ptr, b.state.ptr + 32)),
                  ("out_tiles inside out_error", "out_tiles overlaps out_error", (okp, 3, ok, b.state.ptr, b.err.ptr, b.err.ptr + 4 * n - 4))]
        for name, message, (p, frames, cp, s, e, t) in calls:
            b.err.fill(); b.tiles.fill()
            info = _native.ConvergenceInfo()
            C.memset(C.byref(info), SENT, C.sizeof(info))
            rc = L.pt_convergence_update(ctx, C.byref(p) if p is not None else None, frames, C.byref(cp) if cp is not None else None, s, e, t, C.byref(info))
            assert rc != 0, name
            msg = L.pt_last_error(ctx).decode()
            assert msg.startswith("pt_convergence_update: ") and message in msg, (name, msg)
            assert np.all(b.err.read() == SENT) and np.all(b.tiles.read() == SENT), name
            assert_bits(b.state.read().view(F).reshape(-1, 4), s0, name + " state")
            assert_bits(b.acc.read().view(F).reshape(-1, 4), a1, name + " accumulation")
            assert bytes(info) == bytes([SENT]) * C.sizeof(info), name
        assert L.pt_convergence_update(None, C.byref(okp), 3, C.byref(ok), b.state.ptr, None, None, None) != 0
        assert b"null context" in L.pt_last_error(None)
        assert_call(b, a1, s0, 3, good, "after")
    finally:
        b.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
E2E = dict(width=64, height=64, max_depth=4, spp=16, direct_lighting=True, importance_sampling=True)


@pytest.fixture(scope="module")
def rendered(gpu_state_factory):
    """the Cornell box, 16 launches with an update after each (read-backs kept), then on to 512 frames"""
    state, _ = gpu_state_factory(BOX, **E2E)           # sample_chunks 1, IEEE arithmetic
    conv = pt.Convergence()
    accs, infos = [], []
    try:
        for f in range(CAL_FRAMES):
            state.params.currentFrameIdx = f
            pt.LaunchCurrentFrame(None, state)
            state.params.currentFrameIdx = f + 1
            infos.append(conv.update(state))
            accs.append(pt.readAccumulation(state).reshape(-1, 4))
        out = dict(accs=accs, infos=infos, state=conv.stateImage().reshape(-1, 4), error=conv.errorImage().ravel(), tiles=conv.tiles().ravel())
        while state.params.currentFrameIdx < 512:
            pt.LaunchCurrentFrame(None, state, 16)
            state.params.currentFrameIdx += 16
        out["acc512"] = pt.readAccumulation(state).reshape(-1, 4)
    finally:
        conv.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_a_rendered_sequence_equals_the_reference(rendered):
    s = np.zeros((64 * 64, 4), F)
    for k, (acc, info) in enumerate(zip(rendered["accs"], rendered["infos"])):
        s, err, tiles, ri = cr.update(acc, s, 64, 64, k + 1)
        assert_info(info, ri, "frame %d" % (k + 1))
    assert_bits(rendered["state"], s, "state after 16 launches")
    assert_bits(rendered["error"], err, "out_error")
    assert_bits(rendered["tiles"], tiles, "out_tiles")
    assert np.all(s[:, 3] == CAL_FRAMES) and ri["measured_pixels"] == 64 * 64
    print("16 frames: quantile error %.4f, max %.4f, converged %d of 4096" % (ri["quantile_error"], ri["max_error"], ri["converged_pixels"]))


def test_frame_batches_equal_the_reference(gpu_state_factory):
    state, _ = gpu_state_factory(BOX, **E2E)
    conv = pt.Convergence(maps=False)
    try:
        s = np.zeros((64 * 64, 4), F)
        for batch in (1, 3, 4, 8):
            pt.LaunchCurrentFrame(None, state, batch)
            state.params.currentFrameIdx += batch
            info = conv.update(state)
            s, _, _, ri = cr.update(pt.readAccumulation(state).reshape(-1, 4), s, 64, 64, int(state.params.currentFrameIdx))
            assert_info(info, ri, "after %d frames" % state.params.currentFrameIdx)
        assert_bits(conv.stateImage().reshape(-1, 4), s, "state after the batches 1, 3, 4, 8")
        assert np.all(s[:, 3] == 4) and np.all(s[:, 2] == 16)
    finally:
        conv.close()


def test_calibration_on_the_gpu(rendered):
    """R of tests/test_convergence_host.py from the 16-frame state against the same run carried on to 512 frames: the host test's
    recorded band, moved from its expected value 1 - 16 / 256 to 1 - 16 / 512.  Measured: R = 0.798 (band 0.849 +- 0.422)."""
    s = rendered["state"].astype(np.float64)
    l, v = s[:, 0], s[:, 1] / ((s[:, 3] - 1.0) * CAL_FRAMES)
    l_ref = cr.lum(rendered["acc512"]).astype(np.float64)
    keep = l > 0.01
    ratio = float(((l - l_ref) ** 2)[keep].sum() / v[keep].sum())
    centre = CAL_MEAN - CAL_EXPECTED + (1.0 - CAL_FRAMES / 512.0)
    print("R = %.4f (band %.4f +- %.4f, expected %.4f)" % (ratio, centre, CAL_BAND, 1.0 - CAL_FRAMES / 512.0))
    assert abs(ratio - centre) <= CAL_BAND


# ---- the Python mirror and the app --------------------------------------------------------------------------------------------
def test_render_until_stops_early_or_at_the_cap(gpu_state_factory):
    state, _ = gpu_state_factory(BOX, **E2E)
    loose, tight = pt.Convergence(threshold=0.75), pt.Convergence(threshold=1e-9, permille=1000)
    try:
        used = pt.renderUntil(None, state, loose, 64)
        assert 2 <= used < 64 and loose.converged and loose.info["frames"] == used == state.params.currentFrameIdx
        assert loose.info["converged_pixels"] * 1000 >= loose.info["measured_pixels"] * 950 and loose.info["unmeasured_pixels"] == 0
        state.refreshAccumulationBuffer = True
        pt.updateState(None, state)
        used = pt.renderUntil(None, state, tight, 7, sub_frames=3)
        assert used == 7 and not tight.converged and tight.info["frames"] == 7 and tight.info["measured_pixels"] == 64 * 64
        assert np.all(tight.stateImage()[..., 3] == 3)                      # batches 3, 3, 1
        # a camera change zero-fills the state: the next update is a first observation although the frame count went on
        state.params.cameraEye.x += 1.0
        pt.LaunchCurrentFrame(None, state)
        state.params.currentFrameIdx += 1
        info = tight.update(state)
        assert info["unmeasured_pixels"] == 64 * 64 and info["measured_pixels"] == 0 and np.all(tight.stateImage()[..., 3] == 1)
        assert np.all(tight.errorImage() == -1) and np.all(tight.tiles() == -1)
    finally:
        loose.close(); tight.close()


def test_cli_stops_early_and_writes_the_error_map(gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    base = [exe, "--obj", BOX, "--width", "64", "--height", "64", "--spp-per-launch", "16", "--frames", "64", "--direct-lighting", "--importance-sampling",
            "--out", str(tmp_path / "f.png")]
    r = subprocess.run(base + ["--until-error", "0.75", "--error-out", str(tmp_path / "err.pfm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("Stopped after ") and "(converged)" in last, last
    used = int(last.split()[2])
    assert 2 <= used < 64
    r2 = subprocess.run(base + ["--error-out", str(tmp_path / "x.pfm")], capture_output=True, text=True, timeout=60)
    assert r2.returncode == 2 and "--until-error" in r2.stderr
    # the same run through the Python mirror (the library's defaults, as the app uses them)
    state, _ = gpu_state_factory(BOX, sample_chunks=0, math_mode=None, build_mode=1, **E2E)
    conv = pt.Convergence(threshold=0.75)
    try:
        assert pt.renderUntil(None, state, conv, 64) == used
        err = pt.readPFM(str(tmp_path / "err.pfm"))                     # row 0 = top; the error map's row 0 is the bottom row
        for c in range(3):
            assert_bits(err[::-1, :, c], conv.errorImage(), "error map, channel %d" % c)
        assert ("%d of %d pixels" % (conv.info["converged_pixels"], conv.info["measured_pixels"])) in last
    finally:
        conv.close()
