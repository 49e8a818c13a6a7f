"""Every image kernel at the image shapes its indexing gets wrong: tiny and partial 8 x 4 tiles, 65535-pixel extents, the pixel-class
row limit, both sides of the automatic sample-chunk switch, frame batches, rank partitions up to 8, every queue order, kernel rows,
the post-passes at their borders, and the item and pixel limits.

Two scenes.  The one-emissive-triangle scene of test_gpu_parity.test_edge_cases (DL + IS, maxDepth 2) is exact: every value is
Ke + Ke * Kd or 0, decided by each sample's jitter, and at IEEE the GPU equals the oracle bit for bit in every pixel, so a misplaced,
dropped or doubled sample or pixel fails.  The Cornell box (diffuse, metal, glass) is held to the bars of test_gpu_parity.

Every device output is allocated with a 4 KiB guard band on each side, filled with a sentinel byte: after the call the guards are
unchanged and no sentinel is left inside the image.  tests/test_shapes_host.py pins the work distribution these tests rely on."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import denoise_ref as dr
import motion_ref as mr
import oracle_lib
import temporal_ref as tr
from scene_utils import copy_params, image_mse, make_params
from test_gpu_env_ggx_parity import SAME_FLOOR, THREADS, Pair
from test_gpu_environment import _sky
from test_gpu_parity import MSE_TOL, SAME_BITS_MIN
from test_shapes_host import (AUTO_CHUNK_SHAPES, CLASS_LIMIT_SHAPES, EXACT_SHAPES, EXTREME_SHAPES, PARTITION_SHAPES, PARTITION_WORLDS,
                              TINY_SHAPES, expected_chunks, rank_pixels)

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
GUARD = 4096
SENT = 0xA5
SENT32 = 0xA5A5A5A5
FAST = _native.MATH_FAST


def _L():
    return _native.hip()


class Guarded:
    """nbytes of device memory between two GUARD-byte guard bands, all of it filled with SENT; .ptr points at the middle."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.n = ctx, int(nbytes)
        p = C.c_void_p()
        assert _L().pt_device_malloc(ctx, C.byref(p), self.n + 2 * GUARD) == 0, _L().pt_last_error(ctx)
        self.base = p.value
        self.ptr = self.base + GUARD
        self.fill()

    def fill(self):
        assert _L().pt_device_memset(self.ctx, self.base, SENT, self.n + 2 * GUARD) == 0

    def zero(self):
        assert _L().pt_device_memset(self.ctx, self.ptr, 0, self.n) == 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.n
        assert _L().pt_copy_to_device(self.ctx, self.ptr, a.ctypes.data, a.nbytes) == 0

    def read(self):
        """the bytes inside, after checking that both guards still hold the sentinel"""
        out = np.zeros(self.n + 2 * GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.ctx, out.ctypes.data, self.base, out.nbytes) == 0
        assert np.all(out[:GUARD] == SENT), "write before the buffer: %d bytes" % int((out[:GUARD] != SENT).sum())
        assert np.all(out[GUARD + self.n:] == SENT), "write past the buffer: %d bytes" % int((out[GUARD + self.n:] != SENT).sum())
        return out[GUARD:GUARD + self.n]

    def image(self, w, h):
        return self.read().view(np.float32).reshape(h, w, 4).copy()

    def check_guards(self):
        """the two guards alone (for buffers too large to read back whole)"""
        for off in (0, GUARD + self.n):
            g = np.zeros(GUARD, np.uint8)
            assert _L().pt_copy_to_host(self.ctx, g.ctypes.data, self.base + off, GUARD) == 0
            assert np.all(g == SENT), "write outside the buffer at guard offset %d" % off

    def window(self, w, x0, y0, ww, hh):
        """float32 [hh, ww, 4] of an image w pixels wide, one copy per row"""
        out = np.zeros((hh, ww, 4), np.float32)
        for r in range(hh):
            off = ((y0 + r) * w + x0) * 16
            assert _L().pt_copy_to_host(self.ctx, out[r].ctypes.data, self.ptr + off, ww * 16) == 0
        return out

    def column(self, w, h, x):
        out = np.zeros((h, 1, 4), np.float32)
        for y in range(h):
            assert _L().pt_copy_to_host(self.ctx, out[y].ctypes.data, self.ptr + (y * w + x) * 16, 16) == 0
        return out

    def free(self):
        if self.base:
            _L().pt_device_free(self.ctx, self.base)
            self.base = None


def _stats(ctx):
    s = _native.Stats()
    assert _L().pt_get_stats(ctx, C.byref(s)) == 0
    return s


def _launch(ctx, p, acc, fb=None, frames=1, frame0=0):
    q = copy_params(p)
    q.accumulationBuffer, q.frameBuffer = acc.ptr, (fb.ptr if fb is not None else None)
    q.handle = _L().pt_scene_handle(ctx)
    q.currentFrameIdx = frame0
    rc = _L().pt_launch_frames(ctx, C.byref(q), frames)
    assert rc == 0, _L().pt_last_error(ctx)
    return _stats(ctx)


def render(ctx, p, frames=1, fuse=None, with_fb=True):
    """(accumulation [h, w, 4], framebuffer [h, w, 4] uint8 or None, [stats]) of `frames` frames into fresh guarded buffers, `fuse`
    frames per pt_launch_frames (default: all in one); every pixel of the image must have been written."""
    w, h = int(p.width), int(p.height)
    acc, fb = Guarded(ctx, w * h * 16), (Guarded(ctx, w * h * 4) if with_fb else None)
    try:
        fuse = fuse or frames
        sts, f = [], 0
        while f < frames:
            n = min(fuse, frames - f)
            sts.append(_launch(ctx, p, acc, fb, n, f))
            f += n
        a = acc.image(w, h)
        assert not np.any(a.view(np.uint32) == SENT32), "%d accumulation words never written" % int((a.view(np.uint32) == SENT32).sum())
        b = None
        if fb is not None:
            b = fb.read().reshape(h, w, 4).copy()
            assert np.all(b[..., 3] == 255), "%d framebuffer pixels never written" % int((b[..., 3] != 255).sum())
        return a, b, sts
    finally:
        acc.free()
        if fb is not None:
            fb.free()


def oracle_render(sc, p, frames=1, chunks=1):
    acc = fb = None
    tot = {"radiance_rays": 0, "shadow_rays": 0, "paths": 0}
    for f in range(frames):
        q = copy_params(p)
        q.currentFrameIdx = f
        acc, fb, st, _ = sc.render(q, accumulation=acc, threads=THREADS, chunks=chunks)
        for k in tot:
            tot[k] += st[k]
    return acc, fb, tot


def _bits(a):
    return a.view(np.uint32)


@pytest.fixture(scope="module")
def exact(gpu_state_factory, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("one")
    (d / "one.obj").write_text("mtllib one.mtl\nv 100 100 300\nv 450 100 300\nv 278 450 300\nusemtl m\nf 1 2 3\n")
    (d / "one.mtl").write_text("newmtl m\nKd 0.5 0.6 0.7\nKe 1 2 3\n")
    state, obj = gpu_state_factory(str(d / "one.obj"), width=8, height=8, max_depth=2, spp=2)
    sc = oracle.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    return state, sc


@pytest.fixture(scope="module")
def box(gpu_state_factory, oracle):
    state, obj = gpu_state_factory(BOX, width=8, height=8, max_depth=4, spp=4)
    sc = oracle.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    return state, obj, sc


@pytest.fixture(params=["ieee", "fast"])
def both_modes(request, exact, box):
    """GPU-against-GPU invariants hold at the oracle's level and in the library's default arithmetic."""
    for st in (exact[0], box[0]):
        pt.setMathMode(st, request.param)
    yield request.param
    for st in (exact[0], box[0]):
        pt.setMathMode(st, "ieee")


def _exact_params(w, h, spp):
    return make_params(w, h, spp, 2, True, True)


def _assert_exact(acc, fb, sts, ref, ref_fb, ref_st, w, h, spp, frames=1, what=""):
    diff = ~np.all(_bits(acc) == _bits(ref), axis=-1)
    assert not diff.any(), "%s: %d pixels differ, first at (y, x) %s" % (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    if fb is not None:
        assert np.array_equal(fb, ref_fb), what
    assert np.all(acc[..., 3] == 1.0), what
    assert sum(int(s.paths) for s in sts) == w * h * spp * frames, what
    assert all(int(s.pixels) == w * h for s in sts), what
    assert sum(int(s.radiance_rays) for s in sts) == ref_st["radiance_rays"], what
    assert sum(int(s.shadow_rays) for s in sts) == ref_st["shadow_rays"], what


# ---- shapes x decomposition against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", EXACT_SHAPES, ids=["%dx%d" % s for s in EXACT_SHAPES])
def test_exact_scene_at_every_shape(exact, w, h):
    """Tiny and partial tiles, 65535-pixel extents and the pixel-class limit: bit-equal to the oracle, counters exact, nothing written
    outside the image.  At the extreme and limit shapes pixel classes off give the same bits (at 2 x 32768 they are off anyway)."""
    state, sc = exact
    L = _L()
    spp = 2 if max(w, h) > 1000 else 4
    p = _exact_params(w, h, spp)
    ref, ref_fb, ref_st = oracle_render(sc, p)
    assert ref_st["paths"] == w * h * spp
    acc, fb, sts = render(state.context, p)
    _assert_exact(acc, fb, sts, ref, ref_fb, ref_st, w, h, spp, what="%dx%d" % (w, h))
    if (w, h) in CLASS_LIMIT_SHAPES or (w, h) in EXTREME_SHAPES:
        try:
            assert L.pt_debug_pixel_classes(state.context, 0) == 0
            acc0, fb0, sts0 = render(state.context, p)
        finally:
            L.pt_debug_pixel_classes(state.context, 1)
        _assert_exact(acc0, fb0, sts0, ref, ref_fb, ref_st, w, h, spp, what="%dx%d classes off" % (w, h))
    if (w, h) in TINY_SHAPES:           # the default arithmetic: the same emitter hits, the same paths
        try:
            pt.setMathMode(state, "fast")
            facc, _, fst = render(state.context, p)
        finally:
            pt.setMathMode(state, "ieee")
        assert np.array_equal(facc[..., :3] > 0, ref[..., :3] > 0) and image_mse(facc, ref) < MSE_TOL
        assert int(fst[0].paths) == w * h * spp and int(fst[0].math_mode) == FAST


@pytest.mark.parametrize("w,h,world", AUTO_CHUNK_SHAPES, ids=["%dx%d-world%d" % s for s in AUTO_CHUNK_SHAPES])
def test_auto_chunk_switch(exact, w, h, world):
    """Both sides of 2^20 pixels per rank at 64 spp (at 32 spp the 4-sample floor caps both sides at 8 runs, so the switch would not
    show): the automatic chunk count is the rule's, and windows at the corners and the middle equal oracle.render_window(chunks=used)
    bit for bit.  On 2 ranks every pixel is written by exactly one rank."""
    state, sc = exact
    L = _L()
    spp = 64
    p = _exact_params(w, h, spp)
    want = expected_chunks(w, h, world, spp)
    wins = [(0, 0, 64, 8), (w - 64, h - 8, 64, 8), (w // 2 - 32, h // 2 - 4, 64, 8), (0, h - 4, 32, 4), (w - 32, 0, 32, 4)]
    ref = None
    for win in wins:
        ref, _, _ = oracle_lib.render_window(sc, copy_params(p), win, accumulation=ref, threads=THREADS, chunks=want)
    got = np.zeros((h, w, 4), np.float32)
    owned = np.zeros((h, w), np.int32)
    try:
        assert L.pt_set_sample_chunks(state.context, 0) == 0
        for rank in range(world):
            assert L.pt_set_partition(state.context, rank, world) == 0
            acc = Guarded(state.context, w * h * 16)
            try:
                acc.zero()
                st = _launch(state.context, p, acc)
                part = acc.image(w, h)
            finally:
                acc.free()
            assert int(st.sample_chunks) == want, (st.sample_chunks, want)
            mine = part[..., 3] == 1.0
            assert int(st.pixels) == int(mine.sum()) and int(st.paths) == int(mine.sum()) * spp
            got[mine] = part[mine]
            owned += mine
    finally:
        L.pt_set_partition(state.context, 0, 1)
        L.pt_set_sample_chunks(state.context, 1)
    assert np.all(owned == 1)
    for x0, y0, ww, hh in wins:
        a, b = got[y0:y0 + hh, x0:x0 + ww], ref[y0:y0 + hh, x0:x0 + ww]
        assert np.array_equal(_bits(a), _bits(b)), ("window", (x0, y0, ww, hh))


@pytest.mark.parametrize("spp", [1, 2, 3, 4, 5, 7, 8, 12, 64, 96])
def test_spp_under_auto_chunks(exact, spp):
    state, sc = exact
    L = _L()
    p = _exact_params(17, 13, spp)
    want = expected_chunks(17, 13, 1, spp)
    try:
        assert L.pt_set_sample_chunks(state.context, 0) == 0
        acc, fb, sts = render(state.context, p)
    finally:
        L.pt_set_sample_chunks(state.context, 1)
    assert int(sts[0].sample_chunks) == want
    ref, ref_fb, ref_st = oracle_render(sc, p, chunks=want)
    _assert_exact(acc, fb, sts, ref, ref_fb, ref_st, 17, 13, spp, what="spp %d" % spp)


@pytest.mark.parametrize("w,h", [(1, 1), (9, 5), (65535, 1)], ids=["1x1", "9x5", "65535x1"])
def test_frame_batches_at_edge_shapes(exact, box, both_modes, w, h):
    """pt_launch_frames with 1, 3 and 7 frames (padded sub-frames at 3 and 7) equals separate launches bit for bit, and so does a
    batch that continues an accumulation (3 single frames, then 4 in one launch); at IEEE the exact scene's 7 frames equal the oracle."""
    for state, spp, depth in ((exact[0], 2, 2), (box[0], 4, 4)):
        p = make_params(w, h, spp, depth, True, True)
        want = want_fb = st1 = None
        for frames in (1, 3, 7):
            want, want_fb, st1 = render(state.context, p, frames=frames, fuse=1)
            got, got_fb, stn = render(state.context, p, frames=frames)
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got_fb, want_fb), frames
            assert int(stn[0].paths) == w * h * spp * frames and int(stn[0].pixels) == w * h
            assert int(stn[0].radiance_rays) == sum(int(s.radiance_rays) for s in st1)
            assert int(stn[0].shadow_rays) == sum(int(s.shadow_rays) for s in st1)
        acc, fb = Guarded(state.context, w * h * 16), Guarded(state.context, w * h * 4)
        try:
            for f in range(3):
                _launch(state.context, p, acc, fb, 1, f)
            _launch(state.context, p, acc, fb, 4, 3)
            cont, cont_fb = acc.image(w, h), fb.read().reshape(h, w, 4).copy()
        finally:
            acc.free(); fb.free()
        assert np.array_equal(_bits(cont), _bits(want)) and np.array_equal(cont_fb, want_fb)
        if both_modes == "ieee" and state is exact[0]:
            ref, ref_fb, ref_st = oracle_render(exact[1], p, frames=7)
            assert np.array_equal(_bits(want), _bits(ref)) and np.array_equal(want_fb, ref_fb)
            assert sum(int(s.radiance_rays) for s in st1) == ref_st["radiance_rays"]


@pytest.mark.parametrize("world", PARTITION_WORLDS)
def test_partitions(box, oracle, both_modes, world):
    """World 2, 3, 4, 5 and 8 at 5 x 3, 9 x 5, 17 x 13 and 100 x 52: each rank writes exactly the pixels oracle.sample_pixel gives it
    (the others keep the sentinel), stats.pixels counts them, and together the ranks' pixels are the single-rank launch's bits.  On
    8 ranks a 5 x 3 image leaves ranks without a pixel: their launch succeeds and writes nothing."""
    state = box[0]
    L = _L()
    try:
        assert L.pt_set_sample_chunks(state.context, 4) == 0
        for w, h in PARTITION_SHAPES:
            p = make_params(w, h, 4, 4, True, True)
            whole, _, _ = render(state.context, p, with_fb=False)
            cover = np.zeros((h, w), np.int32)
            empty_ranks = 0
            for rank in range(world):
                assert L.pt_set_partition(state.context, rank, world) == 0
                acc = Guarded(state.context, w * h * 16)
                try:
                    st = _launch(state.context, p, acc)
                    part = acc.image(w, h)
                finally:
                    acc.free()
                xy = rank_pixels(oracle, world, w, h, rank)
                xy = xy[(xy[:, 0] < w) & (xy[:, 1] < h)]
                expect = np.zeros((h, w), bool)
                expect[xy[:, 1], xy[:, 0]] = True
                written = ~np.all(_bits(part) == SENT32, axis=-1)
                assert np.array_equal(written, expect), (w, h, rank)
                assert np.all(_bits(part)[~expect] == SENT32), (w, h, rank)
                assert np.array_equal(_bits(part)[expect], _bits(whole)[expect]), (w, h, rank)
                assert int(st.pixels) == int(expect.sum()) and int(st.paths) == int(expect.sum()) * 4, (w, h, rank)
                cover += expect
                empty_ranks += int(not expect.any())
            assert L.pt_set_partition(state.context, 0, 1) == 0
            assert np.all(cover == 1), (w, h)
            if (w, h, world) == (5, 3, 8):
                assert empty_ranks > 0
    finally:
        L.pt_set_partition(state.context, 0, 1)
        L.pt_set_sample_chunks(state.context, 1)


QUEUE_SHAPES = [(1, 1), (9, 5), (65535, 1), (1, 65535)]


@pytest.mark.parametrize("w,h", QUEUE_SHAPES, ids=["%dx%d" % s for s in QUEUE_SHAPES])
def test_queue_order_and_classes(box, both_modes, w, h):
    """pt_debug_queue_order 0-3 x pt_debug_pixel_classes 0 / 1 (orders 1 and 2 deal units to 8 shards round robin, and a tiny image
    has fewer units than shards): the same bits and counters, two frames in one launch, four sample runs."""
    state = box[0]
    L = _L()
    p = make_params(w, h, 4, 4, True, True)
    ref = None
    try:
        assert L.pt_set_sample_chunks(state.context, 4) == 0
        for classes, order in itertools.product((0, 1), range(4)):
            assert L.pt_debug_pixel_classes(state.context, classes) == 0 and L.pt_debug_queue_order(state.context, order) == 0
            acc, fb, st = render(state.context, p, frames=2)
            cnt = (int(st[0].radiance_rays), int(st[0].shadow_rays), int(st[0].paths), int(st[0].pixels))
            if ref is None:
                ref = (acc, fb, cnt)
                assert cnt[2] == w * h * 4 * 2 and cnt[3] == w * h
            else:
                assert np.array_equal(_bits(acc), _bits(ref[0])) and np.array_equal(fb, ref[1]), (classes, order)
                assert cnt == ref[2], (classes, order)
    finally:
        L.pt_debug_pixel_classes(state.context, 1); L.pt_debug_queue_order(state.context, 1)
        L.pt_set_sample_chunks(state.context, 1)


ROW_SHAPES = {"small": [(1, 1), (9, 5), (31, 33)], "65535x1": [(65535, 1)], "1x65535": [(1, 65535)]}
ROWS = {  # name: (light mode, microfacet, roughness key of test_gpu_env_ggx_parity, map, forced variant, bit-identical floor)
    "default": (0, False, None, None, -1, SAME_BITS_MIN),
    "windowed": (0, False, None, None, 9, SAME_BITS_MIN),
    "lights": (1, False, None, None, -1, SAME_BITS_MIN),
    "env": (0, False, None, "sky", -1, SAME_FLOOR[10]),
    "lights_env": (1, False, None, "sky", -1, SAME_FLOOR[12]),
    "lights_ggx_env": (1, True, "B", "sky", -1, SAME_FLOOR[14]),         # metal Pr 0.3
}


def _odd_sky():
    """a sky map whose texel seams lie off u = 1/4, 1/2, 3/4 and v = 1/2 (31 x 63 texels)"""
    return _sky(31, 63, seed=5)


@pytest.mark.parametrize("group", list(ROW_SHAPES))
@pytest.mark.parametrize("row", list(ROWS))
def test_kernel_rows_at_edge_shapes(oracle, row, group):
    """The default row, the windowed-stack row forced by pt_set_tuning, light mode 1, ENV, LIGHTS ENV and LIGHTS GGX ENV on the Cornell
    box at 1 x 1, 9 x 5 and 31 x 33 together, at 65535 x 1 and at 1 x 65535, at IEEE, against the oracle: MSE under MSE_TOL at every
    shape, paths exact, and over the group's shapes the rays within the parity tests' 2e-3 and the bit-identical pixels above their
    floor.

    The map is looked up at the nearest texel, u = 0.5 + atan2f(d.x, -d.z) / 2 pi, v = acosf(d.y) / pi.  At 65535 x 1 U is 65535 times
    W, so nearly every camera ray that misses leaves at d ~ (+-1, ~0, ~0): u lands at 1/4 or 3/4 and v at 1/2, within an ulp of a texel
    corner of any map whose sides are multiples of 4 and 2, and an ulp between ROCm's atan2f / acosf and glibc's moves a whole sample
    to a neighbouring texel.  Measured with the 32 x 64 sky: MSE 5.4e-5, the same in rows 10, 12 and 14; with that sky made constant
    along u, 1.1e-4 (the v seam alone).  That is the conditioning of the lookup at those directions, not an index, so the extreme
    shapes use a 31 x 63 map, whose seams lie away from those directions, and keep the usual bars."""
    light, micro, rough, env, forced, floor = ROWS[row]
    pr = Pair(oracle, BOX, light, micro=micro, rough=rough, env=env if group == "small" else None)
    L = pr.c.L
    try:
        if env and group != "small":
            img = _odd_sky()
            assert pr.c.env(img) == 0, pr.c.err()
            pr.sc.set_environment(img)
        if forced >= 0:
            assert L.pt_set_tuning(pr.c.ctx, 0, forced) == 0, pr.c.err()
        same_n = same_d = 0
        rays = [0, 0, 0, 0]
        for w, h in ROW_SHAPES[group]:
            spp = 2 if max(w, h) > 1000 else 4
            p = make_params(w, h, spp, 6, True, True)
            acc, fb, sts = render(pr.c.ctx, p)
            ref, _, ref_st = oracle_render(pr.sc, p)
            st = sts[0]
            if forced >= 0:
                assert int(st.variant) == forced
            mse = image_mse(acc, ref)
            assert np.isfinite(acc).all() and mse < MSE_TOL, (row, w, h, mse)
            assert int(st.paths) == ref_st["paths"] == w * h * spp
            same_n += int(np.all(_bits(acc) == _bits(ref), axis=-1).sum())
            same_d += w * h
            rays[0] += int(st.radiance_rays); rays[1] += ref_st["radiance_rays"]
            rays[2] += int(st.shadow_rays); rays[3] += ref_st["shadow_rays"]
        print("%s %s: %.4f of %d pixels bit-identical; radiance rays %d / %d, shadow rays %d / %d" % ((row, group, same_n / same_d, same_d) + tuple(rays)))
        assert same_n / same_d > floor
        assert abs(rays[0] - rays[1]) <= 2e-3 * rays[1] and abs(rays[2] - rays[3]) <= 2e-3 * max(1, rays[3])
    finally:
        if forced >= 0:
            L.pt_set_tuning(pr.c.ctx, 0, -1)
        pr.close()


# ---- post-passes at their edges --------------------------------------------------------------------------------------------------
def _features(state, q):
    w, h = int(q.width), int(q.height)
    alb, nd = Guarded(state.context, w * h * 16), Guarded(state.context, w * h * 16)
    try:
        assert _L().pt_render_features(state.context, C.byref(q), alb.ptr, nd.ptr) == 0, _L().pt_last_error(state.context)
        return alb.image(w, h), nd.image(w, h)
    finally:
        alb.free(); nd.free()


def _camera(q):
    return q.cameraEye.tuple(), q.cameraU.tuple(), q.cameraV.tuple(), q.cameraW.tuple()


def _diffuse(obj):
    return np.array([[m.diffuse.x, m.diffuse.y, m.diffuse.z] for m in obj.getMaterials()], np.float32)


def _check_features(state, obj, q, alb, nd):
    """as test_gpu_denoise._check_features, for any shape (a 1 x 1 image may be all hit or all miss)"""
    w, h = int(q.width), int(q.height)
    rays = dr.pixel_rays(w, h, *_camera(q))
    n = rays.shape[0]
    t = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32)
    assert _L().pt_trace_closest(state.context, rays.ctypes.data, n, t.ctypes.data, prim.ctypes.data) == 0
    assert np.array_equal(alb[..., 3].reshape(-1).view(np.uint32), prim)
    assert np.array_equal(nd[..., 3].reshape(-1).view(np.uint32), t.view(np.uint32))
    ref_alb, ref_nd = dr.features_from_hits(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), _diffuse(obj))
    assert np.abs(nd.reshape(-1, 4)[:, :3] - ref_nd[:, :3]).max() <= 1e-5
    assert np.array_equal(alb.reshape(-1, 4)[:, :3], ref_alb[:, :3])


FEATURE_SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (65535, 1)]


@pytest.mark.parametrize("w,h", FEATURE_SHAPES, ids=["%dx%d" % s for s in FEATURE_SHAPES])
def test_features_at_edge_shapes(box, w, h):
    state, obj, _ = box
    q = make_params(w, h, 4, 4, True, True)
    alb, nd = _features(state, q)
    _check_features(state, obj, q, alb, nd)


DENOISE_CASES = [((1, 1), 1), ((1, 1), 5), ((1, 7), 3), ((7, 1), 3), ((2, 2), 2), ((4, 3), 5), ((5, 5), 1), ((5, 5), 8),
                 ((97, 61), 1), ((97, 61), 5), ((97, 61), 6), ((97, 61), 7), ((97, 61), 8)]


@pytest.mark.parametrize("size,iterations", DENOISE_CASES, ids=["%dx%d-it%d" % (s[0], s[1], i) for s, i in DENOISE_CASES])
def test_denoise_at_edge_shapes(box, size, iterations):
    """Every 5 x 5 window clipped on both sides, and a-trous steps beyond the image (iterations 6-8 at 97 x 61: steps 32-128):
    against denoise_ref at the 1e-4 relative / 1e-5 absolute bar, deterministic, the same in both math modes, the inputs left
    alone; iterations 0 and 9 refused with the context left usable."""
    state, obj, _ = box
    L = _L()
    w, h = size
    q = make_params(w, h, 8, 4, True, True)
    acc, _, _ = render(state.context, q, with_fb=False)
    alb, nd = _features(state, q)
    ref = dr.denoise(acc, alb, nd, iterations)
    bufs = [Guarded(state.context, w * h * 16) for _ in range(4)]
    try:
        for b, a in zip(bufs, (acc, alb, nd)):
            b.put(a)
        d = copy_params(q)
        d.accumulationBuffer = bufs[0].ptr

        def run():
            bufs[3].fill()
            assert L.pt_denoise(state.context, C.byref(d), bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, iterations) == 0, L.pt_last_error(state.context)
            return bufs[3].image(w, h)
        got = run()
        bad = ~(np.abs(got - ref) <= np.maximum(1e-4 * np.abs(ref), 1e-5))
        assert not bad.any(), "%d channels off, worst %s vs %s" % (bad.sum(), got[bad][:4], ref[bad][:4])
        assert np.array_equal(_bits(run()), _bits(got))
        try:
            pt.setMathMode(state, "fast")
            assert np.array_equal(_bits(run()), _bits(got))
        finally:
            pt.setMathMode(state, "ieee")
        for bad_it in (0, 9):
            assert L.pt_denoise(state.context, C.byref(d), bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bad_it) != 0
        assert np.array_equal(_bits(run()), _bits(got))
        for b, a in zip(bufs, (acc, alb, nd)):
            assert np.array_equal(_bits(b.image(w, h)), _bits(a))
    finally:
        for b in bufs:
            b.free()


def _view(state, w, h, orbit, spp):
    q = copy_params(state.params)
    q.width, q.height, q.samplesPerPixel, q.maxDepth = w, h, spp, 8
    q.useDirectLighting = q.useImportanceSampling = 1
    tr.set_camera(q, *tr.orbit_camera(w, h, *orbit))
    acc, _, _ = render(state.context, q, with_fb=False)
    return q, acc


TEMPORAL_CUR = [(1, 1), (1, 9), (9, 1)]
TEMPORAL_PREV = [(1, 1), (1, 9), (9, 1), (97, 61)]


@pytest.mark.parametrize("cur", TEMPORAL_CUR, ids=["%dx%d" % s for s in TEMPORAL_CUR])
def test_temporal_blend_at_edge_shapes(box, cur):
    """pt_temporal_blend with the current view at 1 x 1, 1 x N and N x 1 and the previous view at those and at 97 x 61.  A previous
    view one pixel wide (tall) puts every reprojected point at fx (fy) in [-0.5, 0.5): the taps at -1 and at w' - 1 are taken or
    skipped there.  Against temporal_ref at test_gpu_temporal's bar (weights bit-equal, colour within 1e-6), caps 0, 12 and 256;
    and pt_temporal_blend_motion (unmoved vertices) against motion_ref with the clip off and at gamma 4, its 3 x 3 neighbourhood
    clipped on every side."""
    state, obj, _ = box
    L = _L()
    w, h = cur
    bsdf = tr.tri_bsdf(obj)
    q, acc = _view(state, w, h, (3, 2), 8)
    feat = _features(state, q)
    idx = np.asarray(obj.getIndexBuffer(), np.uint32)
    verts = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    vd = Guarded(state.context, verts.nbytes)
    vd.put(verts)
    took_any = 0
    for wp, hp in TEMPORAL_PREV:
        pq, hist = _view(state, wp, hp, (0, 0), 16)
        hist[..., 3] = 16.0
        pfeat = _features(state, pq)
        arrays = (acc, feat[0], feat[1], hist, pfeat[0], pfeat[1])
        dev = [Guarded(state.context, a.nbytes) for a in arrays]
        out = Guarded(state.context, w * h * 16)
        try:
            for b, a in zip(dev, arrays):
                b.put(a)
            c = copy_params(q)
            c.accumulationBuffer = dev[0].ptr
            for cap in (0.0, 12.0, 256.0):
                out.fill()
                rc = L.pt_temporal_blend(state.context, C.byref(c), 8, dev[1].ptr, dev[2].ptr, C.byref(pq), dev[3].ptr, dev[4].ptr, dev[5].ptr,
                                         cap, out.ptr)
                assert rc == 0, L.pt_last_error(state.context)
                got = out.image(w, h)
                ref, took = tr.blend(acc, feat[0], feat[1], tr.camera_of(q), 8, bsdf, cap, (tr.camera_of(pq), hist, *pfeat))
                assert np.array_equal(got[..., 3].view(np.uint32), ref[..., 3].view(np.uint32)), ((wp, hp), cap)
                assert np.array_equal(got[..., 3] != 8.0, took), ((wp, hp), cap)
                bad = ~(np.abs(got[..., :3] - ref[..., :3]) <= 1e-6 * np.abs(ref[..., :3]))
                assert not bad.any(), ((wp, hp), cap, got[..., :3][bad][:4], ref[..., :3][bad][:4])
                if cap == 0.0:
                    assert not took.any()
                took_any += int(took.sum())
                for gamma in (0.0, 4.0):       # pt_temporal_blend_motion: the clip's 3 x 3 neighbourhood clipped at every border
                    out.fill()
                    rc = L.pt_temporal_blend_motion(state.context, C.byref(c), 8, dev[1].ptr, dev[2].ptr, C.byref(pq), dev[3].ptr, dev[4].ptr,
                                                    dev[5].ptr, vd.ptr, vd.ptr, verts.shape[0], cap, gamma, out.ptr)
                    assert rc == 0, L.pt_last_error(state.context)
                    got = out.image(w, h)
                    ref, took = mr.blend(acc, feat[0], feat[1], tr.camera_of(q), 8, bsdf, cap, (tr.camera_of(pq), hist, *pfeat), idx, verts, verts, gamma)
                    assert np.array_equal(got[..., 3].view(np.uint32), ref[..., 3].view(np.uint32)), ((wp, hp), cap, gamma)
                    assert np.array_equal(got[..., 3] != 8.0, took), ((wp, hp), cap, gamma)
                    bad = ~(np.abs(got[..., :3] - ref[..., :3]) <= 1e-6 * np.abs(ref[..., :3]))
                    assert not bad.any(), ((wp, hp), cap, gamma, got[..., :3][bad][:4], ref[..., :3][bad][:4])
        finally:
            for b in dev + [out]:
                b.free()
    vd.check_guards()
    vd.free()
    print("%dx%d: %d pixel blends took history" % (w, h, took_any))


# ---- limits ----------------------------------------------------------------------------------------------------------------------
def test_post_pass_pixel_limit(box):
    """Features and the denoiser take at most 2^28 pixels and 65535 per side: 65535 x 4097, 16384 x 16385, 65536 x 1 and 1 x 65536
    are refused before any device work (the buffers handed in are 4 KiB and keep their sentinel), and the context stays usable."""
    state, obj, _ = box
    L = _L()
    bufs = [Guarded(state.context, 4096) for _ in range(4)]
    try:
        for w, h in ((65535, 4097), (16384, 16385), (65536, 1), (1, 65536)):
            q = make_params(w, h, 1, 1, True, True)
            q.accumulationBuffer = bufs[0].ptr
            assert L.pt_render_features(state.context, C.byref(q), bufs[1].ptr, bufs[2].ptr) != 0
            assert b"too large" in L.pt_last_error(state.context)
            assert L.pt_denoise(state.context, C.byref(q), bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 1) != 0
            assert b"too large" in L.pt_last_error(state.context)
        for b in bufs:
            assert np.all(b.read() == SENT)
    finally:
        for b in bufs:
            b.free()
    q = make_params(3, 5, 4, 4, True, True)
    alb, nd = _features(state, q)
    _check_features(state, obj, q, alb, nd)


def test_render_item_limit(exact):
    """The launch refuses 2^31 work items before any device work: 65535 x 16381 in 2 sample runs (8192 x 4096 strips x 32 x 2),
    65535 x 32765 in one (8192 x 8192 strips x 32), and 65535 x 65535 and 65529 x 65533 (2^32 slots: a 32-bit count wrapped to 0,
    and the launch succeeded and wrote nothing).  One sub-frame each, so no frame split by the scratch limit can turn a refused batch
    into admitted launches.  The buffer handed in is 4 KiB and keeps its sentinel; the context stays usable."""
    state, sc = exact
    L = _L()
    acc = Guarded(state.context, 4096)
    try:
        for w, h, chunks in ((65535, 16381, 2), (65535, 32765, 1), (65535, 65535, 1), (65529, 65533, 1)):
            q = _exact_params(w, h, chunks)
            q.maxDepth = 1
            q.accumulationBuffer, q.frameBuffer, q.handle = acc.ptr, None, L.pt_scene_handle(state.context)
            assert L.pt_set_sample_chunks(state.context, chunks) == 0
            try:
                assert L.pt_launch_frames(state.context, C.byref(q), 1) != 0, (w, h, chunks)
                err = L.pt_last_error(state.context)
            finally:
                assert L.pt_set_sample_chunks(state.context, 1) == 0
            assert b"2^31 work items" in err, (w, h, err)
        assert np.all(acc.read() == SENT)
    finally:
        acc.free()
    p = _exact_params(9, 5, 4)
    ref, ref_fb, ref_st = oracle_render(sc, p)
    a, fb, sts = render(state.context, p)
    _assert_exact(a, fb, sts, ref, ref_fb, ref_st, 9, 5, 4)


# ---- past 2^28 pixels and near 2^31 items ----------------------------------------------------------------------------------------
def _free_device_bytes():
    import torch
    return int(torch.cuda.mem_get_info()[0])


def _pixel_rays_at(w, h, xs, ys, eye, U, V, W):
    """denoise_ref.pixel_rays for the pixels (xs[i], ys[i]) only, in the same fp32 operations"""
    F = np.float32
    U, V, W, eye = (np.asarray(a, np.float32) for a in (U, V, W, eye))
    dx = F(2.0) * ((np.asarray(xs, np.float32) + F(0.5)) / F(w)) - F(1.0)
    dy = F(2.0) * ((np.asarray(ys, np.float32) + F(0.5)) / F(h)) - F(1.0)
    D = (dx[:, None] * U[None, :] + dy[:, None] * V[None, :]) + W[None, :]
    dot = D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2]
    inv = F(1.0) / np.sqrt(dot)
    r = np.zeros((len(dx), 8), np.float32)
    r[:, 0:3] = eye
    r[:, 3:6] = D * inv[:, None]
    r[:, 6] = F(0.01)
    r[:, 7] = F(1e16)
    return r


def _check_feature_pixels(state, obj, q, xs, ys, alb, nd):
    w, h = int(q.width), int(q.height)
    rays = _pixel_rays_at(w, h, xs, ys, *_camera(q))
    n = rays.shape[0]
    t = np.zeros(n, np.float32); prim = np.zeros(n, np.uint32)
    assert _L().pt_trace_closest(state.context, rays.ctypes.data, n, t.ctypes.data, prim.ctypes.data) == 0
    assert np.array_equal(alb[:, 3].view(np.uint32), prim)
    assert np.array_equal(nd[:, 3].view(np.uint32), t.view(np.uint32))
    ref_alb, ref_nd = dr.features_from_hits(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), _diffuse(obj))
    assert np.abs(nd[:, :3] - ref_nd[:, :3]).max() <= 1e-5
    assert np.array_equal(alb[:, :3], ref_alb[:, :3])


@pytest.mark.parametrize("w,h", [(65535, 4096), (16384, 16384)], ids=["65535x4096", "16384x16384"])
def test_post_passes_at_2_28_pixels(box, w, h):
    """The largest images features and the denoiser take (a float4 byte offset no longer fits 32 bits): the features of the first,
    middle and last rows and columns against the ray queries and denoise_ref.features_from_hits, and a 1-iteration pt_denoise on
    five windows against denoise_ref on crops 8 pixels wider on every side than the window (the filter reaches 4), nothing written
    outside any buffer.  About 24 GB of device memory."""
    state, obj, _ = box
    L = _L()
    n = w * h * 16
    need = 5 * n + (1 << 30)             # accumulation, two features, output, two denoise ping-pong buffers held by the context
    free = _free_device_bytes()
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB free" % (need / 1e9, free / 1e9))
    q = make_params(w, h, 1, 2, True, True)
    bufs = []
    try:
        for _ in range(4):
            bufs.append(Guarded(state.context, n))
        acc, alb, nd, out = bufs
        _launch(state.context, q, acc)
        assert L.pt_render_features(state.context, C.byref(q), alb.ptr, nd.ptr) == 0, L.pt_last_error(state.context)
        d = copy_params(q)
        d.accumulationBuffer = acc.ptr
        assert L.pt_denoise(state.context, C.byref(d), alb.ptr, nd.ptr, out.ptr, 1) == 0, L.pt_last_error(state.context)
        for b in bufs:
            b.check_guards()
        # features: rows 0, h/2, h-1 and columns 0, w/2, w-1
        for y in (0, h // 2, h - 1):
            a, b = alb.window(w, 0, y, w, 1)[0], nd.window(w, 0, y, w, 1)[0]
            _check_feature_pixels(state, obj, q, np.arange(w), np.full(w, y), a, b)
        for x in (0, w // 2, w - 1):
            a, b = alb.column(w, h, x)[:, 0], nd.column(w, h, x)[:, 0]
            _check_feature_pixels(state, obj, q, np.full(h, x), np.arange(h), a, b)
        # the denoiser on windows, against crops with a margin
        M, ww, hh = 8, 48, 24
        for x0, y0 in ((0, 0), (w - ww, 0), (0, h - hh), (w - ww, h - hh), (w // 2 - ww // 2, h // 2 - hh // 2)):
            cx0, cy0 = max(0, x0 - M), max(0, y0 - M)
            cx1, cy1 = min(w, x0 + ww + M), min(h, y0 + hh + M)
            crop = [b.window(w, cx0, cy0, cx1 - cx0, cy1 - cy0) for b in (acc, alb, nd)]
            assert not np.any(_bits(crop[0]) == SENT32) and not np.any(_bits(crop[1]) == SENT32)
            ref = dr.denoise(crop[0], crop[1], crop[2], 1)[y0 - cy0:y0 - cy0 + hh, x0 - cx0:x0 - cx0 + ww]
            got = out.window(w, x0, y0, ww, hh)
            bad = ~(np.abs(got - ref) <= np.maximum(1e-4 * np.abs(ref), 1e-5))
            assert not bad.any(), ((x0, y0), int(bad.sum()), got[bad][:4], ref[bad][:4])
        print("%dx%d: features and 1-iteration denoise checked; %.1f GB free before" % (w, h, free / 1e9))
    finally:
        for b in bufs:
            b.free()


def test_render_near_2_31_items(exact):
    """65535 x 16380 in 2 sample runs of 1 sample each: 8192 tile columns x 4095 strip rows x 32 x 2 = 2^31 - 2^19 work items, the most
    below the limit (a 2-frame batch of that size would be split by the scratch limit, so the second item bit comes from the runs).
    Rows 0, 1, the middle and the last two, and four corner blocks equal oracle_lib.render_window bit for bit; paths = 2 w h.  About
    35 GB of device memory (17 GB of accumulation, 17 GB of per-slot sums)."""
    state, sc = exact
    L = _L()
    w, h, spp = 65535, 16380, 2
    n = w * h * 16
    need = 2 * n + (1 << 30)
    free = _free_device_bytes()
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB free" % (need / 1e9, free / 1e9))
    p = make_params(w, h, spp, 1, True, True)
    acc = None
    try:
        assert L.pt_set_sample_chunks(state.context, 2) == 0
        acc = Guarded(state.context, n)
        st = _launch(state.context, p, acc)
        acc.check_guards()
        assert int(st.paths) == 2 * w * h and int(st.pixels) == w * h and int(st.sample_chunks) == 2
        print("65535x16380, 2^31 - 2^19 items: kernel %.0f ms, launch %.0f ms" % (st.kernel_ms, st.launch_ms))
        wins = [(0, 0, w, 2), (0, h // 2, w, 1), (0, h - 2, w, 2),
                (0, 2, 64, 8), (w - 64, 2, 64, 8), (0, h - 10, 64, 8), (w - 64, h - 10, 64, 8)]
        ref = np.zeros((h, w, 4), np.float32)           # calloc'd: only the windows' pages are ever touched
        for win in wins:
            oracle_lib.render_window(sc, copy_params(p), win, accumulation=ref, threads=THREADS, chunks=2)
        for x0, y0, ww, hh in wins:
            got = acc.window(w, x0, y0, ww, hh)
            want = ref[y0:y0 + hh, x0:x0 + ww]
            assert np.array_equal(_bits(got), _bits(want)), ((x0, y0, ww, hh), int((~np.all(_bits(got) == _bits(want), -1)).sum()))
        assert (ref[0:2, :, :3] > 0).any() or (ref[h // 2, :, :3] > 0).any()      # the windows see the emitter
    finally:
        L.pt_set_sample_chunks(state.context, 1)
        if acc is not None:
            acc.free()
