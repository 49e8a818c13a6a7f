"""pt_bloom on the GPU against tests/bloom_ref.py, bit for bit: out_rgba and the whole info record as uint32 bits with no tolerance, on
synthetic images of every shape the tiling and the pyramid can get wrong and on a rendered one; then the call's contract,
pathtracer.bloom / displayTransform(bloom=) and acgpt_main --bloom.  Every device buffer lies between the sentinel guard bands of
test_gpu_shapes.Guarded."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import bloom_ref as br
import display_ref as dr
from test_firefly_host import synthetic
from test_gpu_shapes import SENT, Guarded

pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
F = np.float32
# (w, h): one texel on every level, one partial tile, a tile less one, a full tile, tiles plus one in both orders, two tiles of level 1
# less and plus one source pixel, narrow images over many tiles, more than 65 535 tile rows on level 1, and a full-size frame (2040
# tiles on level 1, 8160 for the composite: more than the grid, so every workgroup strides)
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (5, 7), (15, 15), (16, 16), (17, 33), (33, 17), (31, 33), (32, 32), (33, 31), (65, 63), (4099, 3),
          (3, 4099), (1, 1048577), (1920, 1080)]
SETS = [dict(threshold=0.0, knee=0.0, clamp=0.0, spread=1.0, levels=8, intensity=0.5),
        dict(threshold=1.0, knee=0.5, clamp=50.0, spread=0.7, levels=5, intensity=0.25),
        dict(threshold=2.0, knee=0.0, clamp=0.0, spread=0.0, levels=1, intensity=1.0)]
CONSTANT = dict(threshold=0.0, knee=0.0, clamp=0.0, spread=1.0, levels=4, intensity=0.5)


def _L():
    return _native.hip()


@pytest.fixture(scope="module")
def ctx():
    c = C.c_void_p()
    assert _L().pt_create(C.byref(c), 0) == 0, _L().pt_last_error(None)
    yield c
    _L().pt_destroy(c)


def tame(img):
    """values near FLT_MAX come down to +-1e4: eight levels of them overflow where the image is one pixel wide, and the sign of the NaN
    that inf - inf then makes is the processor's choice, not the statement's"""
    rgb = img[..., :3]
    huge = np.isfinite(rgb) & (np.abs(rgb) > F(1e30))
    rgb[huge] = np.copysign(F(1e4), rgb[huge])
    return img


def image(w, h):
    """test_firefly_host.synthetic: a background of 0.25 .. 2, spikes up to 2^13, NaN, infinities, negatives, zeros, +-1e4, and a NaN
    with a payload in .w"""
    img = tame(synthetic(h, w, 7000 + 10 * w + h))
    img.setflags(write=False)
    return img


def c_params(p):
    p = br.params(**p)
    return _native.BloomParams(p["threshold"], p["knee"], p["clamp"], p["intensity"], p["spread"], int(p["levels"]))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    diff = g != w
    assert not diff.any(), "%s: %d values differ, first at %s: %s vs %s" % (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), np.asarray(got)[diff][:4], np.asarray(want)[diff][:4])


def assert_record(info, want, what):
    got = np.frombuffer(bytes(info), np.uint32)
    ref = br.info_bits(want)
    assert np.array_equal(got, ref), (what, got.tolist(), ref.tolist())


class Buffers:
    """src and out of one image size, guarded"""

    def __init__(self, ctx, w, h):
        self.ctx, self.w, self.h, self.n = ctx, w, h, w * h
        self.src, self.out = Guarded(ctx, self.n * 16), Guarded(ctx, self.n * 16)

    def call(self, p, info=True):
        """(out [h, w, 4], BloomInfo or None) after one call on a sentinel-filled out; both buffers' guard bands checked"""
        self.out.fill()
        inf = _native.BloomInfo()
        rc = _L().pt_bloom(self.ctx, self.src.ptr, self.w, self.h, C.byref(c_params(p)), self.out.ptr, C.byref(inf) if info else None)
        assert rc == 0, _L().pt_last_error(self.ctx)
        self.src.check_guards()
        return self.out.image(self.w, self.h), (inf if info else None)

    def free(self):
        self.src.free(); self.out.free()


# ---- bit identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_bits_equal_the_reference(ctx, w, h):
    """The three parameter sets, with the record; up to 65 x 63 also each set cut to one level, whose output holds level 1 alone: an
    error of the first kernel is not hidden behind the later levels.  From 64 pixels on the image must hold invalid, bright and dark
    pixels under the second set."""
    b = Buffers(ctx, w, h)
    try:
        src = image(w, h)
        b.src.put(src)
        for i, p in enumerate(SETS):
            what = "%dx%d set %d" % (w, h, i)
            want, ri, pyr = br.bloom(src, p)
            assert all(np.isfinite(e).all() for e in pyr["E"]), what           # no NaN is made on the way: the bits are the data's
            print("%s: levels %d bright %d invalid %d share %.4f" % (what, ri["levels"], ri["bright_pixels"], ri["invalid_pixels"], br.bright_share(ri)))
            assert ri["levels"] == len(br.levels_of(w, h, p["levels"]))
            if w * h >= 64 and i == 1:
                assert ri["invalid_pixels"] > 0 and 0 < ri["bright_pixels"] < w * h - ri["invalid_pixels"], what
            out, info = b.call(p)
            assert_bits(out, want, what)
            assert_record(info, ri, what)
            assert_bits(b.src.image(w, h), src, what + " src")
            if w * h <= 65 * 63 and p["levels"] > 1:
                one = dict(p, levels=1)
                want, ri, _ = br.bloom(src, one)
                out, info = b.call(one)
                assert_bits(out, want, what + ", one level")
                assert_record(info, ri, what + ", one level")
    finally:
        b.free()


def test_a_constant_image_is_exact(ctx):
    w, h = 40, 24
    b = Buffers(ctx, w, h)
    try:
        src = np.full((h, w, 4), 0.5, F)
        src.view(np.uint32)[..., 3] = (np.uint32(0x7FC00000) | np.arange(h * w, dtype=np.uint32).reshape(h, w))
        b.src.put(src)
        out, info = b.call(CONSTANT)
        assert info.levels == 4 and info.bright_pixels == w * h and info.invalid_pixels == 0
        assert np.all(out[..., :3] == F(0.75))
        assert np.array_equal(bits(out)[..., 3], bits(src)[..., 3])
        assert info.total_luma_q16 == info.bright_luma_q16 == w * h * int(float(br.lum(src[0, 0, :3])) * 65536.0)
    finally:
        b.free()


# ---- contract -----------------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_call_without_info_leave_a_clean_record(ctx):
    w, h = 53, 37
    b = Buffers(ctx, w, h)
    try:
        a0, a1 = image(w, h), tame(synthetic(h, w, 2))
        p = SETS[1]
        b.src.put(a0)
        first, i0 = b.call(p)
        second, i1 = b.call(p)
        assert_bits(second, first, "second call")
        assert bytes(i0) == bytes(i1)
        third, none = b.call(p, info=False)             # its counts must not leak into the next call's
        assert none is None
        assert_bits(third, first, "third call")
        b.src.put(a1)
        out, info = b.call(p)
        want, ri, _ = br.bloom(a1, p)
        assert_bits(out, want, "the next image")
        assert_record(info, ri, "the next image")
    finally:
        b.free()


def test_the_pyramid_grows_on_demand():
    """a context of its own: a small image first, then a large one, then the small one again, each against the reference"""
    c = C.c_void_p()
    assert _L().pt_create(C.byref(c), 0) == 0, _L().pt_last_error(None)
    try:
        for w, h in ((9, 7), (301, 203), (9, 7), (64, 300)):
            b = Buffers(c, w, h)
            try:
                src = image(w, h)
                b.src.put(src)
                want, ri, _ = br.bloom(src, SETS[0])
                out, info = b.call(SETS[0])
                assert_bits(out, want, "%dx%d" % (w, h))
                assert_record(info, ri, "%dx%d" % (w, h))
            finally:
                b.free()
    finally:
        _L().pt_destroy(c)


def test_refusals_launch_nothing_and_leave_the_context_usable(ctx):
    w, h = 37, 19
    n = w * h
    b = Buffers(ctx, w, h)
    L = _L()
    try:
        src = image(w, h)
        b.src.put(src)
        good = c_params(SETS[1])
        want, ri, _ = br.bloom(src, SETS[1])
        out, info = b.call(SETS[1])
        assert_bits(out, want, "before")
        nan, inf = float("nan"), float("inf")
        calls = [("null src", "null argument", (None, w, h, good, b.out.ptr)),
                 ("null params", "null argument", (b.src.ptr, w, h, None, b.out.ptr)),
                 ("null out", "null argument", (b.src.ptr, w, h, good, None)),
                 ("zero width", "width and height", (b.src.ptr, 0, h, good, b.out.ptr)),
                 ("zero height", "width and height", (b.src.ptr, w, 0, good, b.out.ptr)),
                 ("too many pixels", "too large", (b.src.ptr, 65536, 32769, good, b.out.ptr))]
        for name, kws in (("threshold", [dict(threshold=v, knee=0.0) for v in (-1.0, nan, inf)]), ("knee", [dict(knee=v) for v in (-0.5, 1.5, nan, inf)]),
                          ("clamp", [dict(clamp=v) for v in (-1.0, nan, inf)]), ("intensity", [dict(intensity=v) for v in (-0.1, nan, inf)]),
                          ("spread", [dict(spread=v) for v in (-0.1, 4.5, nan, inf)]), ("levels", [dict(levels=v) for v in (0, 9, 0xFFFFFFFF)])):
            for kw in kws:
                d = br.params(**dict(SETS[1], **kw))
                bad = _native.BloomParams(d["threshold"], d["knee"], d["clamp"], d["intensity"], d["spread"], int(d["levels"]))
                calls.append(("bad params %s" % kw, name, (b.src.ptr, w, h, bad, b.out.ptr)))
        calls += [("out is src", "out_rgba overlaps", (b.src.ptr, w, h, good, b.src.ptr)),
                  ("out overlaps src from above", "out_rgba overlaps", (b.src.ptr, w, h, good, b.src.ptr + 16 * (n - 1))),
                  ("out overlaps src from below", "out_rgba overlaps", (b.src.ptr + 16, w, h - 1, good, b.src.ptr))]
        for name, message, (s, ww, hh, bp, o) in calls:
            b.out.fill()
            rec = _native.BloomInfo()
            C.memset(C.byref(rec), SENT, C.sizeof(rec))
            rc = L.pt_bloom(ctx, s, ww, hh, C.byref(bp) if bp is not None else None, o, C.byref(rec))
            assert rc != 0, name
            msg = L.pt_last_error(ctx).decode()
            assert msg.startswith("pt_bloom: ") and message in msg, (name, msg)
            assert np.all(b.out.read() == SENT), name
            assert_bits(b.src.image(w, h), src, name + " src")
            assert bytes(rec) == bytes([SENT]) * C.sizeof(rec), name
        assert L.pt_bloom(None, b.src.ptr, w, h, C.byref(good), b.out.ptr, None) != 0
        assert b"null context" in L.pt_last_error(None)
        out, info = b.call(SETS[1])
        assert_bits(out, want, "after")
        assert_record(info, ri, "after")
    finally:
        b.free()


# ---- a rendered image -----------------------------------------------------------------------------------------------------------
E2E = dict(width=64, height=64, max_depth=8, spp=8, direct_lighting=True, importance_sampling=True)
CUSTOM = dict(threshold=0.75, knee=0.25, clamp=8.0, intensity=0.2, spread=0.5, levels=4)


@pytest.fixture(scope="module")
def rendered(gpu_state_factory):
    """the Cornell box, one 8-spp launch: the bloom and the display transform with and without it, through the Python layer"""
    state, _ = gpu_state_factory(BOX, **E2E)           # sample_chunks 1, IEEE arithmetic
    source_hash = _L().pt_kernel_source_hash().decode()
    pt.LaunchCurrentFrame(None, state)
    state.params.currentFrameIdx = 1
    out = dict(acc=pt.readAccumulation(state), stats=bytes(pt.getStats(state)))
    out["plain_before"], out["plain_info"] = pt.displayTransform(state)
    out["bloomed"], out["info"] = pt.bloom(state)
    out["custom"], out["custom_info"] = pt.bloom(state, **CUSTOM)
    out["uploaded"], _ = pt.bloom(state, image=out["acc"], **CUSTOM)
    out["display"], out["display_info"] = pt.displayTransform(state, bloom={})
    out["display_custom"], out["display_custom_info"] = pt.displayTransform(state, curve="reinhard", exposure=1.5, bloom=CUSTOM)
    out["plain_after"], _ = pt.displayTransform(state, bloom=None)
    out["acc_after"], out["stats_after"] = pt.readAccumulation(state), bytes(pt.getStats(state))
    out["hash"], out["hash_before"] = _L().pt_kernel_source_hash().decode(), source_hash
    # what the display transform makes of an uploaded image: the reference's bloom goes through the same device curve
    for name, p, kw in (("display", {}, {}), ("display_custom", CUSTOM, dict(curve="reinhard", exposure=1.5))):
        e = F(out[name + "_info"]["exposure"])
        d = br.params(**p)
        scaled = dict(d, threshold=F(d["threshold"]) / e, knee=F(d["knee"]) / e, clamp=F(d["clamp"]) / e)
        want, ri, _ = br.bloom(out["acc"], scaled)
        out[name + "_want_info"] = ri
        out[name + "_want"], _ = pt.displayTransform(state, image=want, exposure=float(e), **{k: v for k, v in kw.items() if k != "exposure"})
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def info_matches(got, want):
    for k in ("levels", "bright_pixels", "invalid_pixels", "total_luma_q16", "bright_luma_q16"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert F(got["max_luma"]).view(np.uint32) == F(want["max_luma"]).view(np.uint32)
    assert got["bright_share"] == br.bright_share(want)


def test_a_rendered_image_equals_the_reference(rendered):
    acc = rendered["acc"]
    want, ri, _ = br.bloom(acc)
    assert_bits(rendered["bloomed"], want, "the defaults on the accumulation")
    info_matches(rendered["info"], ri)
    assert ri["levels"] == 6 and 0 < ri["bright_pixels"] < 64 * 64
    want, ri, _ = br.bloom(acc, CUSTOM)
    assert_bits(rendered["custom"], want, "custom settings")
    assert_bits(rendered["uploaded"], want, "the same from an uploaded array")
    info_matches(rendered["custom_info"], ri)
    print("8 spp: defaults, %d bright pixels, bright share %.4f, max luminance %.2f" % (rendered["info"]["bright_pixels"], rendered["info"]["bright_share"], rendered["info"]["max_luma"]))


def test_the_call_leaves_the_render_state_alone(rendered):
    assert_bits(rendered["acc_after"], rendered["acc"], "the accumulation")
    assert rendered["stats_after"] == rendered["stats"]
    assert np.array_equal(rendered["plain_after"], rendered["plain_before"])          # bloom=None: today's bytes
    assert np.any(rendered["display"] != rendered["plain_before"])


def test_kernel_source_hash_is_the_parent_commit_s(rendered):
    """the value the library of the parent commit reports: bloom.hip, bloom.h and image_common.h are no render kernel sources"""
    assert rendered["hash"] == rendered["hash_before"] == _build.kernel_source_hash() == "0ae80f7fe3d9b38b"


def test_display_transform_with_bloom(rendered):
    """the bytes are the display transform of bloom_ref's output at the metered exposure; the exposure is that of the image without
    its glare"""
    plain = rendered["plain_info"]
    info = rendered["display_info"]
    assert info["exposure"] == plain["exposure"] and info["metered_pixels"] == plain["metered_pixels"]
    assert np.array_equal(info["histogram"], plain["histogram"])
    ref_info = dr.transform(rendered["acc"].reshape(-1, 4), dr.params())[1]
    assert F(info["exposure"]).view(np.uint32) == F(ref_info["exposure"]).view(np.uint32)
    assert np.array_equal(rendered["display"], rendered["display_want"])
    info_matches(info["bloom"], rendered["display_want_info"])
    assert np.array_equal(rendered["display_custom"], rendered["display_custom_want"])
    info_matches(rendered["display_custom_info"]["bloom"], rendered["display_custom_want_info"])
    assert rendered["display_custom_info"]["exposure"] == 1.5 and rendered["display_custom_info"]["metered_pixels"] == 0


def test_cli_blooms_what_it_shows(tmp_path, gpu_state_factory):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")

    def run(name, *extra):
        d = tmp_path / name
        d.mkdir()
        cmd = [exe, "--obj", BOX, "--width", "64", "--height", "64", "--spp-per-launch", "8", "--frames", "1", "--max-depth", "8", "--direct-lighting",
               "--importance-sampling", "--out", str(d / "f.png"), "--out-hdr", str(d / "f.pfm"), "--save-accum", str(d / "acc.bin")]
        r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout, {f: open(str(d / f), "rb").read() for f in sorted(os.listdir(str(d)))}

    out_a, files_a = run("a", "--tonemap", "aces", "--exposure", "auto")
    out_b, files_b = run("b", "--tonemap", "aces", "--exposure", "auto", "--bloom")
    assert "Bloom:" not in out_a and len([x for x in out_b.splitlines() if x.startswith("Bloom: ")]) == 1
    assert sorted(files_a) == sorted(files_b)
    assert files_a["f.png"] == files_b["f.png"] and files_a["acc.bin"] == files_b["acc.bin"]
    assert files_a["f_display.png"] != files_b["f_display.png"] and files_a["f.pfm"] != files_b["f.pfm"]
    # the same through the Python layer, on the accumulation the app rendered
    raw = pt.readPFM(str(tmp_path / "a" / "f.pfm"))[::-1]              # readPFM puts the top row first, the accumulation the bottom row
    acc = np.concatenate([raw[..., :3], np.ones(raw.shape[:2] + (1,), F)], axis=-1)
    state, _ = gpu_state_factory(BOX, **E2E)
    rgba, info = pt.displayTransform(state, image=acc, curve="aces", bloom={})
    pt.saveImage(str(tmp_path / "py.png"), rgba)
    assert (tmp_path / "py.png").read_bytes() == files_b["f_display.png"]
    line = [x for x in out_b.splitlines() if x.startswith("Bloom: ")][0]
    assert ("%d levels, %d bright, %d invalid" % (info["bloom"]["levels"], info["bloom"]["bright_pixels"], info["bloom"]["invalid_pixels"])) in line, line
    e = F(info["exposure"])
    d = br.params()
    want, _, _ = br.bloom(acc, dict(d, threshold=F(d["threshold"]) / e, knee=F(d["knee"]) / e, clamp=F(d["clamp"]) / e))
    shown = pt.readPFM(str(tmp_path / "b" / "f.pfm"))[::-1]
    assert_bits(shown[..., :3], want[..., :3], "--out-hdr")
    out_c, files_c = run("c", "--tonemap", "linear", "--exposure", "1", "--bloom", "0.5,0.3,3,0.5")
    assert "Bloom: 3 levels" in out_c
    r = subprocess.run([exe, "--obj", BOX, "--bloom"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--bloom" in r.stderr
    r = subprocess.run([exe, "--obj", BOX, "--tonemap", "aces", "--bloom", "1,0.1,9"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--bloom" in r.stderr
