"""Environment maps wider and taller than one workgroup of the CDF scan (csrc/environment.hip env_block_scan: 256 threads, each owning
a run of ceil(n / 256) values), shared by tests/test_env_wide_host.py (oracle against env_ref.py, no GPU) and
tests/test_gpu_env_wide.py (the device against both).  Generated from fixed seeds; rgb float32 [h, w, 3]."""
import numpy as np

F = np.float32
U = 2.0 ** -24                      # one fp32 rounding, relative


def run_length(n, threads=256):
    return (n + threads - 1) // threads


def _uniform(h, w, seed, power=1):
    return (np.random.default_rng(seed).uniform(0.0, 1.0, (h, w, 3)) ** power).astype(F)


def _black_rows():
    img = _uniform(513, 3, 17)
    img[[0, 5, 6, 512]] = 0.0
    return img


def sun_map():
    """a sky of 0.2 with a 3 x 3-texel sun inside a run, past index 256 on both axes"""
    img = np.full((260, 300, 3), 0.2, F)
    img[130:133, 277:280] = (900.0, 800.0, 700.0)
    return img


def faint_sun_map(seed=23):
    """the sun over a sky of 1e-3 scale: past the sun a row's running sum is 4e7 times a sky texel, more than 2^24, so that the
    texels after it add nothing and the hand-over to the next run (a sum in another association) can step down"""
    img = (np.random.default_rng(seed).uniform(0.05, 1.0, (260, 300, 3)) * 1e-3).astype(F)
    img[130:133, 277:280] = (5e4, 4.5e4, 4e4)
    return img


def sparse_map(seed=29):
    """70 % of the texels are zero: long flat stretches of the tables, and run starts of zero weight"""
    r = np.random.default_rng(seed)
    img = r.uniform(0.0, 1.0, (260, 300, 3)).astype(F)
    img[r.uniform(size=(260, 300)) < 0.7] = 0.0
    return img


def one_texel_map():
    img = np.zeros((300, 260, 3), F)
    img[281, 259] = (3.0, 2.0, 1.0)
    return img


ONE_TEXEL = (281, 259)


def real_size_map(seed=31):
    """1024 x 2048 (h x w): a seeded sky at 0.2 scale with a 4 x 4-texel sun of 5e4"""
    img = (np.random.default_rng(seed).uniform(0.05, 1.0, (1024, 2048, 3)) * 0.2).astype(F)
    img[700:704, 1500:1504] = 5e4
    return img


def longest_map(shape):
    """(1, 16384) or (16384, 1): the largest width and height pt_set_environment accepts, runs of 64"""
    return np.random.default_rng(43).uniform(0.0, 1.0, tuple(shape) + (3,)).astype(F)


# (name, builder, uniform): uniform maps hold weights of one scale, where the tables come out sorted
CASES = [
    ("3x257 uniform", lambda: _uniform(3, 257, 11), True),            # run = 2, threads 129 .. 255 own nothing
    ("2x512 uniform", lambda: _uniform(2, 512, 12), True),            # an exact multiple of the workgroup
    ("2x513 uniform^4", lambda: _uniform(2, 513, 13, 4), False),      # run = 3, weights over many scales
    ("3x700 uniform", lambda: _uniform(3, 700, 14), True),            # run = 3
    ("257x4 uniform", lambda: _uniform(257, 4, 15), True),            # the marginal scan at run = 2
    ("300x2 uniform", lambda: _uniform(300, 2, 16), True),            # the marginal scan
    ("513x3 black rows", _black_rows, False),                         # the marginal scan over rows of zero total
    ("260x300 sun", sun_map, False),
    ("260x300 faint-sky sun", faint_sun_map, False),
    ("260x300 sparse", sparse_map, False),
    ("300x260 one texel", one_texel_map, False),
]
SAMPLED = ["260x300 sun", "260x300 faint-sky sun", "260x300 sparse", "300x260 one texel"]

_made = {}


def case(name):
    """the map of that name (built once, read-only)"""
    if name not in _made:
        img = next(c for c in CASES if c[0] == name)[1]()
        img.setflags(write=False)
        _made[name] = img
    return _made[name]


_refs = {}


def reference(name):
    """EnvRef of that map (built once, shared by the tests)"""
    from env_ref import EnvRef
    if name not in _refs:
        _refs[name] = EnvRef(case(name))
    return _refs[name]


# ---- checks both test files make ------------------------------------------------------------------------------------------------
def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_tables_equal(t, ref, what):
    """t: {texels [h, w, 4], conditional, marginal, total, pdf_scale}; ref: EnvRef or such a dict.  Every value bit for bit."""
    if not isinstance(ref, dict):
        ref = {"texels": np.concatenate([ref.rgb, ref.weight[..., None]], -1), "conditional": ref.cond, "marginal": ref.marg,
               "total": ref.total, "pdf_scale": ref.pdf_scale}
    assert t["texels"].shape == ref["texels"].shape, what
    assert np.array_equal(_u32(t["texels"][..., :3]), _u32(ref["texels"][..., :3])), what + ": rgb"
    bad = np.argwhere(_u32(t["texels"][..., 3]) != _u32(ref["texels"][..., 3]))
    assert len(bad) == 0, "%s: %d weights differ, the first at %s" % (what, len(bad), bad[0])
    bad = np.argwhere(_u32(t["conditional"]) != _u32(ref["conditional"]))
    assert len(bad) == 0, "%s: %d conditional entries differ, the first at %s" % (what, len(bad), bad[0])
    bad = np.argwhere(_u32(t["marginal"]) != _u32(ref["marginal"]))
    assert len(bad) == 0, "%s: %d marginal entries differ, the first at %s" % (what, len(bad), bad[0])
    assert _u32(t["total"]) == _u32(ref["total"]) and _u32(t["pdf_scale"]) == _u32(ref["pdf_scale"]), what + ": total, pdf_scale"


def check_samples(name, ref, u, s):
    """s = hook(2, u) of an implementation against EnvRef.sample, test_hook_matches_the_reference's tolerances and exclusions"""
    checked = 0
    for (u1, u2), got in zip(u, s):
        dr, pr, (row, col), (fv, fu) = ref.sample(float(u1), float(u2))
        if min(fv, 1 - fv, fu, 1 - fu) < 1e-3:
            continue
        assert np.allclose(got[:3], dr, atol=1e-5), (name, u1, u2, got, dr)
        assert abs(got[3] - pr) <= 1e-4 * pr, (name, u1, u2, got[3], pr)
        checked += 1
    assert checked > 3500, (name, checked)


def check_one_texel(ref, s):
    """total == weight: every sample lies in the lit texel, with pdf W H / (2 pi^2 sin theta)"""
    row, col = ref.texel(s[:, :3])
    assert np.all(row == ONE_TEXEL[0]) and np.all(col == ONE_TEXEL[1])
    d = s[:, :3].astype(np.float64)
    sin_theta = np.sqrt(1.0 - d[:, 1] ** 2)
    np.testing.assert_allclose(s[:, 3], ref.w * ref.h / (2.0 * np.pi ** 2 * sin_theta), rtol=1e-4)


def sample_inputs():
    return np.random.default_rng(2).uniform(size=(4000, 2)).astype(np.float32)


def check_pdf_of_samples(name, ref, pdf_hook, s):
    """The sample's pdf is the pdf of its direction: pdf_hook(directions) -> [n, 1], s = hook(2, u), away from texel edges, within 1e-4.
    Within 2.8 degrees of a pole (1 - |y| < 1.2e-3; rows 0 .. 3 and 256 .. 259 of 260) the fp32 y of the direction no longer holds
    sin(theta) to 1e-4: its rounding of 2^-24 enters (1 - y)(1 + y) relative to 1 - |y|.  There the bound is that rounding's,
    1.2e-7 / (1 - |y|), as in tests/test_environment_host.py."""
    far = ref.edge_distance(s[:, :3]) > 1e-4
    assert far.sum() > 3500, (name, far.sum())
    rel = np.abs(pdf_hook(s[far, :3])[:, 0].astype(np.float64) / s[far, 3] - 1.0)
    to_pole = 1.0 - np.abs(s[far, 1].astype(np.float64))
    print("%s: pdf of the sampled direction against the sample's pdf, %d samples (%d near a pole), largest relative difference %.2e away from the poles, %.2e near them"
          % (name, far.sum(), (to_pole < 1.2e-3).sum(), rel[to_pole >= 1.2e-3].max(), rel[to_pole < 1.2e-3].max() if (to_pole < 1.2e-3).any() else 0.0))
    assert np.all(rel < np.maximum(1e-4, 1.2e-7 / to_pole)), (name, rel.max())
