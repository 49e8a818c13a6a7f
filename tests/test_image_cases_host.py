"""The case generator of tests/image_cases.py is what it claims, the fp32 mirrors of the denoiser and the two blends agree with their
float64 evaluation and with the closed-form plane answers, and the rules for invalid inputs (include/acgpt.h) hold on the mirrors for
every hostile kind at every position.  No GPU.

fp32 against float64, measured over all valid cases (relative; the denoiser's with its 1e-5 absolute floor):
    denoiser 1.21e-5 (impulse, 48 x 40, 5 iterations), pt_temporal_blend 5.87e-6, pt_temporal_blend_motion 5.87e-6 (dolly, both).
The bounds asserted are 4 x these."""
import numpy as np
import pytest

import denoise_ref as dr
import image_cases as ic

MEASURED = {"denoise": 1.21e-5, "static": 5.87e-6, "motion": 5.87e-6}
F64_BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
# |fx - (x - k)| and |fy - (y - k)| of the closed-form cases in fp32 (footprint_fp32 against expected_footprint): 4.77e-7 and 2.39e-7.
# The accepted weight is a product and a sum of 1 - ax, ax, 1 - ay, ay, each rounded once more: |a - a_exact| <= 2 (dx + dy).
FX_DEV, FY_DEV = 4.77e-7, 2.39e-7
A_BOUND = 2.0 * (FX_DEV + FY_DEV)


# ---- the generator --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ic.SIZES)
def test_denoiser_cases_are_what_they_claim(w, h):
    j, n = ic._along(w, h)
    line = (lambda a: a[0, :]) if w >= h else (lambda a: a[:, 0])
    for kind in ic.DENOISE_KINDS:
        c = ic.denoise_case(kind, w, h)
        assert c["purpose"] and all(c[k].shape == (h, w, 4) and c[k].dtype == np.float32 for k in ("accum", "albedo", "nd"))
        assert np.isfinite(c["accum"]).all() and np.isfinite(c["nd"]).all() and np.isfinite(c["albedo"][..., :3]).all()
        hit = c["nd"][..., 3] >= 0
        length = np.sqrt((c["nd"][..., :3].astype(np.float64) ** 2).sum(axis=-1))
        assert np.abs(length[hit] - 1.0).max(initial=0.0) <= 2.0 ** -23, kind          # unit to 1 ulp
        again = ic.denoise_case.__wrapped__(kind, w, h)
        assert all(np.array_equal(again[k].view(np.uint32), c[k].view(np.uint32)) for k in ("accum", "albedo", "nd"))      # deterministic
    fan = ic.denoise_case("fan", w, h)["nd"].astype(np.float64)
    turn = np.degrees(np.arccos(np.clip((line(fan)[1:, :3] * line(fan)[:-1, :3]).sum(axis=-1), -1, 1)))
    want = np.array(ic.FAN_DEGREES)[np.minimum(np.arange(1, n) * 4 // n, 3)]
    assert np.abs(turn - want).max() <= 0.02, (turn, want)                  # arccos near 1 costs the 0.25 degree steps some digits
    assert set(np.round(want, 2)) == ({0.25, 1.0, 4.0, 16.0} if n >= 8 else set(np.round(want, 2)))
    t = line(ic.denoise_case("depth", w, h)["nd"])[:, 3].astype(np.float64)
    assert t.min() == np.float32(1e-3) and t.max() >= 1e6
    if n >= 40:
        assert set(np.floor(np.log10(t * 1.0000001)).astype(int)) == set(range(-3, 7))              # every decade
        step = np.abs(np.diff(t)) / t[:-1]
        for s in (0.001, 0.01, 0.1):
            assert (np.abs(step - s) < 0.02 * s).sum() >= 9, s
    chk = ic.denoise_case("checker", w, h)
    miss = ~(chk["nd"][..., 3] >= 0)
    assert miss.any() and (~miss).any() and np.all(chk["albedo"][miss, :3] != 0) and np.all(chk["nd"][miss, 1] == 1.0)
    alb = ic.denoise_case("albedo", w, h)["albedo"]
    if n >= 7:
        assert set(np.unique(alb[..., :3])) == set(np.array(ic.ALBEDO_VALUES, np.float32))
    flat = ic.denoise_case("flat", w, h)
    cv = dr.variance(flat["accum"], flat["albedo"], flat["nd"])
    assert np.all(cv[..., 3] == 0.0)                                        # exactly 0: lden is its 1e-6 floor
    imp, mixed = ic.denoise_case("impulse", w, h), ic.denoise_case("mixed", w, h)
    assert (imp["accum"][..., 0] == 1e4).sum() == 1
    assert dr.usable(mixed["accum"], mixed["albedo"], mixed["nd"]).all() and (mixed["nd"][..., 3] < 0).any() == (w * h >= 64)


def test_misses_ignore_their_albedo_and_normal():
    c = ic.denoise_case("checker", 33, 17)
    miss = ~(c["nd"][..., 3] >= 0)
    alb, nd = c["albedo"].copy(), c["nd"].copy()
    alb[miss, :3] = 0.0
    nd[miss, :3] = 0.0
    for it in (1, 3):
        assert np.array_equal(dr.denoise(c["accum"], alb, nd, it).view(np.uint32), ic.denoise_reference("checker", 33, 17)[it].view(np.uint32))


def test_blend_cases_are_what_they_claim():
    sc = ic.scene()
    assert [sc["bsdf"][sc[k]] for k in ("diffuse", "other", "metal", "glass")] == [0, 0, 1, 2]
    for kind in ic.BLEND_KINDS + ic.MOTION_KINDS:
        c = ic.blend_case(kind)
        assert c["purpose"] and max(c["w"], c["h"], c["wp"], c["hp"]) <= 64
        assert c["hist"].shape == (c["hp"], c["wp"], 4) and c["accum"].shape == (c["h"], c["w"], 4)
        assert (c["verts"] is not None) == (kind in ic.MOTION_KINDS)
        if c["verts"] is not None:
            assert c["verts"].shape == sc["verts"].shape == c["prev_verts"].shape
    ids = set(ic.blend_case("materials")["albedo"][..., 3].view(np.uint32).ravel().tolist())
    assert {sc["diffuse"], sc["metal"], sc["glass"], sc["n_tris"] + 5, 0xFFFFFFFF} <= ids
    assert set(ic.blend_case("counts")["hist"][..., 3].ravel().tolist()) == {0.0, -4.0, 1.0, 300.0, np.float32(1e30), 32.0}
    # the plane features are the plane: every hit point has z = -8
    c = ic.blend_case("identity")
    d = dr.pixel_rays(c["w"], c["h"], *c["camera"], dtype=np.float64)[:, 3:6].reshape(c["h"], c["w"], 3)
    assert np.abs(c["nd"][..., 3] * d[..., 2] + ic.DIST).max() <= 1e-6
    # the footprints of the closed-form cases are the shift, to the rounding recorded above
    for kind, shift in ic.CLOSED_FORM.items():
        if kind in ic.MOTION_KINDS:
            continue
        c = ic.blend_case(kind)
        (fx, fy), (ex, ey) = ic.footprint_fp32(c), ic.expected_footprint(c)
        assert np.abs(fx - ex).max() <= FX_DEV * 1.0001 and np.abs(fy - ey).max() <= FY_DEV * 1.0001, kind
    v = ic.blend_case("collapsed")
    i0, i1, _ = sc["idx"][v["prim"]]
    assert np.array_equal(v["verts"][i0], v["verts"][i1])


@pytest.mark.parametrize("position", ic.POSITIONS)
def test_the_planter_changes_only_what_it_names(position):
    c = ic.denoise_case("mixed", 48, 40)
    clean = {"rgb": c["accum"], "albedo": c["albedo"], "nd": c["nd"]}
    for kind in ic.HOSTILE_KINDS:
        got, px = ic.plant(clean, kind, position)
        assert px == ic.hostile_pixels(48, 40, position) and len(px) == {"corner": 1, "edge": 1, "interior": 1, "adjacent": 2, "row": 48}[position]
        changed = np.zeros((40, 48, 12), bool)
        for i, k in enumerate(("rgb", "albedo", "nd")):
            changed[..., 4 * i:4 * i + 4] = got[k].view(np.uint32) != clean[k].view(np.uint32)
        ys, xs, ch = np.nonzero(changed)
        assert set(zip(ys.tolist(), xs.tolist())) <= set(px) and len(set(ch.tolist())) in (1, 2, 3) and len(set((ch // 4).tolist())) == 1, kind
        assert changed.any(), kind
    for (w, h) in ic.SIZES:
        assert all(0 <= y < h and 0 <= x < w for p in ic.POSITIONS for (y, x) in ic.hostile_pixels(w, h, p))


# ---- fp32 against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,w,h", ic.denoise_cases())
def test_denoiser_mirror_against_float64(kind, w, h):
    c = ic.denoise_case(kind, w, h)
    r32, r64 = ic.denoise_reference(kind, w, h), ic.denoise_reference(kind, w, h, np.float64)
    for it in ic.ITERATIONS:
        assert r32[it].dtype == np.float32 and r64[it].dtype == np.float64 and np.isfinite(r64[it]).all()
        err = np.abs(r32[it] - r64[it])
        worst = np.where(err > 1e-5, err / np.abs(r64[it]), 0.0).max()
        print("%s %dx%d %d iterations: fp32 against float64 %.3e" % (kind, w, h, it, worst))
        assert np.all(err <= np.maximum(F64_BOUND["denoise"] * np.abs(r64[it]), 1e-5)), worst
    assert np.array_equal(dr.denoise(c["accum"], c["albedo"], c["nd"], 3).view(np.uint32), r32[3].view(np.uint32))       # the shared passes are denoise()


@pytest.mark.parametrize("kind", ic.BLEND_KINDS + ic.MOTION_KINDS)
def test_blend_mirrors_against_float64(kind):
    for cap in ic.CAPS:
        for form, gamma in ic.blend_forms(kind):
            (o32, t32), (o64, t64) = ic.blend_reference(kind, cap, form, gamma), ic.blend_reference(kind, cap, form, gamma, np.float64)
            assert np.array_equal(t32, t64), (cap, form, gamma)
            err = np.abs(o32 - o64)
            print("%s cap %g %s gamma %g: fp32 against float64 %.3e, %.2f take history" % (kind, cap, form, gamma, (err / np.abs(o64)).max(), t32.mean()))
            assert np.all(err <= F64_BOUND[form] * np.abs(o64)), (cap, form, gamma)
            if cap == 0.0 or kind in ic.PASS_THROUGH:
                assert not t32.any()
    if kind == "unmoved":
        for cap in ic.CAPS:
            a, b = ic.blend_reference(kind, cap, "motion", 0.0)[0], ic.blend_mirror(ic.blend_case(kind), cap, "static", 0.0)[0]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the closed form ------------------------------------------------------------------------------------------------------------------
def check_closed_form(out, case, cap, what):
    """A blend's output against what the shift alone says (image_cases.closed_form)."""
    rgb, wcount, took, a = ic.closed_form(case, cap)
    n = min(ic.COUNT, cap)
    assert np.array_equal(out[..., 3] != case["N"], took), what
    assert np.all(np.abs(out[..., 3] - wcount) <= n * A_BOUND + 2.0 ** -19), (what, np.abs(out[..., 3] - wcount).max())     # 2^-19: an ulp of n + N < 512
    # a tap that should weigh nothing weighs at most A_BOUND; it carries a neighbour's colour, and the blend itself rounds a few times
    tol = A_BOUND * 2.0 * float(case["hist"][..., :3].max()) + 4e-7 * np.abs(rgb)
    assert np.all(np.abs(out[..., :3] - rgb) <= tol), (what, np.abs(out[..., :3] - rgb).max())
    if not (np.array(case["shift"]) % 1).any():
        assert np.all(np.abs(a[took] - 1.0) == 0.0)             # an integer shift: one previous pixel, a = 1


@pytest.mark.parametrize("kind", sorted(ic.CLOSED_FORM))
def test_closed_form_against_the_mirrors(kind):
    case = ic.blend_case(kind)
    for cap in ic.CAPS:
        for form, gamma in ic.blend_forms(kind):
            if gamma == 0.0:
                check_closed_form(ic.blend_reference(kind, cap, form, gamma)[0], case, cap, "%s cap %g %s" % (kind, cap, form))
    assert ic.closed_form(case, 256.0)[2].mean() > 0.5


@pytest.mark.parametrize("kind", ic.PASS_THROUGH)
def test_pass_through_cases(kind):
    c = ic.blend_case(kind)
    for form, gamma in ic.blend_forms(kind):
        out, took = ic.blend_reference(kind, 256.0, form, gamma)
        assert not took.any() and np.array_equal(out[..., :3].view(np.uint32), c["accum"][..., :3].view(np.uint32)) and np.all(out[..., 3] == c["N"])


# ---- invalid inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ic.DENOISE_HOSTILE_KINDS)
def test_denoiser_rules_on_the_mirror(kind):
    for position in ic.POSITIONS:
        for (size, its) in ic.DENOISE_HOSTILE_RUNS:
            accum, alb, nd, px = ic.denoise_hostile(kind, position, size)
            got = ic.denoise_all(accum, alb, nd, its)
            for it in its:
                ic.check_denoise_hostile(got[it], ic.denoise_reference("mixed", *size)[it], accum, alb, nd, px, it,
                                         "%s at %s, %dx%d, %d iterations" % (kind, position, *size, it))
    if kind in ("rgb_nan", "rgb_pinf", "rgb_ninf", "rgb_1e30", "rgb_3e38"):
        accum, alb, nd, px = ic.denoise_hostile(kind, "interior", (48, 40))
        assert not dr.usable(accum, alb, nd)[px[0]]                      # these are the unusable ones, so the pass-through was checked


@pytest.mark.parametrize("base,form,gamma", ic.BLEND_HOSTILE_BASES)
def test_blend_rules_on_the_mirrors(base, form, gamma):
    clean = ic.blend_reference(base, ic.HOSTILE_CAP, form, gamma)[0]
    for (b, f, g, kind, target, position) in ic.blend_hostile_runs():
        if (b, f, g) != (base, form, gamma):
            continue
        case, cur, prv = ic.blend_hostile(base, kind, target, position)
        out, _ = ic.blend_mirror(case, ic.HOSTILE_CAP, form, gamma)
        ic.check_blend_hostile(out, clean, case, cur, prv, gamma, "%s %s gamma %g: %s in %s at %s" % (base, form, gamma, kind, target, position))


def test_a_poisoned_history_heals_on_the_mirror():
    case = dict(ic.blend_case("identity"))
    chains = []
    for poison in (False, True):
        c = dict(case)
        if poison:
            c["hist"] = ic.plant({"rgb": case["hist"]}, "rgb_nan", "interior")[0]["rgb"]
        first, _ = ic.blend_mirror(c, 256.0, "static", 0.0)
        c["hist"] = first
        second, _ = ic.blend_mirror(c, 256.0, "static", 0.0)
        chains.append((first, second))
    (y, x), = ic.hostile_pixels(case["w"], case["h"], "interior")
    for clean, got in zip(*chains):
        assert np.isfinite(got).all()
        differs = (clean.view(np.uint32) != got.view(np.uint32)).any(axis=-1)
        differs[y, x] = False
        assert not differs.any()
