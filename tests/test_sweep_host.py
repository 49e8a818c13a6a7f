"""pt_query_sweep without a GPU: the NumPy statement of the time of impact (tests/sweep_ref.py) on hand-checked sweeps, against its own
float64 evaluation on the Cornell box, against a bisection that knows nothing of the decomposition, the feature coverage of the
"aimed" set, the tie rule, radius 0 against the ray queries, the sweeps that are a miss before any traversal, the interface (symbols,
record size, no scratch memory in the kernels) and the argument checks of querySweep that need no device."""
import os
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import nearest_ref as nr
import query_ref as qr
import sweep_ref as sw

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = os.path.join(pt.SCENES, "cornell_box.obj")

# Measured once on the CPU on the sets "camera", "aimed" and "short" of the Cornell box (scene units, the box is 556 wide; DESIGN.md
# section 28 quotes both), and what the test holds the fp32 statement to, four times each:
#   CONTACT  the largest float64 | dist(o + d * t32, winning triangle) - r | over the sweeps fp32 and float64 both call hits, t32 > 0;
#   BAND     the largest float64 | closest approach of the centre line's piece to the deciding triangle - r | over the sweeps the two
#            call differently (all of them in "short", at tmax = 1 x t, where the piece ends on the contact).
CONTACT_MEASURED = 1.85e-4
BAND_MEASURED = 1.85e-4
CONTACT_BOUND = 4.0 * CONTACT_MEASURED
BAND = 4.0 * BAND_MEASURED
BAND_SHARE = 0.01               # a condition, not a measurement: at most this share of "camera" and of "aimed" lies in the band

TRI = (np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32), np.array([0, 1, 2], np.uint32))


def _one(sweep, verts=TRI[0], idx=TRI[1], mats=(0x05000007,)):
    rec, kind = sw.sweep_records(np.array([sweep], np.float32), verts, idx, np.array(mats, np.uint32), kinds=True)
    return rec[0], rec.view(np.float32)[0], int(kind[0])


def test_hand_checked_sweeps_of_one_triangle():
    """A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0); every value below is exact in fp32"""
    inf = np.inf
    cases = [
        # o, d, r, tmax -> t, kind, (u, v), contact point
        ((1, 1, 5), (0, 0, -1), 1.0, inf, 4.0, sw.FACE, (0.25, 0.25), (1, 1, 0)),             # down onto the face
        ((1, 1, -5), (0, 0, 2), 1.0, inf, 2.0, sw.FACE, (0.25, 0.25), (1, 1, 0)),             # up from below, d of length 2
        ((2, -5, 0), (0, 1, 0), 1.0, inf, 4.0, sw.EDGE, (0.5, 0.0), (2, 0, 0)),               # in the plane, against edge AB
        ((-5, 2, 0), (1, 0, 0), 1.0, inf, 4.0, sw.EDGE, (0.0, 0.5), (0, 2, 0)),               # against edge AC
        ((-5, 0, 0), (1, 0, 0), 1.0, inf, 4.0, sw.VERTEX, (0.0, 0.0), (0, 0, 0)),             # against A, along AB's line
        ((9, 0, 0), (-1, 0, 0), 2.0, inf, 3.0, sw.VERTEX, (1.0, 0.0), (4, 0, 0)),             # against B
        ((1, 1, 0.5), (0, 0, -1), 1.0, inf, 0.0, sw.START, (0.25, 0.25), (1, 1, 0)),          # starts in contact
        ((1, 1, 5), (0, 0, -1), 0.0, inf, 5.0, sw.FACE, (0.25, 0.25), (1, 1, 0)),             # radius 0: a ray
        ((1, 1, 5), (0, 0, -1), 1.0, 4.0, 4.0, sw.FACE, (0.25, 0.25), (1, 1, 0)),             # tmax on the contact: the interval is closed
    ]
    for o, d, r, tmax, t, kind, uv, c in cases:
        u32, f, k = _one(o + d + (r, tmax))
        assert f[0] == F(t) and k == kind, (o, d, f[0], k)
        assert u32[1] == 0 and u32[7] == 7, o                    # the material id without the flags above bit 24
        assert (f[2], f[3]) == uv and tuple(f[4:7]) == c, (o, d, f[2:7])
    misses = [((1, 1, 5), (0, 0, -1), 1.0, 3.5), ((1, 1, 5), (0, 0, 1), 1.0, inf), ((9, 9, 5), (0, 0, -1), 1.0, inf), ((1, 1, 5), (0, 0, 0), 1.0, inf)]
    for o, d, r, tmax in misses:
        u32, f, k = _one(o + d + (r, tmax))
        assert np.array_equal(u32, sw.miss_records(1)[0]) and k == sw.NONE, (o, d)
    assert _one((1, 1, 0.5, 0, 0, 0, 1.0, 0.0))[1][0] == 0.0     # d = 0 and tmax = 0: the start overlap answers
    assert pt.SWEEP_DTYPE.itemsize == 32 and [pt.SWEEP_DTYPE.fields[k][1] for k in pt.SWEEP_DTYPE.names] == [0, 4, 8, 12, 16, 28]
    assert np.array_equal(sw.miss_records(1)[0], np.array([0xBF800000, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0xFFFFFFFF], np.uint32))


@pytest.fixture(scope="module")
def cornell():
    obj = pt.TinyObjWrapper(BOX)
    cam = pt.initCamera()
    cam.setAspectRatio(np.float32(97) / np.float32(61))
    camera = (cam.eye(),) + tuple(cam.UVWFrame())
    verts, idx, mats = obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices()
    return verts, idx, mats, camera


@pytest.fixture(scope="module")
def cornell_sets(cornell):
    """name -> (sweeps, records, kinds) of the three sets of (a) by the fp32 brute force: computed once, shared, never written"""
    verts, idx, mats, camera = cornell
    out = {}
    for name in ("camera", "aimed", "short"):
        s = sw.sweep_set(name, verts, idx, camera, mats)
        rec, kind = sw.sweep_records(s, verts, idx, mats, kinds=True)
        for a in (s, rec, kind):
            a.setflags(write=False)
        out[name] = (s, rec, kind)
    return out


def _f64_answers(s, v0, e1, e2):
    """(t, prim) of the float64 statement by brute force, +inf / -1 on a miss"""
    s64 = s.astype(np.float64)
    a, b, c = (x.astype(np.float64)[None] for x in (v0, e1, e2))
    t_out, p_out = np.full(s.shape[0], np.inf), np.full(s.shape[0], -1, np.int64)
    for start in range(0, s.shape[0], 128):
        sl = slice(start, start + 128)
        t = sw.sweep_triangle(s64[sl, None, 0:3], s64[sl, None, 3:6], s64[sl, 6, None], a, b, c)[0]
        t = np.where(t <= s64[sl, 7, None], t, np.inf)
        p = t.argmin(axis=1)
        t_out[sl] = t[np.arange(p.size), p]
        p_out[sl] = np.where(np.isfinite(t_out[sl]), p, -1)
    return t_out, p_out


@pytest.mark.parametrize("name", ["camera", "aimed", "short"])
def test_fp32_statement_against_its_float64_evaluation(cornell, cornell_sets, name):
    """(a) of the issue.  A sweep "falls in the band" when the float64 closest approach of its centre line's piece [0, tmax] to its
    deciding triangle — fp32's winner, else float64's — is within BAND of r; hit / miss may differ only there.  The share of a set in the
    band is counted over its sweeps with r > 0: with r = 0 (a fifth of "camera", as the set is defined) every hit is a line through
    its triangle, closest approach 0 = r, in the band by construction and no graze."""
    verts, idx, mats, camera = cornell
    s, rec, kind = cornell_sets[name]
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    t32, p32 = rec[:, 0].view(np.float32), rec[:, 1].astype(np.int64)
    t64, p64 = _f64_answers(s, v0, e1, e2)
    hit32, hit64 = t32 >= 0, np.isfinite(t64)
    assert hit32.mean() >= 0.25 and hit64.mean() >= 0.25
    # the contact of the common hits
    both = hit32 & hit64 & (t32 > 0)
    w = p32[both]
    s64 = s.astype(np.float64)
    centre = s64[both, 0:3] + s64[both, 3:6] * t32[both, None].astype(np.float64)
    a = v0[w].astype(np.float64)
    dist = nr.closest_f64(centre, a, a + e1[w], a + e2[w])[0]
    contact = np.abs(dist - s64[both, 6]).max()
    # the band: every sweep with a deciding triangle
    decided = hit32 | hit64
    w = np.where(hit32, p32, p64)[decided]
    approach = sw.line_distance_f64(s[decided], v0[w], e1[w], e2[w])
    off = np.abs(approach - s64[decided, 6])
    differ = (hit32 != hit64)[decided]
    band_seen = off[differ].max() if differ.any() else 0.0
    in_band = ((off <= BAND) & (s64[decided, 6] > 0)).sum() / s.shape[0]
    print("%s: %d common hits, largest |dist - r| %.3e (bound %.3e); %d sweeps decided differently, largest |approach - r| %.3e (band %.3e); "
          "%.4f of the set in the band" % (name, both.sum(), contact, CONTACT_BOUND, differ.sum(), band_seen, BAND, in_band))
    assert both.sum() >= 200
    assert contact <= CONTACT_BOUND
    assert band_seen <= BAND
    if name != "short":             # a third of "short" ends on its contact by construction
        assert in_band <= BAND_SHARE
    else:
        assert differ.any()         # the band is measured on something


def test_measured_figures_are_this_codes(cornell, cornell_sets):
    """The constants quoted above are the maxima over the three sets, not stale ones: within a factor 2 below what the sets give now"""
    verts, idx, mats, camera = cornell
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    contact, band = 0.0, 0.0
    for name, (s, rec, kind) in cornell_sets.items():
        t32, p32 = rec[:, 0].view(np.float32), rec[:, 1].astype(np.int64)
        t64, p64 = _f64_answers(s, v0, e1, e2)
        hit32, hit64 = t32 >= 0, np.isfinite(t64)
        both = hit32 & hit64 & (t32 > 0)
        s64 = s.astype(np.float64)
        a = v0[p32[both]].astype(np.float64)
        centre = s64[both, 0:3] + s64[both, 3:6] * t32[both, None].astype(np.float64)
        contact = max(contact, np.abs(nr.closest_f64(centre, a, a + e1[p32[both]], a + e2[p32[both]])[0] - s64[both, 6]).max())
        differ = hit32 != hit64
        if differ.any():
            w = np.where(hit32, p32, p64)[differ]
            band = max(band, np.abs(sw.line_distance_f64(s[differ], v0[w], e1[w], e2[w]) - s64[differ, 6]).max())
    print("largest contact deviation %.3e (quoted %.3e), largest band %.3e (quoted %.3e)" % (contact, CONTACT_MEASURED, band, BAND_MEASURED))
    assert CONTACT_MEASURED / 2.0 <= contact <= CONTACT_MEASURED * 1.05
    assert BAND_MEASURED / 2.0 <= band <= BAND_MEASURED * 1.05


def _random_pairs(n=2000, seed=29, drawn=2200):
    """Random triangles of edge ~2 around points up to 10 from the origin (area at least 0.1), each with a sphere of radius 0.01 .. 1.5
    that starts 2 .. 12 away (a tenth within its radius of the target) and is aimed at a point within 2 radii of a random point of the triangle: hits through every kind of
    feature and near misses"""
    rng = np.random.default_rng(seed)
    n, wanted = drawn, n
    centre = rng.uniform(-10.0, 10.0, (n, 3))
    v = [(centre + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32) for _ in range(3)]
    b = rng.random((n, 2)); fold = b.sum(axis=1) > 1.0; b[fold] = 1.0 - b[fold]
    r = rng.uniform(0.01, 1.5, n)
    target = v[0] + b[:, 0:1] * (v[1].astype(np.float64) - v[0]) + b[:, 1:2] * (v[2].astype(np.float64) - v[0]) + sw._unit(rng, n) * (r * rng.uniform(0.0, 2.0, n))[:, None]
    away = np.where(rng.random(n) < 0.1, r * rng.uniform(0.0, 1.0, n), rng.uniform(2.0, 12.0, n))          # a tenth start near the target: overlaps
    o = target + sw._unit(rng, n) * away[:, None]
    d = target - o
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    s = sw._pack(o, d, r, np.inf)
    nrm = np.cross(v[1].astype(np.float64) - v[0], v[2].astype(np.float64) - v[0])
    keep = np.flatnonzero(np.linalg.norm(nrm, axis=1) >= 0.2)[:wanted]
    return s[keep], v[0][keep], (v[1] - v[0])[keep], (v[2] - v[0])[keep]


def test_float64_statement_against_an_independent_bisection():
    """(b) of the issue: the decomposition is the geometric truth.  The distance from a point of the line to the triangle is convex
    along the line, so dist <= r holds on one interval; its lower end by bisection on closest_f64 knows nothing of spheres, cylinders
    and offset planes.  1e-6 relative to the larger of t and 1 (|d| = 1, triangles of size ~1)."""
    s, v0, e1, e2 = _random_pairs()
    assert s.shape[0] == 2000
    t, kind = sw.sweep_triangle(*(x.astype(np.float64) for x in (s[:, 0:3], s[:, 3:6])), s[:, 6].astype(np.float64), *(x.astype(np.float64) for x in (v0, e1, e2)))
    tb = sw.bisect_impact_f64(s, v0, e1, e2)
    hit, hit_b = np.isfinite(t), np.isfinite(tb)
    for k in (sw.START, sw.VERTEX, sw.EDGE, sw.FACE, sw.NONE):
        assert (kind == k).mean() >= 0.02, (k, (kind == k).mean())
    # the two may call a sweep differently only on a graze: the closest approach within 1e-9 of r
    differ = hit != hit_b
    if differ.any():
        graze = np.abs(sw.line_distance_f64(s[differ], v0[differ], e1[differ], e2[differ], iters=200) - s[differ, 6].astype(np.float64))
        assert (graze <= 1e-9).all(), graze.max()
    both = hit & hit_b
    assert both.mean() >= 0.3
    err = np.abs(t[both] - tb[both]) / np.maximum(t[both], 1.0)
    print("largest relative |t - bisection| over %d hits: %.3e" % (both.sum(), err.max()))
    assert err.max() <= 1e-6
    # and float64 leaves the sphere touching: the statement's own claim, within 1e-9
    moving = both & (t > 0)
    c = s[moving, 0:3].astype(np.float64) + s[moving, 3:6].astype(np.float64) * t[moving, None]
    a = v0[moving].astype(np.float64)
    assert np.abs(nr.closest_f64(c, a, a + e1[moving], a + e2[moving])[0] - s[moving, 6]).max() <= 1e-9


def test_every_kind_of_feature_wins_its_share_of_aimed(cornell_sets):
    s, rec, kind = cornell_sets["aimed"]
    shares = {k: float((kind == k).mean()) for k in (sw.START, sw.VERTEX, sw.EDGE, sw.FACE)}
    print("aimed: start overlap %.3f, vertex %.3f, edge %.3f, face %.3f" % tuple(shares[k] for k in (sw.START, sw.VERTEX, sw.EDGE, sw.FACE)))
    assert all(v >= 0.05 for v in shares.values()), shares
    assert np.unique(rec[:, 1]).size >= 64


def test_ties_go_to_the_lowest_triangle_index():
    """Two copies of one triangle: every time of impact is the same bits.  Whichever copy the index buffer lists first is triangle 0 and wins."""
    verts = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1], [0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32)
    sweeps = np.array([[1, 1, 5, 0.1, 0.2, -1, 0.7, np.inf], [2, -5, 0.3, 0, 1, 0, 1.0, np.inf], [-5, -4, 1, 1, 0.8, -0.2, 0.5, np.inf]], np.float32)
    for idx in (np.array([0, 1, 2, 3, 4, 5], np.uint32), np.array([3, 4, 5, 0, 1, 2], np.uint32)):
        v0, e1, e2 = nr.records_of_scene(verts, idx)
        t = sw.sweep_triangle(sweeps[:, None, 0:3], sweeps[:, None, 3:6], sweeps[:, 6, None], v0[None], e1[None], e2[None])[0]
        assert np.array_equal(t[:, 0].view(np.uint32), t[:, 1].view(np.uint32)) and np.isfinite(t).all()
        rec = sw.sweep_records(sweeps, verts, idx, np.array([3, 4], np.uint32))
        assert (rec[:, 1] == 0).all() and (rec[:, 7] == 3).all()


def test_radius_zero_is_the_ray_query(cornell):
    """Generic camera rays with radius 0: the same triangle as the closest hit of the ray queries with tmin = 0, wherever that hit's
    barycentrics are at least 1e-3 from an edge"""
    import denoise_ref as dr
    verts, idx, mats, camera = cornell
    rng = np.random.default_rng(77)
    rays = dr.pixel_rays(97, 61, *camera)[np.sort(rng.permutation(97 * 61)[:600])].copy()
    rays[:, 6], rays[:, 7] = 0.0, np.inf
    t, prim = nr.ray_first_hits(np.where(np.isinf(rays), 1e30, rays), verts, idx)
    hits = qr.hit_records(rays, t, prim, verts, idx, mats)
    u, v = hits[:, 2].view(np.float32), hits[:, 3].view(np.float32)
    inner = (prim != 0xFFFFFFFF) & (u >= 1e-3) & (v >= 1e-3) & (u + v <= 1.0 - 1e-3)
    assert inner.sum() >= 300
    rec = sw.sweep_records(sw._pack(rays[:, 0:3], rays[:, 3:6], 0.0, np.inf), verts, idx, mats)
    assert np.array_equal(rec[inner, 1], prim[inner])
    assert np.abs(rec[inner, 0].view(np.float32) - t[inner]).max() <= 1e-3 * float(np.abs(t[inner]).max())
    assert (rec[prim == 0xFFFFFFFF, 1] == 0xFFFFFFFF).mean() >= 0.9         # what the ray misses a point does not find, but for a graze of an edge


def test_sweeps_that_miss_before_any_traversal():
    good = np.array([1, 1, 5, 0, 0, -1, 1.0, 10.0], np.float32)
    bad, why = sw.bad_sweeps(good)
    assert bad.shape[0] == 18 + 5 + 4
    ok = sw.castable(bad)
    assert not ok.any(), [w for w, k in zip(why, ok) if k]
    assert np.array_equal(sw.sweep_records(bad, TRI[0], TRI[1], np.zeros(1, np.uint32)), sw.miss_records(bad.shape[0]))
    allowed = np.array([good, good, good, good], np.float32)
    allowed[1, 7] = np.inf
    allowed[2, 6] = -0.0                 # a radius of zero, whatever its sign bit
    allowed[3, 3:6] = 0.0                # d = 0 is a sweep: it misses by the test, not before it
    assert sw.castable(allowed).all()
    rec = sw.sweep_records(allowed, TRI[0], TRI[1], np.zeros(1, np.uint32))
    assert (rec[:3, 1] == 0).all() and rec[3, 1] == 0xFFFFFFFF
    assert np.array_equal(sw.sweep_records(allowed, TRI[0], np.zeros(0, np.uint32), np.zeros(0, np.uint32)), sw.miss_records(4))
    # the set of the GPU tests holds every case, and a third of it is bad
    s = sw.sweep_set("bad", TRI[0], TRI[1])
    assert (~sw.castable(s)).sum() == len(range(1, sw.SET_SIZE, 3))


def test_sets_are_what_they_say(cornell):
    verts, idx, mats, camera = cornell
    lo, hi = nr.scene_box(verts, idx)
    for name in sw.SWEEP_SETS:
        s = sw.sweep_set(name, verts, idx, camera, mats)
        assert s.shape == (sw.SET_SIZE, 8) and s.dtype == np.float32, name
        assert np.array_equal(s.view(np.uint32), sw.sweep_set(name, verts, idx, camera, mats).view(np.uint32)), name          # fixed seeds
        if name != "bad":
            assert sw.castable(s).all(), name
    rec, kind = sw.sweep_records(sw.sweep_set("inside", verts, idx), verts, idx, mats, kinds=True)
    assert (rec[:, 0] == 0).all() and (kind == sw.START).all()
    s = sw.sweep_set("zero_d", verts, idx)
    t = sw.sweep_records(s, verts, idx, mats)[:, 0].view(np.float32)
    assert (s[:, 3:6] == 0).all() and np.isin(t, (0.0, -1.0)).all() and 0.2 <= (t == 0).mean() <= 0.8
    s = sw.sweep_set("outside", verts, idx)
    assert ((s[:, 0:3] < lo) | (s[:, 0:3] > hi)).any(axis=1).all()
    t = sw.sweep_records(s, verts, idx, mats)[:, 0].view(np.float32)
    assert (t > 0).mean() >= 0.25 and (t < 0).mean() >= 0.2 and not (t == 0).any()
    s = sw.sweep_set("short", verts, idx, camera, mats)
    t = sw.sweep_records(s, verts, idx, mats)[:, 0].view(np.float32)
    assert (t >= 0).mean() >= 0.25 and (t < 0).mean() >= 0.25
    on_the_end = (t == s[:, 7])
    assert on_the_end.mean() >= 0.1                     # tmax = 1 x t: the closed end of the interval decides
    s = sw.sweep_set("grazing", verts, idx)
    rec, kind = sw.sweep_records(s, verts, idx, mats, kinds=True)
    assert (kind == sw.EDGE).mean() >= 0.05 and np.unique(rec[:, 1]).size >= 64


def test_build_lists_and_abi():
    assert "sweep.hip" in _build.HIP_SOURCES and "sweep.h" in _build.HIP_HEADERS
    for name in ("sweep.hip", "sweep.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    for name in ("pt_query_sweep", "pt_query_sweep_any"):
        assert name in _native.ABI_SYMBOLS
    assert "pt_debug_sweep_visits" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert "typedef struct { float t; uint32_t prim; float u, v; float cx, cy, cz; uint32_t material; } pt_sweep_hit;" in hdr
    assert "int pt_query_sweep(pt_ctx* ctx, const float* sweeps, size_t n, pt_sweep_hit* hits);" in hdr
    assert "int pt_query_sweep_any(pt_ctx* ctx, const float* sweeps, size_t n, uint8_t* blocked);" in hdr
    assert "int pt_debug_sweep_visits(pt_ctx* ctx, const float* sweeps, size_t n, pt_sweep_hit* hits, uint32_t* visits);" in open(os.path.join(ROOT, "include", "acgpt_test.h")).read()
    assert "static_assert(sizeof(pt_sweep_hit) == 32" in open(os.path.join(_build.CSRC, "capi_query.hip")).read()


def test_symbols_are_exported_and_bound(built):
    L = _native.hip()
    for name in ("pt_query_sweep", "pt_query_sweep_any", "pt_debug_sweep_visits"):
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (5 if name == "pt_debug_sweep_visits" else 4), name
    assert L.pt_abi_version() == 4
    assert L.pt_query_sweep(None, None, 0, None) != 0                     # a null context is refused before anything else


def test_sweep_kernels_use_no_scratch_memory(built):
    """The four k_query_sweep instantiations (two node formats, each with its counting twin) and the any-hit kernels beside them: no
    private segment, no spilled register — the eight features and the walk's best candidate fit the register file."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_query_sweep" in k["name"]]
    main = [k for k in rows if "k_query_sweep<" in k["name"]]
    assert len(main) == 4 and len(rows) == 6, [k["name"] for k in rows]
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] <= 128, k                    # four waves per SIMD at the least


def test_querysweep_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    for bad in (np.zeros((4, 5), np.float32), np.zeros(8, np.float32), np.zeros((2, 8, 1), np.float32), [[1, 2]]):
        with pytest.raises(pt.PathTracerError, match="expected an"):
            pt.querySweep(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.querySweep(state, np.zeros((2, 8), np.complex64))
    o, d = np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32)
    with pytest.raises(pt.PathTracerError, match="need a radius"):
        pt.querySweep(state, o, d)
    with pytest.raises(pt.PathTracerError, match="as many directions"):
        pt.querySweep(state, o, np.ones((3, 3), np.float32), radius=1.0)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, 2.0, 3.0]):
        with pytest.raises(pt.PathTracerError, match="radius"):
            pt.querySweep(state, o, d, radius=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(pt.PathTracerError, match="tmax"):
            pt.querySweep(state, o, d, radius=1.0, tmax=bad)
    with pytest.raises(pt.PathTracerError, match="seventh column"):
        pt.querySweep(state, np.zeros((2, 8), np.float32), radius=1.0)
    empty = pt.querySweep(state, np.zeros((0, 8), np.float32))
    assert sorted(empty) == ["material", "point", "prim", "t", "u", "v"]
    assert empty["t"].shape == (0,) and empty["point"].shape == (0, 3) and empty["prim"].dtype == np.uint32
    assert pt.querySweep(state, np.zeros((0, 3)), np.zeros((0, 3)), radius=1.0, any_hit=True).shape == (0,)
    torch = pytest.importorskip("torch")
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.querySweep(state, torch.zeros((4, 8), dtype=torch.float32))


def test_sweep_contacts():
    sweeps = np.array([[1, 1, 5, 0, 0, -1, 1.0, np.inf], [1, 1, 0.5, 0, 0, -1, 1.0, np.inf], [9, 9, 5, 0, 0, -1, 1.0, np.inf], [2, -5, 0, 0, 2, 0, 1.0, np.inf]], np.float32)
    rec = sw.sweep_records(sweeps, TRI[0], TRI[1], np.zeros(1, np.uint32)).view(np.float32)
    result = {"t": rec[:, 0].copy(), "point": rec[:, 4:7].copy()}
    centre, normal, start = pt.sweepContacts(result, sweeps)
    assert np.array_equal(centre[0], [1, 1, 1]) and np.array_equal(normal[0], [0, 0, 1]) and not start[0]
    assert np.array_equal(centre[1], [1, 1, 0.5]) and np.array_equal(normal[1], [0, 0, 1]) and start[1]
    assert np.isnan(centre[2]).all() and np.isnan(normal[2]).all() and not start[2]
    assert np.array_equal(centre[3], [2, -1, 0]) and np.array_equal(normal[3], [0, -1, 0])
    with pytest.raises(pt.PathTracerError, match="expected the"):
        pt.sweepContacts(result, sweeps[:, :7])
