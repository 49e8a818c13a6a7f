"""Case generator of tests/test_gpu_small_slab.py: the ray / box cases of test_gpu_golden.test_gpu_fp16_slab_is_conservative (a copy of
its generator, so that the two can move apart), as 19-float records of pt_selftest ops 41 / 42 / 43: ray o xyz, d xyz, box lo xyz, hi xyz,
scene centre xyz, inv_scale xyz, tmax.  Plain NumPy: no GPU, no library."""
import numpy as np

CENTRE = np.array([100.0, -50.0, 30.0], np.float32)
H = np.float32(300.0)
SQUEEZE = np.array([1.0, 0.313881, 1.0 / 40.0], np.float32)      # y: the lower face lands between two fp16 values under x's scale
FLATTEN = np.array([1.0, 0.5, 0.0], np.float32)


def exact_slab(o, d, lo, hi, tmin, tmax):
    """Ray / box in float64 on the very fp32 values the device gets: True where the ray meets the box within [tmin, tmax]."""
    o, d, lo, hi = (x.astype(np.float64) for x in (o, d, lo, hi))
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    par = d == 0.0                                      # parallel to the slab: inside it or never
    inside = (o >= lo) & (o <= hi)
    tn = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
    tf = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
    return np.maximum(tn.max(axis=1), tmin) <= np.minimum(tf.min(axis=1), tmax.astype(np.float64))


def _unit(d):
    d = (d / np.maximum(np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True), 1e-30)).astype(np.float32)
    d[np.abs(d).max(axis=1) == 0] = np.array([0.0, 1.0, 0.0], np.float32)
    return d


def _record(o, d, lo, hi, inv3, tmax):
    n = len(o)
    rec = np.concatenate([o, d, lo, hi, np.broadcast_to(CENTRE, (n, 3)), np.broadcast_to(inv3, (n, 3)), tmax[:, None]], axis=1).astype(np.float32)
    assert rec.shape == (n, 19)
    return np.ascontiguousarray(rec)


def case_sets(n=1 << 20, seed=20261004):
    """{name: (records [n, 19], must [n], wide [n], least share of must)}: `must` where the ray meets the box as it was before the builder's
    pad, `wide` where it meets the padded box inflated by 2 % of the scene on every axis.
      one_scale: every axis scaled alike, the scene's farthest plane at 1023
      squeezed:  the scene squeezed to 0.313881 and 1 / 40 on y and z, a scale per axis
      flat:      everything in the plane z = centre.z (the z axis holds nothing but the boxes' pad), a thousandth of the rays in the plane"""
    rng = np.random.default_rng(seed)
    centre = CENTRE
    coord_max = np.float32(np.abs(centre).max() + H)
    pad_abs = np.float32(coord_max / np.float32(524288.0))
    # inner boxes: log-uniform sizes, a quarter flat on one axis (axis-aligned triangles), a quarter touching the scene's rim
    size = (H * np.exp(rng.uniform(np.log(1e-4), 0.0, (n, 3)))).astype(np.float32)
    flat = rng.random(n) < 0.25
    size[flat, rng.integers(0, 3, flat.sum())] = 0.0
    lo0 = (centre - H + rng.random((n, 3), dtype=np.float32) * (2 * H - size)).astype(np.float32)
    rim = rng.random(n) < 0.25
    side = rng.integers(0, 2, (n, 3)).astype(bool)
    lo0 = np.where(rim[:, None] & side, centre + H - size, np.where(rim[:, None], centre - H, lo0)).astype(np.float32)
    hi0 = (lo0 + size).astype(np.float32)
    padded = lambda a, b: np.maximum(np.float32(1e-5) * np.maximum(np.float32(1.0), np.maximum(np.abs(a), np.abs(b))), pad_abs).astype(np.float32)
    pad = padded(lo0, hi0)
    lo, hi = (lo0 - pad).astype(np.float32), (hi0 + pad).astype(np.float32)     # what lbvh_build.hip k_prepare hands on
    # origins: three quarters inside the scene, the rest up to 32 scene sizes away
    far = rng.random(n) < 0.25
    o = (centre + (rng.random((n, 3), dtype=np.float32) * 2 - 1) * np.where(far[:, None], 64 * H, H)).astype(np.float32)
    # directions: aimed at a point of the inner box's surface (corners, edges, faces: grazing rays), some random
    u = rng.random((n, 3), dtype=np.float32)
    snap = rng.integers(0, 3, (n, 3))                   # 0 -> lo plane, 1 -> hi plane, 2 -> somewhere between
    target = np.where(snap == 0, lo0, np.where(snap == 1, hi0, lo0 + u * size)).astype(np.float32)
    d = (target - o).astype(np.float32)
    rnd_dir = rng.random(n) < 0.15
    d[rnd_dir] = rng.normal(size=(int(rnd_dir.sum()), 3)).astype(np.float32)
    d = (d / np.maximum(np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True), 1e-30)).astype(np.float32)
    # axis-parallel and near-degenerate components (incl. -0.0 and denormals)
    for frac, val in ((0.06, 0.0), (0.02, -0.0), (0.02, 1e-30), (0.02, -1e-38), (0.02, 1e-45)):
        m = rng.random(n) < frac
        d[m, rng.integers(0, 3, int(m.sum()))] = np.float32(val)
    keep = np.abs(d).max(axis=1) > 0
    d[~keep] = np.array([0.0, 1.0, 0.0], np.float32)
    tmax = np.where(rng.random(n) < 0.5, np.float32(1e16), (np.linalg.norm((target - o).astype(np.float64), axis=1) * rng.uniform(0.5, 1.5, n)).astype(np.float32)).astype(np.float32)
    out = {}

    must = exact_slab(o, d, lo0, hi0, 0.01, tmax)
    wide = exact_slab(o, d, lo - np.float32(0.02) * H, hi + np.float32(0.02) * H, 0.01, tmax)
    half_ext = np.float32(np.abs(np.concatenate([lo, hi]) - centre).max())
    inv1 = np.full(3, np.float32(half_ext / np.float32(1023.0)), np.float32)
    out["one_scale"] = (_record(o, d, lo, hi, inv1, tmax), must, wide, 0.3)

    # boxes, origins and targets squeezed about the centre, directions re-aimed
    f = lambda p: (centre + (p - centre) * SQUEEZE).astype(np.float32)
    lo0s, hi0s, os_ = f(lo0), f(hi0), f(o)
    ds = _unit((d * SQUEEZE).astype(np.float32))
    pads = padded(lo0s, hi0s)
    los, his = (lo0s - pads).astype(np.float32), (hi0s + pads).astype(np.float32)
    must = exact_slab(os_, ds, lo0s, hi0s, 0.01, tmax)
    wide = exact_slab(os_, ds, los - np.float32(0.02) * H * SQUEEZE, his + np.float32(0.02) * H * SQUEEZE, 0.01, tmax)
    inv3 = (np.abs(np.concatenate([los, his]) - centre).max(axis=0) / np.float32(1023.0)).astype(np.float32)
    assert inv3[0] > 2.5 * inv3[1] > 25 * inv3[2] > 0
    out["squeezed"] = (_record(os_, ds, los, his, inv3, tmax), must, wide, 0.2)

    # rays through the plane from both sides
    ff = lambda p: (centre + (p - centre) * FLATTEN).astype(np.float32)
    lo0f, hi0f = ff(lo0), ff(hi0)
    of = (centre + (o - centre) * np.array([1.0, 0.5, 0.05], np.float32)).astype(np.float32)
    df = (ff(target) - of).astype(np.float32)
    inplane = rng.random(n) < 1e-3
    df[inplane, 2] = 0.0; of[inplane, 2] = centre[2]
    df = _unit(df)
    padf = padded(lo0f, hi0f)
    lof, hif = (lo0f - padf).astype(np.float32), (hi0f + padf).astype(np.float32)
    must = exact_slab(of, df, lo0f, hi0f, 0.01, tmax)
    inv3f = (np.abs(np.concatenate([lof, hif]) - centre).max(axis=0) / np.float32(1023.0)).astype(np.float32)
    assert inv3f[2] < 1e-4 * inv3f[0]
    grow = (np.float32(0.02) * np.float32(1023.0) * inv3f).astype(np.float32)      # 2 % of the scene's half extent per axis: on z, of the pad
    wide = exact_slab(of, df, lof - grow, hif + grow, 0.01, tmax)
    out["flat"] = (_record(of, df, lof, hif, inv3f, tmax), must, wide, 0.1)
    return out
