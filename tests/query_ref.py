"""NumPy statement of pt_query_closest's hit record (include/acgpt.h states the same definition), and the ray sets its tests shoot.

The record's epilogue is fp32 in the operation order of csrc/query.hip — plain multiplies and adds, left to right, one IEEE division
per barycentric — so the GPU's record equals this one bit for bit.  The triangle edges are what the build stores in a TriRecord:
e1 = v1 - v0 and e2 = v2 - v0, one fp32 subtraction per component (csrc/lbvh_build.hip k_prepare, csrc/refit.hip k_rf_leaves), and
the normal is k_gather_leaves' normalize(cross(e1, e2)) = cross * (1 / sqrt(dot))."""
import numpy as np

F = np.float32
MISS_PRIM = np.uint32(0xFFFFFFFF)
SHADE_MAT_MASK = np.uint32(0x00FFFFFF)          # kShadeMatMask (csrc/pt_device.h)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def traceable(rays):
    """False where a ray is a miss before any traversal: a non-finite origin or direction component, a NaN tmin or tmax, or
    not (tmax > tmin)."""
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(rays[:, 0:6]).all(axis=1) & (rays[:, 7] > rays[:, 6])


def barycentrics(o, d, v0, e1, e2):
    """(u, v) of v1 and v2, any float dtype, in the order the header writes:
    p = cross(d, e2); det = dot(e1, p); s = o - v0; u = dot(s, p) / det; q = cross(s, e1); v = dot(d, q) / det"""
    p = _cross(d, e2)
    det = _dot(e1, p)
    s = o - v0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = _dot(s, p) / det
        q = _cross(s, e1)
        v = _dot(d, q) / det
    return u, v


def miss_records(n):
    """n miss records as uint32 [n, 8]: {-1, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0xFFFFFFFF}"""
    rec = np.zeros((n, 8), np.uint32)
    rec[:, 0] = F(-1.0).view(np.uint32)
    rec[:, 1] = MISS_PRIM
    rec[:, 7] = MISS_PRIM
    return rec


def hit_records(rays, t, prim, verts, idx, mat_ids):
    """pt_hit records as uint32 [n, 8] (t, prim, u, v, nx, ny, nz, material) from closest hits {t, prim} (pt_trace_closest's: -1 /
    0xFFFFFFFF on a miss) of `rays` against the scene (verts [*, 4] or flat, idx, one material id per triangle).  A ray that is no
    ray (traceable) or a scene without triangles gives the miss record whatever {t, prim} says."""
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    t = np.asarray(t, np.float32); prim = np.asarray(prim, np.uint32)
    idx = np.asarray(idx, np.uint32).reshape(-1, 3)
    rec = miss_records(rays.shape[0])
    hit = (prim != MISS_PRIM) & traceable(rays) & (idx.shape[0] > 0)
    if not hit.any():
        return rec
    p = prim[hit].astype(np.int64)
    tri = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3][idx[p]]
    v0 = tri[:, 0]
    e1, e2 = tri[:, 1] - v0, tri[:, 2] - v0
    o, d = rays[hit, 0:3], rays[hit, 3:6]
    u, v = barycentrics(o, d, v0, e1, e2)
    c = _cross(e1, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt(_dot(c, c))
        nrm = c * inv[:, None]
        away = _dot(nrm, d) > F(0.0)
    nrm[away] = -nrm[away]
    out = np.zeros((p.size, 8), np.float32)
    out[:, 0] = t[hit]
    out[:, 2] = u
    out[:, 3] = v
    out[:, 4:7] = nrm
    out = out.view(np.uint32)
    out[:, 1] = prim[hit]
    out[:, 7] = np.asarray(mat_ids, np.uint32)[p] & SHADE_MAT_MASK
    rec[hit] = out
    return rec


def barycentrics_f64(o, d, v0, v1, v2):
    """Moeller-Trumbore's (u, v) in float64 from the fp32 inputs: what the fp32 statement above is measured against."""
    o, d, v0, v1, v2 = (np.asarray(a, np.float64) for a in (o, d, v0, v1, v2))
    return barycentrics(o, d, v0, v1 - v0, v2 - v0)


# ---- ray sets --------------------------------------------------------------------------------------------------------------------
# Fixed seeds, chosen on the CPU with the oracle's brute force so that on the Cornell fixtures every set but the all-miss one hits
# on at least a quarter of its rays and misses on at least a tenth (tests/test_query_host.py holds that; the GPU tests hold it again
# on pt_trace_closest's own answers).
RAY_SETS = ("camera", "inside", "occlusion", "in_wall_planes", "outside")
SET_SIZE = 1000


def _rays(o, d, tmin, tmax):
    r = np.zeros((o.shape[0], 8), np.float32)
    r[:, 0:3] = o; r[:, 3:6] = d; r[:, 6] = tmin; r[:, 7] = tmax
    return r


def scene_box(verts, idx):
    used = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3][np.unique(np.asarray(idx, np.uint32))]
    return used.min(axis=0), used.max(axis=0)


def ray_set(name, verts, idx, camera):
    """SET_SIZE rays of the named set.  camera: (eye, U, V, W)."""
    import denoise_ref as dr
    lo, hi = scene_box(verts, idx)
    verts = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    idx = np.asarray(idx, np.uint32).reshape(-1, 3)
    ext = hi - lo
    n = SET_SIZE
    if name == "camera":            # pixel-centre rays of a 97 x 61 image, a fixed random choice of its pixels
        rng = np.random.default_rng(101)
        return dr.pixel_rays(97, 61, *camera)[np.sort(rng.permutation(97 * 61)[:n])]
    if name == "inside":            # from points inside the scene box, any direction and length, the reach 0 .. 1.5 box diagonals
        rng = np.random.default_rng(202)
        o = lo + rng.random((n, 3)).astype(np.float32) * ext
        d = rng.normal(size=(n, 3)).astype(np.float32) * rng.uniform(0.25, 4.0, (n, 1)).astype(np.float32)
        reach = rng.uniform(0.0, 1.5, n).astype(np.float32) * F(np.sqrt(float((ext * ext).sum())))
        tmax = reach / np.sqrt((d * d).sum(axis=1))
        tmax[::16] = np.inf
        return _rays(o, d, F(0.0), tmax)
    if name == "occlusion":         # the ambient-occlusion shape: leave a surface point along a random direction, tmin 1e-3, a short reach
        rng = np.random.default_rng(303)
        tri = verts[idx[rng.integers(0, idx.shape[0], n)]]
        b = rng.random((n, 2)).astype(np.float32)
        fold = b.sum(axis=1) > 1.0
        b[fold] = F(1.0) - b[fold]
        o = tri[:, 0] + b[:, 0:1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:2] * (tri[:, 2] - tri[:, 0])
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
        return _rays(o, d, F(1e-3), rng.uniform(0.05, 0.6, n).astype(np.float32) * F(ext.max()))
    if name == "in_wall_planes":    # axis-parallel rays lying in the planes of the scene box's faces: two zero direction components
        rng = np.random.default_rng(404)
        o = lo + rng.random((n, 3)).astype(np.float32) * ext
        face = rng.integers(0, 3, n)                     # the axis whose plane the ray lies in
        side = rng.integers(0, 2, n)
        o[np.arange(n), face] = np.where(side == 0, lo[face], hi[face])
        along = (face + 1 + rng.integers(0, 2, n)) % 3   # one of the other two axes
        d = np.zeros((n, 3), np.float32)
        d[np.arange(n), along] = np.where(rng.integers(0, 2, n) == 0, F(-1.0), F(1.0)) * rng.uniform(0.5, 2.0, n).astype(np.float32)
        reach = rng.uniform(0.0, 1.2, n).astype(np.float32) * ext[along]
        return _rays(o, d, F(0.0), reach / np.abs(d[np.arange(n), along]))
    if name == "outside":           # from outside the scene box, pointing away from it: every one a miss
        rng = np.random.default_rng(505)
        c = F(0.5) * (lo + hi)
        away = rng.normal(size=(n, 3)).astype(np.float32)
        away /= np.sqrt((away * away).sum(axis=1, keepdims=True))
        o = c + away * (F(1.5) * F(np.sqrt(float((ext * ext).sum()))))
        d = away + F(0.2) * rng.normal(size=(n, 3)).astype(np.float32)
        d[(d * away).sum(axis=1) <= 0] = away[(d * away).sum(axis=1) <= 0]
        return _rays(o, d, F(0.0), F(1e16))
    raise ValueError(name)


# the bad rays of the tests: each with what makes it a miss before any traversal; `good` is the ray they are made from
def bad_rays(good):
    good = np.asarray(good, np.float32).reshape(8)
    out, why = [], []
    for k in range(8):
        for val in (np.nan, np.inf, -np.inf):
            if k == 6 and val == -np.inf:
                continue        # tmin = -inf is a ray: the interval is (-inf, tmax)
            if k == 7 and val == np.inf:
                continue        # tmax = +inf is allowed
            r = good.copy(); r[k] = val
            out.append(r); why.append("field %d = %s" % (k, val))
    r = good.copy(); r[7] = r[6]
    out.append(r); why.append("tmax == tmin")
    r = good.copy(); r[7] = np.nextafter(r[6], F(-np.inf))
    out.append(r); why.append("tmax < tmin")
    r = good.copy(); r[6], r[7] = F(5.0), F(-5.0)
    out.append(r); why.append("tmax < 0 < tmin")
    return np.array(out, np.float32), why
