"""NumPy reference of pt_render_features / pt_denoise (include/acgpt.h states the same definition).

Everything is fp32 in the operation order of csrc/denoise.hip, taps dy-major, so that the GPU result agrees with this one to the
last bits of expf / sqrtf.  A skipped tap (outside the image, or exactly one of p and q a miss) adds an exact zero here.
Images are [h, w, 4] float32 with row 0 at the bottom, as the accumulation buffer is.

dtype=np.float64 evaluates the same formulas from the same fp32 inputs in double precision, with the constants as the header
writes them (0.01, not its fp32 rounding): what the fp32 arithmetic is measured against.  Only the decision which pixels are unusable
stays an fp32 one, since the rule is stated on fp32 values.

NaN: the kernel's fmaxf(x, 0) returns 0 for a NaN x.  Every max below is written np.where(x > 0, x, 0), which says the same
explicitly; nothing here depends on how a library's maximum treats NaN.  The rules for invalid inputs are those of include/acgpt.h."""
import numpy as np

F = np.float32
SIGMA_Z = F(0.01)
NORMAL_SQUARINGS = 7            # sigma_n = 2^7 = 128
SIGMA_L = F(5.0)
ALBEDO_FLOOR = F(0.01)
MAX_LUM = F(2.0 ** 60)          # a pixel whose |l(c)| exceeds it is unusable: its square and the sums of squares stay finite below it
H = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], np.float32)
G = np.array([0.25, 0.5, 0.25], np.float32)


# ---- features ------------------------------------------------------------------------------------------------------------------
def pixel_rays(w, h, eye, U, V, W, dtype=np.float32):
    """[h*w, 8] rays through the pixel centres (origin, direction, tmin 0.01, tmax 1e16), pixel index y * w + x, row 0 at the bottom:
    d = 2 * ((x + 0.5) / w, (y + 0.5) / h) - 1, dir = normalize(d.x U + d.y V + W) with 1 / sqrt(dot), left to right."""
    F = np.dtype(dtype).type
    U, V, W, eye = (np.asarray(a, np.float32).astype(dtype) for a in (U, V, W, eye))
    dx = F(2.0) * ((np.arange(w, dtype=dtype) + F(0.5)) / F(w)) - F(1.0)
    dy = F(2.0) * ((np.arange(h, dtype=dtype) + F(0.5)) / F(h)) - F(1.0)
    D = (dx[None, :, None] * U[None, None, :] + dy[:, None, None] * V[None, None, :]) + W[None, None, :]
    dot = D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2]
    inv = F(1.0) / np.sqrt(dot)
    r = np.zeros((h * w, 8), dtype)
    r[:, 0:3] = eye
    r[:, 3:6] = (D * inv[..., None]).reshape(-1, 3)
    r[:, 6] = F(0.01)
    r[:, 7] = F(1e16)
    return r


def features_from_hits(rays, t, prim, verts, idx, mat_ids, diffuse):
    """albedo_prim, normal_depth ([n, 4] float32) from closest hits (t = -1 / prim = 0xFFFFFFFF on a miss): the normal is
    normalize(cross(v1 - v0, v2 - v0)) negated where it faces away from the ray, the albedo the material's diffuse colour."""
    n = rays.shape[0]
    hit = prim != 0xFFFFFFFF
    alb = np.zeros((n, 4), np.float32)
    nd = np.zeros((n, 4), np.float32)
    alb[:, 3] = np.uint32(0xFFFFFFFF).view(np.float32)
    nd[:, 3] = F(-1.0)
    p = prim[hit].astype(np.int64)
    tri = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3][np.asarray(idx, np.uint32).reshape(-1, 3)[p]]
    a, b = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    inv = F(1.0) / np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    nrm = c * inv[:, None]
    d = rays[hit, 3:6]
    away = (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1] + nrm[:, 2] * d[:, 2]) > F(0.0)
    nrm[away] = -nrm[away]
    nd[hit, 0:3] = nrm
    nd[hit, 3] = t[hit]
    alb[hit, 0:3] = np.asarray(diffuse, np.float32)[np.asarray(mat_ids, np.uint32)[p]]
    alb[hit, 3] = prim[hit].view(np.float32)
    return alb, nd


# ---- filter --------------------------------------------------------------------------------------------------------------------
def _lum(c):
    T = c.dtype.type
    return T(0.2126) * c[..., 0] + T(0.7152) * c[..., 1] + T(0.0722) * c[..., 2]


def _tap(a, dy, dx):
    """a[y + dy, x + dx] (zero outside) and whether the tap is inside the image."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    if abs(dy) >= h or abs(dx) >= w:
        return out, inside
    ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
    xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    inside[yd, xd] = True
    return out, inside


def _geometry(ndp, ndq, zden):
    """(tap usable, w_n, z) for every pixel; see include/acgpt.h."""
    T = ndp.dtype.type
    hp, hq = ndp[..., 3] >= 0, ndq[..., 3] >= 0           # a NaN distance is a miss
    with np.errstate(all="ignore"):
        zok = (zden != 0) & np.isfinite(zden)              # else: z = 0 where t_q == t_p, and every other tap is skipped
        z = np.where(zok, np.abs(ndp[..., 3] - ndq[..., 3]) / zden, T(0.0))
        dot = ndp[..., 0] * ndq[..., 0] + ndp[..., 1] * ndq[..., 1] + ndp[..., 2] * ndq[..., 2]
        c = np.where(dot > 0, dot, T(0.0))                 # fmaxf(dot, 0): 0 for a NaN dot
        for _ in range(NORMAL_SQUARINGS):
            c = c * c
    ok = (hp == hq) & (~hp | zok | (ndq[..., 3] == ndp[..., 3]))
    return ok, np.where(hp, c, T(1.0)).astype(ndp.dtype), np.where(hp, z, T(0.0)).astype(ndp.dtype)


def demodulate(accum, albedo, nd):
    T = accum.dtype.type
    hit = nd[..., 3] >= 0
    floor = T(0.01)
    alb = albedo[..., :3]
    a = np.where(hit[..., None], np.where(alb > floor, alb, floor), T(1.0)).astype(accum.dtype)      # fmaxf(albedo, 0.01): 0.01 for NaN
    with np.errstate(all="ignore"):
        return accum[..., :3] / a, a


def usable(accum, albedo, nd):
    """[h, w] bool, decided in fp32: every demodulated channel finite and |l(c)| <= 2^60 (a NaN l fails)."""
    accum, albedo, nd = (np.ascontiguousarray(a, np.float32) for a in (accum, albedo, nd))
    c, _ = demodulate(accum, albedo, nd)
    with np.errstate(all="ignore"):
        return np.isfinite(c).all(axis=-1) & (np.abs(_lum(c)) <= MAX_LUM)


def variance(accum, albedo, nd, dtype=np.float32):
    """{c, var} after the pre-pass (5x5, step 1, geometry weights only); var = -1 marks an unusable pixel."""
    T = np.dtype(dtype).type
    use = usable(accum, albedo, nd)
    accum, albedo, nd = (np.ascontiguousarray(a, np.float32).astype(dtype) for a in (accum, albedo, nd))
    c, _ = demodulate(accum, albedo, nd)
    with np.errstate(all="ignore"):
        lp = _lum(c)
    zden = T(0.01) * T(1.0) * nd[..., 3]
    l = lp
    sw = np.zeros(lp.shape, dtype); s1 = np.zeros_like(sw); s2 = np.zeros_like(sw)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ndq, inside = _tap(nd, dy, dx)
            lq, _ = _tap(l, dy, dx)
            uq, _ = _tap(use, dy, dx)
            ok, wn, z = _geometry(nd, ndq, zden)
            ok &= inside & uq
            with np.errstate(all="ignore"):
                wq = np.where(ok, wn * np.exp(-z), T(0.0)).astype(dtype)
                dl = np.where(ok, lq - lp, T(0.0)).astype(dtype)
                sw += wq; s1 += wq * dl; s2 += wq * (dl * dl)
    with np.errstate(all="ignore"):
        m1, m2 = s1 / sw, s2 / sw
        v = m2 - m1 * m1
        v = np.where(v > 0, v, T(0.0))                                 # fmaxf(v, 0): 0 for NaN
        v = np.where((sw > 0) & np.isfinite(v), v, T(0.0))             # no weight at all: var 0
    v = np.where(use, v, T(-1.0))
    return np.concatenate([c, v[..., None]], axis=-1).astype(dtype)


def atrous(cv, nd, step):
    """One iteration at `step`: {c', var'}, in cv's dtype."""
    dtype = cv.dtype
    T = dtype.type
    nd = nd.astype(dtype)
    h, w = cv.shape[:2]
    var = cv[..., 3]
    gs = np.zeros((h, w), dtype); gw = np.zeros((h, w), dtype)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            vq, inside = _tap(var, dy, dx)
            inside &= ~(vq < 0)
            k = T(G[dx + 1]) * T(G[dy + 1])
            gs += np.where(inside, k * vq, T(0.0)).astype(dtype)
            gw += np.where(inside, k, T(0.0)).astype(dtype)
    with np.errstate(all="ignore"):
        lden = T(5.0) * np.sqrt(gs / gw) + T(1e-6)
        lp = _lum(cv)
    zden = T(0.01) * T(step) * nd[..., 3]
    sk = np.zeros((h, w), dtype); sc = np.zeros((h, w, 3), dtype); sv = np.zeros((h, w), dtype)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, inside = _tap(cv, dy * step, dx * step)
            ndq, _ = _tap(nd, dy * step, dx * step)
            ok, wn, z = _geometry(nd, ndq, zden)
            ok &= inside & ~(cq[..., 3] < 0)
            cq = np.where(ok[..., None], cq, T(0.0))
            with np.errstate(all="ignore"):
                el = np.abs(lp - _lum(cq)) / lden
                k = np.where(ok, T(H[dx + 2]) * T(H[dy + 2]) * wn * np.exp(-(z + el)), T(0.0)).astype(dtype)
                sk += k
                sc += k[..., None] * cq[..., :3]
                sv += (k * k) * cq[..., 3]
    with np.errstate(all="ignore"):
        c = sc / sk[..., None]
        v = sv / (sk * sk)
    keep = ~((sk > 0) & np.isfinite(c).all(axis=-1) & np.isfinite(v)) | (var < 0)      # keeps c_p and var_p for this pass
    out = np.concatenate([c, v[..., None]], axis=-1).astype(dtype)
    out[keep] = cv[keep]
    return out


def denoise(accum, albedo, nd, iterations=5, dtype=np.float32):
    """The output of pt_denoise: [h, w, 4] linear radiance, alpha 1 (float32, or the float64 evaluation with dtype=np.float64)."""
    assert 1 <= iterations <= 8
    accum, albedo, nd = (np.ascontiguousarray(a, np.float32) for a in (accum, albedo, nd))
    cv = variance(accum, albedo, nd, dtype)
    bad = cv[..., 3] < 0
    for i in range(iterations):
        cv = atrous(cv, nd, 1 << i)
    _, a = demodulate(accum.astype(dtype), albedo.astype(dtype), nd.astype(dtype))
    out = np.ones(accum.shape, dtype)
    with np.errstate(all="ignore"):
        out[..., :3] = cv[..., :3] * a
    out[bad, :3] = accum[bad, :3]                  # an unusable pixel: its accumulation rgb as bits
    return out
