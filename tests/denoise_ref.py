"""NumPy reference of pt_render_features / pt_denoise (include/acgpt.h states the same definition).

Everything is fp32 in the operation order of csrc/denoise.hip, taps dy-major, so that the GPU result agrees with this one to the
last bits of expf / sqrtf.  A skipped tap (outside the image, or exactly one of p and q a miss) adds an exact zero here.
Images are [h, w, 4] float32 with row 0 at the bottom, as the accumulation buffer is."""
import numpy as np

F = np.float32
SIGMA_Z = F(0.01)
NORMAL_SQUARINGS = 7            # sigma_n = 2^7 = 128
SIGMA_L = F(5.0)
ALBEDO_FLOOR = F(0.01)
H = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], np.float32)
G = np.array([0.25, 0.5, 0.25], np.float32)


# ---- features ------------------------------------------------------------------------------------------------------------------
def pixel_rays(w, h, eye, U, V, W):
    """[h*w, 8] rays through the pixel centres (origin, direction, tmin 0.01, tmax 1e16), pixel index y * w + x, row 0 at the bottom:
    d = 2 * ((x + 0.5) / w, (y + 0.5) / h) - 1, dir = normalize(d.x U + d.y V + W) with 1 / sqrt(dot), left to right."""
    U, V, W, eye = (np.asarray(a, np.float32) for a in (U, V, W, eye))
    dx = F(2.0) * ((np.arange(w, dtype=np.float32) + F(0.5)) / F(w)) - F(1.0)
    dy = F(2.0) * ((np.arange(h, dtype=np.float32) + F(0.5)) / F(h)) - F(1.0)
    D = (dx[None, :, None] * U[None, None, :] + dy[:, None, None] * V[None, None, :]) + W[None, None, :]
    dot = D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2]
    inv = F(1.0) / np.sqrt(dot)
    r = np.zeros((h * w, 8), np.float32)
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
    return F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1] + F(0.0722) * c[..., 2]


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
    hp, hq = ndp[..., 3] >= 0, ndq[..., 3] >= 0
    with np.errstate(all="ignore"):
        z = np.abs(ndp[..., 3] - ndq[..., 3]) / zden
        c = np.maximum(ndp[..., 0] * ndq[..., 0] + ndp[..., 1] * ndq[..., 1] + ndp[..., 2] * ndq[..., 2], F(0.0))
        for _ in range(NORMAL_SQUARINGS):
            c = c * c
    return hp == hq, np.where(hp, c, F(1.0)).astype(np.float32), np.where(hp, z, F(0.0)).astype(np.float32)


def demodulate(accum, albedo, nd):
    hit = nd[..., 3] >= 0
    a = np.where(hit[..., None], np.maximum(albedo[..., :3], ALBEDO_FLOOR), F(1.0)).astype(np.float32)
    return accum[..., :3] / a, a


def variance(accum, albedo, nd):
    """{c, var} after the pre-pass (5x5, step 1, geometry weights only)."""
    c, _ = demodulate(accum, albedo, nd)
    lp = _lum(c)
    zden = SIGMA_Z * F(1.0) * nd[..., 3]
    l = _lum(c)
    sw = np.zeros(lp.shape, np.float32); s1 = np.zeros_like(sw); s2 = np.zeros_like(sw)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ndq, inside = _tap(nd, dy, dx)
            lq, _ = _tap(l, dy, dx)
            ok, wn, z = _geometry(nd, ndq, zden)
            ok &= inside
            with np.errstate(all="ignore"):
                wq = np.where(ok, wn * np.exp(-z), F(0.0)).astype(np.float32)
            dl = np.where(ok, lq - lp, F(0.0)).astype(np.float32)
            sw += wq; s1 += wq * dl; s2 += wq * (dl * dl)
    m1, m2 = s1 / sw, s2 / sw
    return np.concatenate([c, np.maximum(m2 - m1 * m1, F(0.0))[..., None]], axis=-1).astype(np.float32)


def atrous(cv, nd, step):
    """One iteration at `step`: {c', var'}."""
    h, w = cv.shape[:2]
    var = cv[..., 3]
    gs = np.zeros((h, w), np.float32); gw = np.zeros((h, w), np.float32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            vq, inside = _tap(var, dy, dx)
            k = G[dx + 1] * G[dy + 1]
            gs += np.where(inside, k * vq, F(0.0)).astype(np.float32)
            gw += np.where(inside, k, F(0.0)).astype(np.float32)
    lden = SIGMA_L * np.sqrt(gs / gw) + F(1e-6)
    lp = _lum(cv)
    zden = SIGMA_Z * F(step) * nd[..., 3]
    sk = np.zeros((h, w), np.float32); sc = np.zeros((h, w, 3), np.float32); sv = np.zeros((h, w), np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, inside = _tap(cv, dy * step, dx * step)
            ndq, _ = _tap(nd, dy * step, dx * step)
            ok, wn, z = _geometry(nd, ndq, zden)
            ok &= inside
            with np.errstate(all="ignore"):
                el = np.abs(lp - _lum(cq)) / lden
                k = np.where(ok, H[dx + 2] * H[dy + 2] * wn * np.exp(-(z + el)), F(0.0)).astype(np.float32)
            sk += k
            sc += k[..., None] * cq[..., :3]
            sv += (k * k) * cq[..., 3]
    return np.concatenate([sc / sk[..., None], (sv / (sk * sk))[..., None]], axis=-1).astype(np.float32)


def denoise(accum, albedo, nd, iterations=5):
    """The output of pt_denoise: [h, w, 4] linear radiance, alpha 1."""
    assert 1 <= iterations <= 8
    accum, albedo, nd = (np.ascontiguousarray(a, np.float32) for a in (accum, albedo, nd))
    cv = variance(accum, albedo, nd)
    for i in range(iterations):
        cv = atrous(cv, nd, 1 << i)
    _, a = demodulate(accum, albedo, nd)
    out = np.ones(accum.shape, np.float32)
    out[..., :3] = cv[..., :3] * a
    return out
