"""NumPy statement of the microfacet material model (pt_set_material_model(ctx, PT_MATERIALS_MICROFACET), include/acgpt.h;
csrc/pt_microfacet.h): isotropic GGX, Smith G1, height-correlated G2, Heitz 2018 visible-normal sampling, the reference's conductor
Fresnel and Walter et al. 2007 for the dielectric, with the BTDF normalised without a 1 / eta^2 factor.  Vectorised over the
leading axis, float64.  The normal is (0, 0, 1) face-forwarded to wo, as pt_debug_microfacet has it; the tangent frame is
onb_transform's."""
import numpy as np

METALLIC, REFRACTION = 1, 2
SMOOTH_ALPHA = 1e-3
ETA_C = np.array([1.45, 0.7, 1.55])
K_C = np.array([3.0, 2.2, 3.5])


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def onb_axes(n):
    """(tg, bn) of onb_transform for unit normals n [..., 3]."""
    n = np.asarray(n, np.float64)
    bx = np.where(np.abs(n[..., 0]) > np.abs(n[..., 2]), -n[..., 1], 0.0)
    by = np.where(np.abs(n[..., 0]) > np.abs(n[..., 2]), n[..., 0], -n[..., 2])
    bz = np.where(np.abs(n[..., 0]) > np.abs(n[..., 2]), 0.0, n[..., 1])
    bn = _normalize(np.stack([bx, by, bz], -1))
    return np.cross(bn, n), bn


def lam(c, a2):
    c2 = c * c
    with np.errstate(divide="ignore", invalid="ignore"):
        return 0.5 * (np.sqrt(1.0 + a2 * (1.0 - c2) / c2) - 1.0)


def g1(c, a2):
    return 1.0 / (1.0 + lam(c, a2))


def ggx_d(ch, a2):
    t = ch * ch * (a2 - 1.0) + 1.0
    return a2 / (np.pi * t * t)


def sample_vndf(ve, alpha, u1, u2):
    """Heitz 2018 in the local frame: half vectors for local directions ve (z > 0)."""
    a = np.asarray(alpha, np.float64)[..., None] * np.ones_like(ve)
    vh = _normalize(np.stack([a[..., 0] * ve[..., 0], a[..., 1] * ve[..., 1], ve[..., 2]], -1))
    lensq = vh[..., 0] ** 2 + vh[..., 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sqrt(lensq)
    t1v = np.where((lensq > 0)[..., None], np.stack([-vh[..., 1] * inv, vh[..., 0] * inv, np.zeros_like(lensq)], -1),
                   np.array([1.0, 0.0, 0.0]))
    t2v = np.cross(vh, t1v)
    r = np.sqrt(u1)
    phi = 2.0 * np.pi * u2
    t1 = r * np.cos(phi)
    s = 0.5 * (1.0 + vh[..., 2])
    t2 = (1.0 - s) * np.sqrt(np.maximum(0.0, 1.0 - t1 * t1)) + s * (r * np.sin(phi))
    nh = t1[..., None] * t1v + t2[..., None] * t2v + np.sqrt(np.maximum(0.0, 1.0 - t1 * t1 - t2 * t2))[..., None] * vh
    return _normalize(np.stack([a[..., 0] * nh[..., 0], a[..., 1] * nh[..., 1], np.maximum(0.0, nh[..., 2])], -1))


def fresnel_conductor(c):
    """fresnelSchlickConductor with the reference's constants, per channel: [..., 3]."""
    c = np.asarray(c, np.float64)[..., None]
    eta2, k2, c2 = ETA_C ** 2, K_C ** 2, c * c
    t1 = eta2 - k2 - c2
    ab = np.sqrt(t1 * t1 + 4 * eta2 * k2)
    t2 = ab + c2
    rs = (t2 - 2 * ETA_C * c + c2) / (t2 + 2 * ETA_C * c + c2)
    rp = rs * (t2 - 2 * ETA_C * c + 1.0) / (t2 + 2 * ETA_C * c + 1.0)
    return (rs + rp) * 0.5


def fr_dielectric(cos_i, eta_i, eta_t):
    cos_i = np.clip(np.asarray(cos_i, np.float64), -1.0, 1.0)
    flip = ~(cos_i > 0)
    ei = np.where(flip, eta_t, eta_i)
    et = np.where(flip, eta_i, eta_t)
    cos_i = np.abs(cos_i)
    sin_i = np.sqrt(np.maximum(0.0, 1.0 - cos_i * cos_i))
    sin_t = ei / et * sin_i
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    rpar = (et * cos_i - ei * cos_t) / (et * cos_i + ei * cos_t)
    rper = (ei * cos_i - et * cos_t) / (ei * cos_i + et * cos_t)
    return np.where(sin_t >= 1.0, 1.0, (rpar * rpar + rper * rper) / 2.0)


def _frame(wo):
    n = np.zeros_like(wo)
    n[..., 2] = np.where(wo[..., 2] >= 0, 1.0, -1.0)       # faceforward((0, 0, 1), wo): copysign(1, wo.z)
    return n, wo[..., 2] > 0


def sample(bsdf, wo, alpha, ior, u1, u2, u3):
    """-> wi [n, 3], weight [n, 3] (f |cos_i| / pdf without Kd), pdf [n], lobe [n] (0 ended, 1 reflection, 2 transmission)."""
    wo = np.asarray(wo, np.float64)
    n = wo.shape[0]
    bsdf, alpha, ior = (np.broadcast_to(np.asarray(x, np.float64), (n,)) for x in (bsdf, alpha, ior))
    u1, u2, u3 = (np.broadcast_to(np.asarray(x, np.float64), (n,)) for x in (u1, u2, u3))
    N, entering = _frame(wo)
    tg, bn = onb_axes(N)
    co = _dot(wo, N)
    hl = sample_vndf(np.stack([_dot(wo, tg), _dot(wo, bn), co], -1), alpha, u1, u2)
    h = hl[..., :1] * tg + hl[..., 1:2] * bn + hl[..., 2:] * N
    a2 = alpha * alpha
    oh = _dot(wo, h)
    lo = lam(co, a2)
    d = ggx_d(_dot(N, h), a2)
    pdf_h = d / (4.0 * co * (1.0 + lo))
    glass = bsdf == REFRACTION
    F = np.where(glass, fr_dielectric(np.where(entering, oh, -oh), 1.0, ior), 1.0)
    transmit = glass & ~(u3 < F)
    # reflection
    wr = 2.0 * oh[:, None] * h - wo
    cr = _dot(wr, N)
    gr = (1.0 + lo) / (1.0 + lo + lam(cr, a2))
    wt_r = np.where(glass[:, None], gr[:, None] * np.ones(3), fresnel_conductor(oh) * gr[:, None])
    pdf_r = np.where(glass, F * pdf_h, pdf_h)
    # transmission
    eta = np.where(entering, ior, 1.0 / ior)
    e = 1.0 / eta
    k = 1.0 - e * e * (1.0 - oh * oh)
    wt = (e * oh - np.sqrt(np.maximum(k, 0.0)))[:, None] * h - e[:, None] * wo
    ct = _dot(wt, N)
    ih = _dot(wt, h)
    den = oh + eta * ih
    gt = (1.0 + lo) / (1.0 + lo + lam(ct, a2))
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf_t = (1.0 - F) * d * oh * eta * eta * np.abs(ih) / (co * (1.0 + lo) * den * den)
    ok_r = ~transmit & (cr > 0)
    ok_t = transmit & (k >= 0) & (ct < 0)
    wi = np.where(transmit[:, None], wt, wr)
    weight = np.where(ok_r[:, None], wt_r, np.where(ok_t[:, None], gt[:, None] * np.ones(3), 0.0))
    pdf = np.where(ok_r, pdf_r, np.where(ok_t, pdf_t, 0.0))
    lobe = np.where(ok_r, 1, np.where(ok_t, 2, 0))
    return wi, weight, pdf, lobe


def evaluate(bsdf, wo, wi, alpha, ior):
    """-> f [n, 3] (without Kd), pdf [n]: the BSDF and the solid-angle pdf with which sample() draws wi."""
    wo = np.asarray(wo, np.float64)
    wi = np.asarray(wi, np.float64)
    n = wo.shape[0]
    bsdf, alpha, ior = (np.broadcast_to(np.asarray(x, np.float64), (n,)) for x in (bsdf, alpha, ior))
    N, entering = _frame(wo)
    a2 = alpha * alpha
    co, ci = _dot(wo, N), _dot(wi, N)
    lo = lam(co, a2)
    glass = bsdf == REFRACTION
    with np.errstate(divide="ignore", invalid="ignore"):
        # reflection
        hr = _normalize(wo + wi)
        ohr = _dot(wo, hr)
        dr = ggx_d(_dot(N, hr), a2)
        g2r = 1.0 / (1.0 + lo + lam(ci, a2))
        dg = dr * g2r / (4.0 * co * ci)
        pdf_hr = dr / (4.0 * co * (1.0 + lo))
        Fr = fr_dielectric(np.where(entering, ohr, -ohr), 1.0, ior)
        f_r = np.where(glass[:, None], (Fr * dg)[:, None] * np.ones(3), fresnel_conductor(ohr) * dg[:, None])
        p_r = np.where(glass, Fr * pdf_hr, pdf_hr)
        ok_r = (ci > 0) & (ohr > 0)
        # transmission
        eta = np.where(entering, ior, 1.0 / ior)
        ht = _normalize(wo + eta[:, None] * wi)
        ht = np.where((_dot(ht, N) < 0)[:, None], -ht, ht)
        oht, iht = _dot(wo, ht), _dot(wi, ht)
        Ft = fr_dielectric(np.where(entering, oht, -oht), 1.0, ior)
        dt = ggx_d(_dot(N, ht), a2)
        g2t = 1.0 / (1.0 + lo + lam(ci, a2))
        den = oht + eta * iht
        j = dt * oht * eta * eta * np.abs(iht) / (co * den * den)
        f_t = (1.0 - Ft) * j * g2t / np.abs(ci)
        p_t = (1.0 - Ft) * j / (1.0 + lo)
        ok_t = glass & (ci < 0) & (oht > 0) & (iht < 0)
    f = np.where(ok_r[:, None], f_r, np.where(ok_t[:, None], f_t[:, None] * np.ones(3), 0.0))
    pdf = np.where(ok_r, p_r, np.where(ok_t, p_t, 0.0))
    return np.nan_to_num(f), np.nan_to_num(pdf)


def sphere_grid(n_theta, n_phi):
    """Midpoint quadrature over the unit sphere: directions [n, 3] and their solid angles [n]."""
    t = (np.arange(n_theta) + 0.5) * np.pi / n_theta
    p = (np.arange(n_phi) + 0.5) * 2 * np.pi / n_phi
    T, P = np.meshgrid(t, p, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    dw = (np.sin(T) * (np.pi / n_theta) * (2 * np.pi / n_phi)).reshape(-1)
    return d, dw


def albedo(bsdf, cos_o, alpha, ior=1.5, n=200000, seed=0):
    """Single-scatter directional albedo E(cos_o) = mean of the sampled weight (per channel, without Kd), by Monte Carlo."""
    rng = np.random.default_rng(seed)
    so = np.sqrt(1.0 - cos_o * cos_o)
    wo = np.tile([so, 0.0, cos_o], (n, 1))
    _, w, _, _ = sample(bsdf, wo, alpha, ior, rng.random(n), rng.random(n), rng.random(n))
    return w.mean(0), w.std(0) / np.sqrt(n)
