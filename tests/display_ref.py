"""NumPy statement of pt_display_transform (include/acgpt.h): the bins, the meter, the tone curves.  Every floating-point value is
float32 and every operation is written once, in the order the header and csrc/display.hip write it; the metering is integer
arithmetic (Python ints).  make_color is here for the CPU tests only: the device's powf is not NumPy's, so the GPU tests compare the
frame buffer with pt_resolve_framebuffer of the call's own output instead."""
import numpy as np

F = np.float32
BINS = 320
BIN_BASE = 856                      # bits(2^-20) >> 20
L_MIN = F(2.0 ** -20)
X_MAX = F(65504.0)
LINEAR, REINHARD, ACES = 0, 1, 2
CURVES = {"linear": LINEAR, "reinhard": REINHARD, "aces": ACES}

DEFAULTS = dict(tone_curve=ACES, exposure=0.0, key=0.18, white=4.0, lo_permille=100, hi_permille=900, min_exposure=2.0 ** -16, max_exposure=2.0 ** 16,
                prev_exposure=0.0, adapt=1.0)


def params(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def lum(rgb):
    """0.2126 r + 0.7152 g + 0.0722 b, left to right; rgb: float32 [..., >= 3]"""
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


def metered(l):
    l = np.asarray(l, F)
    with np.errstate(all="ignore"):
        return np.isfinite(l) & (l >= L_MIN)


def bin_index(l):
    """bin of every luminance, -1 where the pixel is not metered"""
    l = np.asarray(l, F)
    k = np.minimum((l.view(np.uint32).astype(np.int64) >> 20) - BIN_BASE, BINS - 1)
    return np.where(metered(l), k, -1)


def histogram(src):
    """(counts uint32 [320], unmetered pixels) of a float32 [n, >= 3] image"""
    k = bin_index(lum(src)).ravel()
    return np.bincount(k[k >= 0], minlength=BINS).astype(np.uint32), int((k < 0).sum())


def window(n, lo_permille, hi_permille):
    r_lo, r_hi = n * int(lo_permille) // 1000, n * int(hi_permille) // 1000
    return (0, n) if r_hi <= r_lo else (r_lo, r_hi)


def mean_luminance(hist, lo_permille, hi_permille):
    """L_avg (float32): the windowed mean of the bin centres, steps 1-5; 0 for an empty histogram"""
    n = int(np.sum(hist, dtype=np.uint64))
    if n == 0:
        return F(0.0)
    r_lo, r_hi = window(n, lo_permille, hi_permille)
    c = T = S = 0
    for k in range(BINS):
        h = int(hist[k])
        t = max(0, min(c + h, r_hi) - max(c, r_lo))
        T += t
        S += t * (2 * k + 1)
        c += h
    return np.array([(BIN_BASE << 20) + (S << 19) // T], np.uint32).view(F)[0]


def mean_luminance_sorted(bins_of_pixels, lo_permille, hi_permille):
    """the same by brute force: sort the pixels' bins, keep the ranks r_lo .. r_hi - 1, average 2k + 1"""
    ks = sorted(int(k) for k in bins_of_pixels)
    if not ks:
        return F(0.0)
    r_lo, r_hi = window(len(ks), lo_permille, hi_permille)
    kept = ks[r_lo:r_hi]
    return np.array([(BIN_BASE << 20) + (sum(2 * k + 1 for k in kept) << 19) // len(kept)], np.uint32).view(F)[0]


def meter(hist, dp):
    """(exposure, metered_luminance) as float32, steps 1-7 and the n == 0 rule"""
    prev, adapt = F(dp["prev_exposure"]), F(dp["adapt"])
    if int(np.sum(hist, dtype=np.uint64)) == 0:
        return (prev if prev > 0 else F(1.0)), F(0.0)
    l_avg = mean_luminance(hist, dp["lo_permille"], dp["hi_permille"])
    with np.errstate(all="ignore"):
        target = F(dp["key"]) / l_avg
        target = np.maximum(target, F(dp["min_exposure"]))
        target = np.minimum(target, F(dp["max_exposure"]))
        exposure = prev + (target - prev) * adapt if prev > 0 else target
    return F(exposure), l_avg


def tone(x, curve, white=4.0):
    """y of x: float32 [..., 3], already clamped to [0, 65504]"""
    x = np.asarray(x, F)
    one = F(1.0)
    with np.errstate(all="ignore"):
        if curve == ACES:
            return np.minimum((x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14)), one)
        if curve == REINHARD:
            l = lum(x)
            w2 = F(white) * F(white)
            s = np.where(l > 0, (one + l / w2) / (one + l), F(0.0)).astype(F)
            return np.minimum(x * s[..., None], one)
        assert curve == LINEAR
        return np.minimum(x, one)


def apply(src, exposure, curve, white=4.0):
    """out_rgba: float32 [..., 4] = {y, 1}"""
    src = np.asarray(src, F)
    with np.errstate(all="ignore"):
        v = src[..., :3] * F(exposure)
        x = np.where(v > 0, np.where(v < X_MAX, v, X_MAX), F(0.0)).astype(F)
    out = np.ones(src.shape[:-1] + (4,), F)
    out[..., :3] = tone(x, curve, white)
    return out


def transform(src, dp):
    """(out_rgba float32 [n, 4], info dict) of a float32 [n, 4] image under pt_display_params as a dict (params())"""
    src = np.asarray(src, F)
    if dp["exposure"] > 0:
        info = dict(exposure=F(dp["exposure"]), metered_luminance=F(0.0), metered_pixels=0, unmetered_pixels=0, histogram=np.zeros(BINS, np.uint32))
    else:
        hist, unmetered = histogram(src.reshape(-1, src.shape[-1]))
        e, l_avg = meter(hist, dp)
        info = dict(exposure=e, metered_luminance=l_avg, metered_pixels=int(hist.sum(dtype=np.uint64)), unmetered_pixels=unmetered, histogram=hist)
    return apply(src, info["exposure"], dp["tone_curve"], dp["white"]), info


def make_color(y):
    """uint8 [..., 4] of display-linear [..., 3] (csrc/pt_shading.h make_color; CPU tests only: powf differs in the last bit)"""
    c = np.clip(np.asarray(y, F), F(0.0), F(1.0))
    with np.errstate(all="ignore"):
        s = np.where(c < F(0.0031308), F(12.92) * c, F(1.055) * np.power(c, F(1.0) / F(2.4), dtype=F) - F(0.055)).astype(F)
    q = np.minimum((np.clip(s, F(0.0), F(1.0)) * F(256.0)).astype(np.uint32), 255).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], axis=-1)
