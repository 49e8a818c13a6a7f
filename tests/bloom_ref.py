"""NumPy statement of pt_bloom (include/acgpt.h): the levels, the prefilter, the binomial down step, the bilinear up step, the combine,
the composite and the info record.  With dtype = float32 (the default) every value is float32 and every operation is written once, in
the order the header and csrc/bloom.hip write it; the counts and the two q16 sums are integers (the sums modulo 2^64, as the
device's).  dtype = float64 is the twin the tests hold the float32 result to: the same operations, rounded 2^29 times finer."""
import numpy as np

F = np.float32
Q16_CAP = 2.0 ** 24
MAX_LEVELS = 8
# threshold, knee and levels as the issue sets them, the intensity from tools/bloom_sweep.py's table
DEFAULTS = dict(threshold=1.0, knee=0.5, clamp=0.0, intensity=0.02, spread=1.0, levels=6)


def params(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def check(p):
    fin = all(np.isfinite(p[k]) for k in ("threshold", "knee", "clamp", "intensity", "spread"))
    assert fin and p["threshold"] >= 0 and 0 <= p["knee"] <= p["threshold"] and p["clamp"] >= 0 and p["intensity"] >= 0 and 0 <= p["spread"] <= 4
    assert 1 <= int(p["levels"]) <= MAX_LEVELS


def levels_of(w, h, levels):
    """[(w_1, h_1), ..., (w_n, h_n)]: halved rounding up, until `levels` are built or a level is 1 x 1"""
    out = []
    for _ in range(int(levels)):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
        if w == 1 and h == 1:
            break
    return out


def lum(rgb, dtype=F):
    """(0.2126 r + 0.7152 g) + 0.0722 b; rgb: [..., >= 3]"""
    rgb = np.asarray(rgb, dtype)
    with np.errstate(all="ignore"):
        return (dtype(0.2126) * rgb[..., 0] + dtype(0.7152) * rgb[..., 1]) + dtype(0.0722) * rgb[..., 2]


def valid(l):
    with np.errstate(all="ignore"):
        return np.isfinite(l) & (l >= 0)


def q16(x):
    """(uint64) trunc(min(x, 2^24) * 65536) of non-negative values"""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        return (np.minimum(x, x.dtype.type(Q16_CAP)) * x.dtype.type(65536.0)).astype(np.uint64)


def excess(l, threshold, knee, clamp, dtype=F):
    """e of valid luminances l: the part above the threshold, through the knee and the clamp"""
    T, K, C = dtype(threshold), dtype(knee), dtype(clamp)
    l = np.asarray(l, dtype)
    zero = dtype(0.0)
    with np.errstate(all="ignore"):
        d = l - T
        if K > 0:
            s = np.minimum(np.maximum(l - (T - K), zero), K + K)
            q = (s * s) / ((K + K) + (K + K))
            e = np.maximum(q, d)
        else:
            e = np.maximum(d, zero)
        if C > 0:
            e = np.minimum(e, C)
    return e


def prefilter(img, threshold, knee, clamp, dtype=F):
    """(P [h, w, 3], l [h, w], ok, lit, e): the bright part of every pixel; invalid and dark pixels give 0"""
    rgb = np.asarray(img, dtype)[..., :3]
    l = lum(rgb, dtype)
    ok = valid(l)
    safe = np.where(ok, l, dtype(0.0))
    e = np.where(ok, excess(safe, threshold, knee, clamp, dtype), dtype(0.0))
    lit = ok & (e > 0)
    with np.errstate(all="ignore"):
        c = np.where(lit, e / np.where(lit, safe, dtype(1.0)), dtype(0.0)).astype(dtype)
        P = np.where(lit[..., None], rgb * c[..., None], dtype(0.0)).astype(dtype)
    return P, l, ok, lit, e


def _tap4(a, b, c, d, dtype):
    return ((dtype(0.125) * a + dtype(0.375) * b) + dtype(0.375) * c) + dtype(0.125) * d


def down(A, dtype=F):
    """D: [h, w, 3] -> [(h + 1) // 2, (w + 1) // 2, 3], the binomial {1, 3, 3, 1} / 8 in x, then in y, edge-clamped"""
    A = np.asarray(A, dtype)
    h, w = A.shape[:2]
    X, Y = np.arange((w + 1) // 2), np.arange((h + 1) // 2)
    cx = [np.clip(2 * X + o, 0, w - 1) for o in (-1, 0, 1, 2)]
    cy = [np.clip(2 * Y + o, 0, h - 1) for o in (-1, 0, 1, 2)]
    with np.errstate(all="ignore"):
        row = _tap4(A[:, cx[0]], A[:, cx[1]], A[:, cx[2]], A[:, cx[3]], dtype)
        return _tap4(row[cy[0]], row[cy[1]], row[cy[2]], row[cy[3]], dtype).astype(dtype)


def _taps(n, cn, dtype):
    """(j0, j1, a0, a1) of the n fine texels over cn coarse ones"""
    x = np.arange(n)
    i, odd = x >> 1, (x & 1) == 1
    j0 = np.where(odd, i, np.maximum(i - 1, 0))
    j1 = np.where(odd, np.minimum(i + 1, cn - 1), i)
    a0 = np.where(odd, dtype(0.75), dtype(0.25)).astype(dtype)
    a1 = np.where(odd, dtype(0.25), dtype(0.75)).astype(dtype)
    return j0, j1, a0, a1


def up(E, w, h, dtype=F):
    """U: the coarse level E [ch, cw, 3] at the size w x h of the next finer one, bilinear at the texel centres"""
    E = np.asarray(E, dtype)
    ch, cw = E.shape[:2]
    assert cw == (w + 1) // 2 and ch == (h + 1) // 2
    j0, j1, a0, a1 = _taps(w, cw, dtype)
    k0, k1, b0, b1 = _taps(h, ch, dtype)
    with np.errstate(all="ignore"):
        row = a0[None, :, None] * E[:, j0] + a1[None, :, None] * E[:, j1]
        return (b0[:, None, None] * row[k0] + b1[:, None, None] * row[k1]).astype(dtype)


def gain_of(n, intensity, spread, dtype=F):
    norm, t = dtype(1.0), dtype(1.0)
    for _ in range(n - 1):
        t = t * dtype(spread)
        norm = norm + t
    return dtype(intensity) / norm


def bloom(img, p=None, dtype=F):
    """img: float32 [h, w, 4]; p: a dict of pt_bloom_params' fields (params()).  Returns (out [h, w, 4] of dtype, info dict,
    pyramid): pyramid["down"][k - 1] is level k as the down steps leave it, pyramid["E"][k - 1] is E_k after the combine."""
    p = params() if p is None else params(**p)
    check(p)
    img = np.ascontiguousarray(img, F)
    h, w = img.shape[:2]
    sizes = levels_of(w, h, p["levels"])
    n = len(sizes)
    P, l, ok, lit, e = prefilter(img, p["threshold"], p["knee"], p["clamp"], dtype)
    D = []
    A = P
    for _ in range(n):
        A = down(A, dtype)
        D.append(A)
    assert [(a.shape[1], a.shape[0]) for a in D] == sizes
    E = [None] * n
    E[n - 1] = D[n - 1]
    with np.errstate(all="ignore"):
        for k in range(n - 2, -1, -1):
            E[k] = (D[k] + dtype(p["spread"]) * up(E[k + 1], D[k].shape[1], D[k].shape[0], dtype)).astype(dtype)
        gain = gain_of(n, p["intensity"], p["spread"], dtype)
        out = img.astype(dtype)
        out[..., :3] = img[..., :3].astype(dtype) + gain * up(E[0], w, h, dtype)
    if dtype is F:
        out.view(np.uint32)[..., 3] = img.view(np.uint32)[..., 3]
    lv = l[ok]
    info = {
        "levels": n, "bright_pixels": int(lit.sum()), "invalid_pixels": int((~ok).sum()), "reserved": 0,
        "total_luma_q16": int(q16(lv).sum(dtype=np.uint64)), "bright_luma_q16": int(q16(e[lit]).sum(dtype=np.uint64)),
        "max_luma": (float(lv.astype(F).view(np.uint32).max().view(F)) if lv.size else 0.0), "reserved2": 0,
    }
    return out, info, {"down": D, "E": E, "P": P, "gain": gain}


def bright_share(info):
    return info["bright_luma_q16"] / info["total_luma_q16"] if info["total_luma_q16"] else 0.0


def info_bits(info):
    """the record as the ten uint32 words of pt_bloom_info"""
    rec = np.zeros(10, np.uint32)
    rec[0:4] = [info["levels"], info["bright_pixels"], info["invalid_pixels"], info["reserved"]]
    rec[4:8] = np.array([info["total_luma_q16"], info["bright_luma_q16"]], np.uint64).view(np.uint32)
    rec[8] = np.array([info["max_luma"]], F).view(np.uint32)[0]
    rec[9] = info["reserved2"]
    return rec
