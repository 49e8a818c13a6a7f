"""NumPy statement of pt_firefly_filter (include/acgpt.h): the rank rule, the clamp, the replacement of invalid pixels and the info
record.  Every floating-point value is float32 and every operation is written once, in the order the header and csrc/firefly.hip
write it; the counts and the two q16 sums are integers (the sums modulo 2^64, as the device's)."""
import numpy as np

F = np.float32
Q16_CAP = F(2.0 ** 24)
# the calibrated defaults (floor is the convergence pass's lum_floor)
DEFAULTS = dict(ratio=16.0, floor=0.01, rank=1, radius=1)


def params(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def lum(rgb):
    """(0.2126 r + 0.7152 g) + 0.0722 b; rgb: float32 [..., >= 3]"""
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


def valid(l):
    with np.errstate(all="ignore"):
        return np.isfinite(l) & (l >= 0)


def taps(radius):
    """dy outer, dx inner, both ascending, without (0, 0)"""
    return [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dx, dy) != (0, 0)]


def q16(x):
    """(uint64) trunc(min(x, 2^24) * 65536) of non-negative float32"""
    with np.errstate(all="ignore"):
        return (np.minimum(np.asarray(x, F), Q16_CAP) * F(65536.0)).astype(np.uint64)


def filter(src, ratio=None, floor=None, rank=None, radius=None):
    """src: float32 [h, w, 4].  Returns (out float32 [h, w, 4], info dict).  info holds pt_firefly_info's fields and, for the tests,
    passed_undefined: the valid pixels that passed because fewer than `rank` neighbours were valid."""
    p = params(**{k: v for k, v in dict(ratio=ratio, floor=floor, rank=rank, radius=radius).items() if v is not None})
    ratio, floor, rank, radius = F(p["ratio"]), F(p["floor"]), int(p["rank"]), int(p["radius"])
    assert np.isfinite(ratio) and ratio >= 1 and np.isfinite(floor) and floor > 0 and 1 <= rank <= 4 and radius in (1, 2)
    src = np.ascontiguousarray(src, F)
    h, w = src.shape[:2]
    l = lum(src)
    ok = valid(l)
    # the luminances with a halo; an invalid or out-of-image entry holds -1, below every valid one
    lp = np.full((h + 2 * radius, w + 2 * radius), F(-1.0), F)
    lp[radius:radius + h, radius:radius + w] = np.where(ok, l, F(-1.0))
    top = [np.full((h, w), F(-1.0), F) for _ in range(rank)]          # the `rank` largest so far, descending
    n = np.zeros((h, w), np.int32)
    for dx, dy in taps(radius):
        v = lp[radius + dy:radius + dy + h, radius + dx:radius + dx + w]
        n += v >= 0
        for k in range(rank):
            hi, v = np.maximum(top[k], v), np.minimum(top[k], v)
            top[k] = hi
    defined = n >= rank
    with np.errstate(all="ignore"):
        t = ratio * np.maximum(top[rank - 1], floor)
        clamped = ok & defined & (l > t)
        s = np.where(clamped, t / np.where(clamped, l, F(1.0)), F(1.0)).astype(F)
    out = src.copy()
    with np.errstate(all="ignore"):
        scaled = src[..., :3] * s[..., None]
    out[..., :3][clamped] = scaled[clamped]
    # invalid pixels: the mean of the valid neighbours' colours, added in tap order from 0
    bad = ~ok
    by, bx = np.nonzero(bad)
    acc = np.zeros((by.size, 3), F)
    cnt = np.zeros(by.size, np.int32)
    with np.errstate(all="ignore"):
        for dx, dy in taps(radius):
            qy, qx = by + dy, bx + dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.where(inside, qy, 0), np.where(inside, qx, 0)
            use = inside & ok[qy, qx]
            acc = acc + np.where(use[:, None], src[qy, qx, :3], F(0.0))      # a sum that started at +0 never is -0: adding +0 keeps its bits
            cnt += use
        mean = np.where(cnt[:, None] > 0, acc / np.maximum(cnt, 1).astype(F)[:, None], F(0.0)).astype(F)
    out[by, bx, :3] = mean
    out.view(np.uint32)[..., 3] = src.view(np.uint32)[..., 3]
    with np.errstate(all="ignore"):
        over = (l[clamped] / t[clamped]).astype(F)
        removed = q16(l[clamped] - t[clamped])
    info = {
        "clamped_pixels": int(clamped.sum()), "replaced_pixels": int(bad.sum()), "passed_pixels": int((ok & ~clamped).sum()), "reserved": 0,
        "total_luma_q16": int(q16(l[ok]).sum(dtype=np.uint64)), "removed_luma_q16": int(removed.sum(dtype=np.uint64)),
        "max_ratio": float(over.view(np.uint32).max().view(F)) if over.size else 0.0, "reserved2": 0,
        "passed_undefined": int((ok & ~defined).sum()),
    }
    return out, info


def removed_share(info):
    return info["removed_luma_q16"] / info["total_luma_q16"] if info["total_luma_q16"] else 0.0


INFO_FIELDS = ("clamped_pixels", "replaced_pixels", "passed_pixels", "reserved", "total_luma_q16", "removed_luma_q16", "max_ratio", "reserved2")


def info_bits(info):
    """the record as the ten uint32 words of pt_firefly_info"""
    rec = np.zeros(10, np.uint32)
    rec[0:4] = [info["clamped_pixels"], info["replaced_pixels"], info["passed_pixels"], info["reserved"]]
    rec[4:8] = np.array([info["total_luma_q16"], info["removed_luma_q16"]], np.uint64).view(np.uint32)
    rec[8] = np.array([info["max_ratio"]], F).view(np.uint32)[0]
    rec[9] = info["reserved2"]
    return rec
