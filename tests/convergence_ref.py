"""NumPy statement of pt_convergence_update (include/acgpt.h): West's weighted update per pixel, the error, the reductions.  Every
floating-point value is float32 and every operation is written once, in the order the header and csrc/convergence.hip write it; the
reductions are integer arithmetic (Python ints) or a max of bit patterns."""
import numpy as np

F = np.float32
BINS = 256
TILE = 16
BIN_BASE = 824                      # bits(2^-24) >> 20
MAX_FRAMES = 1 << 24

DEFAULTS = dict(lum_floor=0.01, threshold=0.02, quantile_permille=950)


def params(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def lum(rgb):
    """0.2126 r + 0.7152 g + 0.0722 b, left to right (pt_denoise's l); rgb: float32 [..., >= 3]"""
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def bin_index(err):
    """histogram bin of every error: clamp((bits >> 20) - 824, 0, 255)"""
    return np.clip((bits(err).astype(np.int64) >> 20) - BIN_BASE, 0, BINS - 1)


def bin_upper_edge(j):
    return np.array([(BIN_BASE + int(j) + 1) << 20], np.uint32).view(F)[0]


def quantile_bin(hist, permille):
    """(r, j): the rank and the first bin whose inclusive prefix count reaches it; j is None for an empty histogram"""
    n = int(np.sum(hist, dtype=np.uint64))
    if n == 0:
        return 0, None
    r = max(1, (n * int(permille) + 999) // 1000)
    c = 0
    for j in range(BINS):
        c += int(hist[j])
        if c >= r:
            return r, j
    raise AssertionError("prefix counts never reach r")


def update_pixels(l1, state, accum_frames, lum_floor):
    """(state' float32 [n, 4], err float32 [n] with -1 where there is none, measured bool [n], invalid bool [n]) of luminances
    float32 [n] and state float32 [n, 4] = {l0, M2, k0, B}"""
    l1 = np.asarray(l1, F)
    state = np.asarray(state, F)
    l0, m2, k0, b = state[:, 0], state[:, 1], state[:, 2], state[:, 3]
    k1 = F(accum_frames)
    with np.errstate(all="ignore"):
        invalid = ~np.isfinite(l1)
        first = ~invalid & (~(k0 > 0) | ~(k1 > k0))
        measured = ~invalid & ~first
        n = k1 - k0
        d = l1 - l0
        w = (k0 * k1) / n
        m2n = m2 + w * (d * d)
        bn = b + F(1.0)
        v = m2n / ((bn - F(1.0)) * k1)
        sem = np.sqrt(v)
        err = sem / np.maximum(l1, F(lum_floor))
    out = np.zeros_like(state)
    out[first] = np.stack([l1[first], np.zeros(int(first.sum()), F), np.full(int(first.sum()), k1, F), np.ones(int(first.sum()), F)], axis=-1)
    out[measured] = np.stack([l1[measured], m2n[measured], np.full(int(measured.sum()), k1, F), bn[measured]], axis=-1)
    return out, np.where(measured, err, F(-1.0)).astype(F), measured, invalid


def reduce_errors(err, measured, n_unmeasured, n_invalid, accum_frames, cp):
    """the info record of the errors of the measured pixels"""
    e = np.asarray(err, F)[measured]
    hist = np.bincount(bin_index(e), minlength=BINS).astype(np.uint32)
    with np.errstate(all="ignore"):
        converged = int(np.count_nonzero(e <= F(cp["threshold"])))
    _, j = quantile_bin(hist, cp["quantile_permille"])
    return dict(frames=int(accum_frames), measured_pixels=int(e.size), unmeasured_pixels=int(n_unmeasured), invalid_pixels=int(n_invalid),
                converged_pixels=converged, max_error=(np.array([bits(e).max()], np.uint32).view(F)[0] if e.size else F(0.0)),
                quantile_error=(bin_upper_edge(j) if j is not None else F(0.0)), histogram=hist)


def tile_max(err, measured, w, h):
    """float32 [ceil(h/16) * ceil(w/16)]: per tile the max error bits of its measured pixels, -1 without one; tile row 0 = image row 0"""
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    key = np.zeros((ty * TILE, tx * TILE), np.int64)                 # 0: no measured pixel; else bits + 1
    key[:h, :w] = np.where(measured, bits(err).astype(np.int64) + 1, 0).reshape(h, w)
    m = key.reshape(ty, TILE, tx, TILE).max(axis=(1, 3)).ravel()
    out = np.full(m.shape, F(-1.0), F)
    out[m > 0] = (m[m > 0] - 1).astype(np.uint32).view(F)
    return out


def update(accum, state, w, h, accum_frames, cp=None):
    """(state', out_error [w*h], out_tiles, info) of an accumulation float32 [w*h, >= 3] and a state float32 [w*h, 4]"""
    cp = params() if cp is None else cp
    assert 1 <= int(accum_frames) <= MAX_FRAMES
    accum = np.asarray(accum, F).reshape(w * h, -1)
    state = np.asarray(state, F).reshape(w * h, 4)
    new, err, measured, invalid = update_pixels(lum(accum), state, accum_frames, cp["lum_floor"])
    n_inv = int(invalid.sum())
    info = reduce_errors(err, measured, w * h - int(measured.sum()) - n_inv, n_inv, accum_frames, cp)
    return new, err, tile_max(err, measured, w, h), info


def is_converged(info, permille):
    """pathtracer.Convergence.converged"""
    return info["unmeasured_pixels"] == 0 and info["invalid_pixels"] == 0 and info["converged_pixels"] * 1000 >= info["measured_pixels"] * int(permille)
