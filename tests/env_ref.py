"""numpy restatement of the environment map (include/acgpt.h pt_set_environment; csrc/pt_environment.h, csrc/environment.hip):
mapping, sampling weights and CDFs in the device's fp32 summation order, the device's bisection of those tables (they are not sorted
across run boundaries once a run holds several values), the sample and its pdf, and the exact measure the bisection gives each bin."""
import numpy as np

F = np.float32
INV_2PI, INV_PI, PI = F(0.159154943091895336), F(0.318309886183790672), F(3.14159265358979323846)


def block_scan(vals, threads=256):
    """environment.hip env_block_scan: thread t sums its run of ceil(n / 256) values in order, Hillis-Steele over the run sums,
    then each run's values added in order to the sum of the runs before it; normalised by the total (uniform when it is 0)."""
    out, total = block_scan_rows(np.asarray(vals, F)[None, :], threads)
    return out[0], total[0]


def block_scan_rows(vals, threads=256):
    """block_scan of every row of vals [rows, n] -> (out [rows, n], totals [rows]).  The same fp32 operations in the same order, one
    numpy operation for all threads and rows at a time: a run is padded with zeros to its full length, and adding 0.0 changes no bit."""
    vals = np.asarray(vals, F)
    rows, n = vals.shape
    run = (n + threads - 1) // threads
    runs = np.zeros((rows, threads * run), F)
    runs[:, :n] = vals
    runs = runs.reshape(rows, threads, run)
    sums = np.zeros((rows, threads), F)
    for j in range(run):
        sums = sums + runs[:, :, j]
    for off in (1, 2, 4, 8, 16, 32, 64, 128):
        old = sums.copy()
        sums[:, off:] = old[:, off:] + old[:, :-off]
    total = sums[:, -1].copy()
    acc = np.zeros((rows, threads), F)
    acc[:, 1:] = sums[:, :-1]
    out = np.zeros((rows, threads, run), F)
    safe = np.where(total > 0, total, F(1))[:, None]
    for j in range(run):
        acc = acc + runs[:, :, j]
        out[:, :, j] = acc / safe
    assert sums.dtype == F and acc.dtype == F and out.dtype == F
    out = out.reshape(rows, threads * run)[:, :n].copy()
    black = ~(total > 0)
    if black.any():
        out[black] = (np.arange(1, n + 1, dtype=F) / F(n)).astype(F)
    return out, total


def search(cdf, x):
    """pt_environment.h env_search, step for step: the bisection lo = 0, hi = n - 1, mid = (lo + hi) >> 1, hi = mid where cdf[mid] > x
    and lo = mid + 1 where not.  On a sorted table this is the first index with cdf[k] > x (n - 1 if none).  The tables are not sorted
    across run boundaries once a run holds more than one value (block_scan), and there the bin is whatever this walk arrives at."""
    lo, hi = 0, len(cdf) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if cdf[mid] > x:
            hi = mid
        else:
            lo = mid + 1
    return lo


def search_many(cdf, x):
    """search() for an array of x at once"""
    cdf = np.asarray(cdf)
    x = np.asarray(x, np.float64)
    lo = np.zeros(x.shape, np.int64)
    hi = np.full(x.shape, len(cdf) - 1, np.int64)
    while True:
        active = lo < hi
        if not active.any():
            return lo
        mid = (lo + hi) >> 1
        gt = cdf[mid].astype(np.float64) > x
        hi = np.where(active & gt, mid, hi)
        lo = np.where(active & ~gt, mid + 1, lo)


def selection_measure(cdf):
    """The exact (Lebesgue) measure of the x in [0, 1) that search() sends to each bin, float64 [n].  Every comparison of the walk is
    cdf[mid] > x, so between two consecutive distinct table values the walk is the same for every x: one walk per such interval, from
    its left end (an interval is closed on the left: cdf[mid] > x holds for x = v exactly where it holds just above v, up to the next
    table value).  O(n log n)."""
    cdf = np.asarray(cdf, F)
    v = np.unique(cdf.astype(np.float64))
    edges = np.concatenate([[0.0], v[(v > 0.0) & (v < 1.0)], [1.0]])
    k = search_many(cdf, edges[:-1])
    m = np.zeros(len(cdf), np.float64)
    np.add.at(m, k, np.diff(edges))
    return m


def decreasing_steps(cdf):
    """how many i have cdf[i] < cdf[i - 1], along the last axis"""
    cdf = np.asarray(cdf, F)
    return int((np.diff(cdf, axis=-1) < 0).sum())


class EnvRef:
    def __init__(self, rgb, scale=(1.0, 1.0, 1.0)):
        rgb = np.asarray(rgb, F) * np.asarray(scale, F)
        self.h, self.w = rgb.shape[:2]
        self.rgb = rgb.astype(F)
        row_sin = np.sin(np.pi * (np.arange(self.h) + 0.5) / self.h).astype(F)
        lum = ((F(0.2126) * self.rgb[..., 0] + F(0.7152) * self.rgb[..., 1]).astype(F) + F(0.0722) * self.rgb[..., 2]).astype(F)
        self.weight = (lum * row_sin[:, None]).astype(F)
        self.cond, self.row_total = block_scan_rows(self.weight)
        self.marg, self.total = block_scan(self.row_total)
        self.pdf_scale = F(self.w * self.h / (2.0 * np.pi * np.pi * float(self.total))) if self.total > 0 else F(0)

    # ---- mapping ------------------------------------------------------------------------------------------------------
    def uv(self, d):
        d = np.asarray(d, F)
        u = (F(0.5) + np.arctan2(d[..., 0], -d[..., 2]).astype(F) * INV_2PI).astype(F)
        v = (np.arccos(np.clip(d[..., 1], -1, 1)).astype(F) * INV_PI).astype(F)
        return u, v

    def texel(self, d):
        u, v = self.uv(d)
        col = np.clip((u * F(self.w)).astype(np.int64), 0, self.w - 1)
        row = np.clip((v * F(self.h)).astype(np.int64), 0, self.h - 1)
        return row, col

    def edge_distance(self, d):
        """angular distance (radians, approximate) from d to the nearest texel edge: where the device may round to the neighbour"""
        u, v = self.uv(d)
        du = np.abs(u.astype(np.float64) * self.w - np.round(u.astype(np.float64) * self.w)) / self.w * 2 * np.pi
        dv = np.abs(v.astype(np.float64) * self.h - np.round(v.astype(np.float64) * self.h)) / self.h * np.pi
        s = np.sqrt(np.maximum(0.0, 1.0 - np.asarray(d, np.float64)[..., 1] ** 2))
        return np.minimum(du * s, dv)

    def eval(self, d):
        row, col = self.texel(d)
        return self.rgb[row, col]

    def pdf(self, d):
        d = np.asarray(d, F)
        row, col = self.texel(d)
        y = d[..., 1]
        s = np.sqrt(np.maximum(F(0), ((F(1) - y) * (F(1) + y)).astype(F))).astype(np.float64)     # sin(theta) from d.y in fp32, as the device
        w = self.weight[row, col].astype(np.float64)
        return np.where(s > 0, w * float(self.pdf_scale) / np.where(s > 0, s, 1), 0.0)

    # ---- sampling -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _pick(cdf, x):
        k = search(cdf, x)
        c0 = float(cdf[k - 1]) if k else 0.0
        c1 = float(cdf[k])
        f = (x - c0) / (c1 - c0) if c1 > c0 else 0.5
        return k, min(max(f, 0.0), 0.99999994)

    def sample(self, u1, u2):
        """(u1, u2) -> (direction, solid-angle pdf, (row, col), the bin offsets)"""
        row, fv = self._pick(self.marg, u1)
        col, fu = self._pick(self.cond[row], u2)
        u, v = (col + fu) / self.w, (row + fv) / self.h
        th, ph = np.pi * v, 2 * np.pi * (u - 0.5)
        st = max(np.sin(th), 0.0)
        d = np.array([st * np.sin(ph), np.cos(th), -st * np.cos(ph)])
        pdf = float(self.weight[row, col]) * float(self.pdf_scale) / st if st > 0 else 0.0
        return d, pdf, (row, col), (fv, fu)


def sphere_directions(n, seed=0):
    r = np.random.default_rng(seed)
    d = r.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
