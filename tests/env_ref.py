"""numpy restatement of the environment map (include/acgpt.h pt_set_environment; csrc/pt_environment.h, csrc/environment.hip):
mapping, sampling weights and CDFs in the device's fp32 summation order, the sample and its pdf."""
import numpy as np

F = np.float32
INV_2PI, INV_PI, PI = F(0.159154943091895336), F(0.318309886183790672), F(3.14159265358979323846)


def block_scan(vals, threads=256):
    """environment.hip env_block_scan: thread t sums its run of ceil(n / 256) values in order, Hillis-Steele over the run sums,
    then each run's values added in order to the sum of the runs before it; normalised by the total (uniform when it is 0)."""
    vals = np.asarray(vals, F)
    n = len(vals)
    run = (n + threads - 1) // threads
    sums = np.zeros(threads, F)
    for t in range(threads):
        b, e = min(t * run, n), min(t * run + run, n)
        s = F(0)
        for v in vals[b:e]:
            s = F(s + v)
        sums[t] = s
    for off in (1, 2, 4, 8, 16, 32, 64, 128):
        old = sums.copy()
        sums[off:] = (old[off:] + old[:-off]).astype(F)
    total = sums[-1]
    out = np.zeros(n, F)
    for t in range(threads):
        b, e = min(t * run, n), min(t * run + run, n)
        acc = sums[t - 1] if t else F(0)
        for i in range(b, e):
            acc = F(acc + vals[i])
            out[i] = F(acc / total) if total > 0 else F(F(i + 1) / F(n))
    return out, total


class EnvRef:
    def __init__(self, rgb, scale=(1.0, 1.0, 1.0)):
        rgb = np.asarray(rgb, F) * np.asarray(scale, F)
        self.h, self.w = rgb.shape[:2]
        self.rgb = rgb.astype(F)
        row_sin = np.sin(np.pi * (np.arange(self.h) + 0.5) / self.h).astype(F)
        lum = ((F(0.2126) * self.rgb[..., 0] + F(0.7152) * self.rgb[..., 1]).astype(F) + F(0.0722) * self.rgb[..., 2]).astype(F)
        self.weight = (lum * row_sin[:, None]).astype(F)
        self.cond = np.zeros((self.h, self.w), F)
        row_total = np.zeros(self.h, F)
        for r in range(self.h):
            self.cond[r], row_total[r] = block_scan(self.weight[r])
        self.marg, self.total = block_scan(row_total)
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
        k = min(int(np.searchsorted(cdf, x, side="right")), len(cdf) - 1)
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
