"""pt_query_winding in NumPy (include/acgpt.h states the contract; csrc/winding.h the moments).

    exact(points, verts, idx, dtype)                       the brute force: every triangle's solid angle, summed sequentially in dtype
    moments(children, empty, records)                      the far-field moments per node, fp32 and bottom up, operation for operation
    walk(children, moments, records, points, beta, dtype)  the accept rule in fp32; the two counts per point and the sum in dtype

A triangle is what the scene's record holds: v0, e1 = v1 - v0, e2 = v2 - v0 in fp32, and its vertices are v0, v0 + e1, v0 + e2 in fp32
(the other queries' convention, nearest_ref.records_of_scene).  The arithmetic of the sum is the kernel's own within a tolerance; the
moments and the accept decisions are not: they are compared bit for bit and integer for integer."""
import numpy as np

F = np.float32
BETA_DEFAULT = 2.0              # PT_WINDING_BETA_DEFAULT


def record_vertices(records):
    """(v0, v1, v2) float32 [n, 3] of TriRecord words [n, 12]: v0, v0 + e1, v0 + e2"""
    f = np.ascontiguousarray(records, np.uint32).reshape(-1, 12).view(F)
    v0, e1, e2 = f[:, 0:3], f[:, 3:6], f[:, 6:9]
    return v0.copy(), (v0 + e1).astype(F), (v0 + e2).astype(F)


def records_of_scene(verts, idx):
    """TriRecord words [n, 12] of a scene in its own triangle order (triangle index in word 9)"""
    v = np.asarray(verts, F).reshape(-1, 4)[:, :3] if np.asarray(verts).ndim == 1 else np.asarray(verts, F)[:, :3]
    i = np.asarray(idx, np.int64).reshape(-1, 3)
    out = np.zeros((len(i), 12), np.uint32)
    f = out.view(F)
    a, b, c = v[i[:, 0]], v[i[:, 1]], v[i[:, 2]]
    f[:, 0:3], f[:, 3:6], f[:, 6:9] = a, (b - a).astype(F), (c - a).astype(F)
    out[:, 9] = np.arange(len(i), dtype=np.uint32)
    return out


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def solid_angle(q, v0, v1, v2):
    """Omega of the triangles (v0, v1, v2) [..., 3] at q [..., 3] in q's dtype (van Oosterom and Strackee)"""
    dt = q.dtype
    a, b, c = v0.astype(dt) - q, v1.astype(dt) - q, v2.astype(dt) - q
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    det = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    return (dt.type(2.0) * np.arctan2(det, den)).astype(dt)


def _finite(points):
    return np.isfinite(np.asarray(points, F)[:, :3]).all(axis=1)


def exact(points, verts, idx, dtype=np.float64):
    """w [n] in dtype: (1 / 4 pi) of the sum over every triangle, in triangle order, one accumulator per point; a NaN for a point with
    a non-finite coordinate"""
    dt = np.dtype(dtype)
    p = np.asarray(points, F)[:, :3]
    ok = _finite(p)
    q = np.where(ok[:, None], p, F(0.0)).astype(dt)
    v0, v1, v2 = record_vertices(records_of_scene(verts, idx))
    total = np.zeros(len(q), dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(len(v0)):
            total = (total + solid_angle(q, v0[t][None, :], v1[t][None, :], v2[t][None, :])).astype(dt)
    w = (total * dt.type(0.25 / np.pi)).astype(dt) if dt == np.float64 else (total * F(F(0.25) / F(np.pi))).astype(dt)
    return np.where(ok, w, dt.type(np.nan))


# ---- the moments ------------------------------------------------------------------------------------------------------------------

def triangle_sums(records):
    """per record (N [n, 3], A [n], S [n, 3], lo [n, 3], hi [n, 3]) float32: csrc/winding.h wind_triangle"""
    f = np.ascontiguousarray(records, np.uint32).reshape(-1, 12).view(F)
    v0, e1, e2 = f[:, 0:3], f[:, 3:6], f[:, 6:9]
    with np.errstate(over="ignore", invalid="ignore"):
        n2 = np.stack([(e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1]), (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2]),
                       (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])], axis=1).astype(F)
        area = (F(0.5) * np.sqrt(((n2[:, 0] * n2[:, 0] + n2[:, 1] * n2[:, 1]) + n2[:, 2] * n2[:, 2]).astype(F))).astype(F)
        c = (v0 + ((e1 + e2).astype(F) / F(3.0)).astype(F)).astype(F)
        s = (area[:, None] * c).astype(F)
    v1, v2 = (v0 + e1).astype(F), (v0 + e2).astype(F)
    return (F(0.5) * n2).astype(F), area, s, np.minimum(v0, np.minimum(v1, v2)), np.maximum(v0, np.maximum(v1, v2))


def moment_of(n, area, s, lo, hi):
    """[..., 8] float32 {p, r2, N, A} from a node's sums: csrc/winding.h wind_moment"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = np.where((area == 0)[..., None], (F(0.5) * (lo + hi).astype(F)).astype(F), (s / area[..., None]).astype(F)).astype(F)
        m = np.maximum((p - lo).astype(F), (hi - p).astype(F))
        r2 = (((m[..., 0] * m[..., 0]).astype(F) + (m[..., 1] * m[..., 1]).astype(F)).astype(F) + (m[..., 2] * m[..., 2]).astype(F)).astype(F)
    out = np.zeros(p.shape[:-1] + (8,), F)
    out[..., 0:3], out[..., 3], out[..., 4:7], out[..., 7] = p, r2, n, area
    return out


def levels_of(children, empty):
    """the inner nodes per depth, root first"""
    levels, frontier = [], np.array([0], np.int64)
    while frontier.size:
        levels.append(frontier)
        ch, live = children[frontier], ~empty[frontier]
        frontier = ch[(ch >= 0) & live].astype(np.int64)
        assert len(levels) <= children.shape[0]
    return levels


def moments(children, empty, records):
    """float32 [n_nodes, 8] {p[3], r2, N[3], A}: per node child 0 then child 1, N = N0 + N1, A = A0 + A1, S = S0 + S1, lo / hi the exact
    min / max, p = S / A (the box centre where A is 0), r2 to the farthest corner.  An empty child adds nothing: the node is its one
    live child."""
    children = np.asarray(children, np.int64)
    n = children.shape[0]
    tn, ta, ts, tlo, thi = triangle_sums(records)
    N, A, S = np.zeros((n, 3), F), np.zeros(n, F), np.zeros((n, 3), F)
    lo, hi = np.zeros((n, 3), F), np.zeros((n, 3), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for lev in reversed(levels_of(children, empty)):
            part = []
            for k in (0, 1):
                c = children[lev, k]
                leaf = c < 0
                s, j = np.where(leaf, ~c, 0), np.where(leaf, 0, c)
                pick = lambda t, a: np.where(leaf[:, None] if t.ndim == 2 else leaf, t[s], a[j])
                part.append((pick(tn, N), pick(ta, A), pick(ts, S), pick(tlo, lo), pick(thi, hi)))
            (n0, a0, s0, l0, h0), (n1, a1, s1, l1, h1) = part
            one = empty[lev, 1]
            N[lev] = np.where(one[:, None], n0, (n0 + n1).astype(F))
            A[lev] = np.where(one, a0, (a0 + a1).astype(F))
            S[lev] = np.where(one[:, None], s0, (s0 + s1).astype(F))
            lo[lev] = np.where(one[:, None], l0, np.minimum(l0, l1))
            hi[lev] = np.where(one[:, None], h0, np.maximum(h0, h1))
    return moment_of(N, A, S, lo, hi)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------

def accepts(mom, q, beta2):
    """(taken [m] bool, d2 [m] float32, dx [m, 3] float32) of one node's moment for the points q [m, 3] float32: d2 > beta2 * r2 in
    fp32 as written"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (mom[0:3][None, :] - q).astype(F)
        d2 = (((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        return d2 > F(beta2) * mom[3], d2, d


def _dipole(mom, q, dt):
    d = mom[0:3].astype(dt)[None, :] - q
    d2 = _dot(d, d)
    return _dot(mom[4:7].astype(dt)[None, :], d) / (d2 * np.sqrt(d2))


def walk(children, empty, mom, records, points, beta, dtype=np.float64):
    """(visits uint32 [n, 2] = {dipoles taken, triangles evaluated}, w [n] in dtype).  The root's moment is tested first, then every
    inner child before it is entered; leaves are always exact.  The sum runs in the order of the device's walk: a node's dipoles at
    the visit, then child 0's subtree, then child 1's.  A point with a non-finite coordinate: no traversal, a NaN."""
    dt = np.dtype(dtype)
    children = np.asarray(children, np.int64)
    p = np.asarray(points, F)[:, :3]
    ok = _finite(p)
    q32 = np.where(ok[:, None], p, F(0.0)).astype(F)
    q = q32.astype(dt)
    with np.errstate(over="ignore"):
        beta2 = F(beta) * F(beta)
    n = len(q)
    visits = np.zeros((n, 2), np.uint32)
    total = np.zeros(n, dt)
    n_tris = len(np.asarray(records).reshape(-1, 12))
    if n_tris and n:
        v0, v1, v2 = record_vertices(records)
        taken = accepts(mom[0], q32, beta2)[0] & ok
        if taken.any():
            total[taken] = _dipole(mom[0], q[taken], dt)
            visits[taken, 0] += 1
        stack = [(0, np.flatnonzero(ok & ~taken))]
        while stack:
            node, at = stack.pop()
            if at.size == 0:
                continue
            if node < 0:
                t = ~node
                with np.errstate(invalid="ignore", divide="ignore"):
                    total[at] = (total[at] + solid_angle(q[at], v0[t][None, :], v1[t][None, :], v2[t][None, :])).astype(dt)
                visits[at, 1] += 1
                continue
            enter = []
            for k in (0, 1):
                c = int(children[node, k])
                if empty[node, k]:
                    continue
                rest = at
                if c >= 0:
                    far = accepts(mom[c], q32[at], beta2)[0]
                    took = at[far]
                    if took.size:
                        total[took] = (total[took] + _dipole(mom[c], q[took], dt)).astype(dt)
                        visits[took, 0] += 1
                    rest = at[~far]
                enter.append((c, rest))
            stack.extend(reversed(enter))              # child 0 is popped first
    scale = dt.type(0.25 / np.pi) if dt == np.float64 else F(F(0.25) / F(np.pi))
    return visits, np.where(ok, (total * scale).astype(dt), dt.type(np.nan))
