"""NumPy statement of pt_query_nearest_k and pt_query_within_any (include/acgpt.h): the brute force over every pair of a point and a
triangle that the GPU's records, counts and bytes are held to, bit for bit.

d2 is nearest_ref.closest_on_triangle, the fp32 statement pt_query_nearest uses; a triangle is a candidate iff d2 <= max_radius *
max_radius in fp32 (a NaN d2 is none); the list is the candidates under a stable sort on d2, so equal d2 goes to the lower triangle
index; each record is built exactly as nearest_ref.nearest_records builds its one.  The point sets are nearest_ref's; the radii of
these tests are their own (K_RADIUS), chosen so that the sets split into points with no candidate, with fewer than eight, and with
more than eight (tests/test_nearest_k_host.py holds that by this brute force alone)."""
import numpy as np

import nearest_ref as nr

F = np.float32
MAX_K = 8                                 # PT_QUERY_NEAREST_MAX
MISS_PRIM = nr.MISS_PRIM

# in units of the scene box's diagonal
K_RADIUS = {"surface": 1e-4, "inside": 0.08, "shell": 9.93, "features": 0.005, "wall_planes": 0.06}


def set_radius(name, verts, idx):
    lo, hi = nr.scene_box(verts, idx)
    ext = hi - lo
    return F(K_RADIUS[name]) * F(np.sqrt(float((ext * ext).sum())))


def miss_lists(n, k):
    """n lists of k miss records, uint32 [n, k, 8]"""
    return np.broadcast_to(nr.miss_records(1)[0], (n, k, 8)).copy()


def _sorted_candidates(d2, cand, kk):
    """The first kk candidates of every row in ascending (d2, triangle index) — the order a stable sort on d2 leaves them in — as
    (order int64 [rows, kk], kept bool [rows, kk]).  d2 is a sum of squares, never negative, so its bits order as it does, +inf (a
    candidate under max_radius = +inf) included; one 64-bit key per pair, {d2's bits, index}, all ones in the upper word for "no
    candidate", lets a partition find the first kk without sorting the row."""
    key = (np.where(cand, d2.view(np.uint32), np.uint32(0xFFFFFFFF)).astype(np.uint64) << np.uint64(32)) | np.arange(d2.shape[1], dtype=np.uint64)[None]
    if kk < key.shape[1]:
        key = np.partition(key, kk - 1, axis=1)[:, :kk]
    key = np.sort(key, axis=1)
    return (key & np.uint64(0xFFFFFFFF)).astype(np.int64), (key >> np.uint64(32)) != np.uint64(0xFFFFFFFF)


def _nearest_k(p, r2_of, verts, idx, mat_ids, k, chunk):
    """The brute force for one set of points (p [n, 4]; its fourth column decides `searchable`) under each of the squared radii
    r2_of(rows) -> list of float32 [rows]: the distances are computed once and read once per radius."""
    n = p.shape[0]
    n_radii = len(r2_of(slice(0, 0)))
    outs = [(miss_lists(n, k), np.zeros(n, np.uint32), np.full((n, k), np.inf, np.float32)) for _ in range(n_radii)]
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    n_tris = v0.shape[0]
    if n_tris and n:
        mats = np.asarray(mat_ids, np.uint32)
        ok = nr.searchable(p)
        kk = min(k, n_tris)
        chunk = chunk or max(1, min(2048, 1_000_000 // n_tris))
        for start in range(0, n, chunk):
            sl = slice(start, min(n, start + chunk))
            with np.errstate(all="ignore"):
                d2, v, w, c = nr.closest_on_triangle(p[sl, None, 0:3], v0[None], e1[None], e2[None])
            d2 = np.ascontiguousarray(d2, np.float32)
            for (rec, counts, d2_kept), r2 in zip(outs, r2_of(sl)):
                with np.errstate(invalid="ignore"):
                    cand = (d2 <= r2[:, None]) & ok[sl, None]
                counts[sl] = cand.sum(axis=1)
                order, kept = _sorted_candidates(d2, cand, kk)
                rows = np.arange(order.shape[0])[:, None]
                out = np.zeros(order.shape + (8,), np.float32)
                with np.errstate(all="ignore"):
                    out[..., 0] = np.sqrt(d2[rows, order])
                out[..., 2] = v[rows, order]
                out[..., 3] = w[rows, order]
                out[..., 4:7] = c[rows, order]
                out = out.view(np.uint32)
                out[..., 1] = order.astype(np.uint32)
                out[..., 7] = mats[order] & nr.SHADE_MAT_MASK
                sub = rec[sl, :kk]
                sub[kept] = out[kept]
                d2_kept[sl, :kk] = np.where(kept, d2[rows, order], F(np.inf))
    return [(rec, counts, (counts != 0).astype(np.uint8), d2_kept) for rec, counts, d2_kept in outs]


def nearest_k(points, verts, idx, mat_ids, k=MAX_K, chunk=None, return_d2=False):
    """(records uint32 [n, k, 8], counts uint32 [n], hit uint8 [n]) by brute force.  records[i, j]: pt_nearest of the j-th candidate of
    point i in ascending (d2, prim), the miss record past the last; the lists for a smaller k are records[:, :k].  counts: the number of
    candidates, not clamped.  hit: counts != 0.  return_d2: also the fp32 d2 of every listed entry, float32 [n, k], +inf past the last
    (what the tests of ties look at)."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 4))
    with np.errstate(all="ignore"):
        r2 = p[:, 3] * p[:, 3]
    got = _nearest_k(p, lambda sl: [r2[sl]], verts, idx, mat_ids, k, chunk)[0]
    return got if return_d2 else got[:3]


def nearest_k_radii(points, radii, verts, idx, mat_ids, k=MAX_K, chunk=None):
    """nearest_k of the (n, 3) points under each of the radii (one number each, none of them negative or a NaN), the distances
    computed once: a list of (records, counts, hit)"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r2s = [F(r) * F(r) for r in radii]
    assert all(F(r) >= 0 for r in radii)
    got = _nearest_k(nr.with_radius(pts, 0.0), lambda sl: [np.full(len(range(*sl.indices(pts.shape[0]))), r2, np.float32) for r2 in r2s], verts, idx, mat_ids, k, chunk)
    return [g[:3] for g in got]


def nearest_k_of_scene(obj, points, k=MAX_K, **kw):
    return nearest_k(points, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), k=k, **kw)


def all_d2(points, verts, idx):
    """(d2 float32 [n, n_tris] with NaN where the triangle is no candidate, for searchable points) — the whole matrix, for the tests
    that look past entry 8"""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 4))
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    with np.errstate(all="ignore"):
        d2 = nr.closest_on_triangle(p[:, None, 0:3], v0[None], e1[None], e2[None])[0]
        cand = (d2 <= (p[:, 3] * p[:, 3])[:, None]) & nr.searchable(p)[:, None]
    return np.where(cand, d2, F(np.nan)).astype(np.float32)


def classes(counts):
    """The shares of a set by the number of candidates: (none, 1 to 7, exactly 8, more than 8)"""
    c = np.asarray(counts)
    return float((c == 0).mean()), float(((c >= 1) & (c <= 7)).mean()), float((c == 8).mean()), float((c > 8).mean())


def tie_at_the_cut(points, verts, idx):
    """The share of points whose sorted candidates tie exactly between entries 7 and 8 (the last kept of a list of 8 and the first
    dropped)"""
    d2 = np.sort(np.where(np.isnan(x := all_d2(points, verts, idx)), F(np.inf), x), axis=1)
    if d2.shape[1] < 9:
        return 0.0
    return float(((d2[:, 7] == d2[:, 8]) & np.isfinite(d2[:, 8])).mean())
