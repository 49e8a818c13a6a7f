"""The reference of pt_query_multi (include/acgpt.h), all on the CPU: which triangles a ray hits inside its interval, the first of them
in ascending (t, prim), and how many there are.

Whether a triangle is a hit, and at which t, is the oracle's own brute-force tri_test — fused operations that NumPy cannot state —,
asked one triangle at a time: an oracle scene of triangle i's own three vertices with trace_closest(rays, use_bvh=False) gives the t
of triangle i alone or no hit, and that t does not depend on the other triangles of the scene.  All of a scene's rays go through each one-triangle scene
in one call.  The running first `keep` hits of every ray are merged chunk by chunk of triangles, so a 20 000-triangle scene never
holds its whole [triangles, rays] matrix.  The rest of each record is query_ref.hit_records, pt_query_closest's epilogue.

A plain module: tests/test_multihit_host.py holds it to hand-checked cases and to the oracle's closest and any hit on whole scenes,
tests/test_gpu_multihit.py holds the GPU to it."""
import numpy as np

import query_ref as qr
import query_scenes as qs

F = np.float32
MISS = 0xFFFFFFFF
KEEP = 8                                  # PT_QUERY_MULTI_MAX
CHUNK = 256                               # triangles merged into the running lists at a time
ONE = np.arange(3, dtype=np.uint32)       # the index buffer of a one-triangle scene
INERT = (0, 0, 0, 0, 0, 1, 0, 1)          # what stands in for a ray that is none when the rays go to the oracle


def first_hits(oracle, verts, idx, mat_ids, mats, rays, keep=KEEP):
    """(t [n, keep] f32, prim [n, keep] u32, count [n] u32) of the rays against the scene: column j is the ray's j-th hit in ascending
    (t, prim), {+inf, 0xFFFFFFFF} past its last; count is the number of triangles hit, not clamped.  A ray that is a miss before any
    traversal (query_ref.traceable) hits nothing."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 4)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    mat_ids = np.ascontiguousarray(mat_ids, np.uint32)
    n = rays.shape[0]
    ok = qr.traceable(rays)
    send = rays.copy()
    send[~ok] = INERT
    top_t = np.full((keep, n), np.inf, np.float32)
    top_p = np.full((keep, n), MISS, np.uint32)
    count = np.zeros(n, np.uint32)
    for a in range(0, idx.shape[0], CHUNK):
        b = min(a + CHUNK, idx.shape[0])
        ct = np.full((b - a, n), np.inf, np.float32)
        for i in range(a, b):
            sc = oracle.scene(verts[idx[i].astype(np.int64)], ONE, mat_ids[i:i + 1], mats)      # the triangle's own three vertices
            try:
                t, p = sc.trace_closest(send, use_bvh=False)
            finally:
                sc.close()
            hit = (p != MISS) & ok
            assert (p[hit] == 0).all() and not np.isinf(t[hit]).any()
            ct[i - a, hit] = t[hit]
            count += hit.astype(np.uint32)
        # the kept rows are in (t, prim) order and name lower triangles than the chunk, whose rows ascend: a stable sort by t alone
        # leaves equal t in ascending prim
        all_t = np.concatenate([top_t, ct])
        all_p = np.concatenate([top_p, np.where(np.isinf(ct), np.uint32(MISS), np.arange(a, b, dtype=np.uint32)[:, None])])
        order = np.argsort(all_t, axis=0, kind="stable")[:keep]
        top_t = np.take_along_axis(all_t, order, axis=0)
        top_p = np.take_along_axis(all_p, order, axis=0)
    return np.ascontiguousarray(top_t.T), np.ascontiguousarray(top_p.T), count


def records(rays, t, prim, max_hits, verts, idx, mat_ids):
    """pt_hit records as uint32 [n, max_hits, 8] of the first max_hits columns of first_hits' (t, prim): query_ref.hit_records per
    column, the miss record past a ray's last hit"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    out = np.zeros((rays.shape[0], max_hits, 8), np.uint32)
    for j in range(max_hits):
        tj = np.where(prim[:, j] != MISS, t[:, j], F(-1.0)).astype(np.float32)
        out[:, j] = qr.hit_records(rays, tj, prim[:, j], verts, idx, mat_ids)
    return out


class Reference:
    """first_hits of one ray array against one scene, computed once: .rays, .t, .prim, .count, and records(max_hits, rows)"""

    def __init__(self, oracle, verts, idx, mat_ids, mats, rays):
        self.rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        self._scene = (verts, idx, mat_ids)
        self.t, self.prim, self.count = first_hits(oracle, verts, idx, mat_ids, mats, self.rays)
        self._rec = records(self.rays, self.t, self.prim, KEEP, verts, idx, mat_ids)
        for a in (self.rays, self.t, self.prim, self.count, self._rec):
            a.setflags(write=False)

    def records(self, max_hits, rows=slice(None)):
        return self._rec[rows, :max_hits]

    def part(self, a, b):
        """The reference of rays a .. b alone (a ray's answer does not depend on the others)"""
        r = object.__new__(Reference)
        r.rays, r.t, r.prim, r.count, r._rec, r._scene = self.rays[a:b], self.t[a:b], self.prim[a:b], self.count[a:b], self._rec[a:b], self._scene
        return r


_cache = {}


def scene_reference(oracle, name):
    """set name -> Reference of query_scenes.ray_sets(name) on scene `name`; every set goes through each one-triangle scene in one call"""
    if name not in _cache:
        v, idx, ids, mats = qs.SCENES[name].arrays()
        sets = qs.ray_sets(name)
        whole = Reference(oracle, v, idx, ids, mats, np.concatenate(list(sets.values())))
        out, a = {}, 0
        for k, rays in sets.items():
            out[k] = whole.part(a, a + len(rays))
            a += len(rays)
        _cache[name] = out
    return _cache[name]


# ---- a closed mesh ---------------------------------------------------------------------------------------------------------------

def icosphere(subdiv, centre, radius):
    """(verts [n, 4] f32, idx [t, 3] u32) of an icosphere, 20 * 4^subdiv triangles with shared vertices, outward winding: closed"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [tuple(np.array(p, np.float64) / np.linalg.norm(p)) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = (np.array(v[a]) + np.array(v[b])) / 2.0
                v.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.zeros((len(v), 4), np.float32)
    verts[:, :3] = (np.array(centre, np.float64) + radius * np.array(v, np.float64)).astype(np.float32)
    return verts, np.array(f, np.uint32)


def shell_points(n, centre, radius, seed=909):
    """n points around the centre, float32 [n, 3]: the first half at radii in [0, 0.95 R], the rest in [1.02 R, 2 R], and which are the
    first half (inside the icosphere of that radius, whose faces sag less than 0.01 R below the sphere from subdivision 2 on)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = np.arange(n) < n // 2
    r = np.where(inside, rng.uniform(0.0, 0.95, n), rng.uniform(1.02, 2.0, n)) * radius
    return (np.array(centre, np.float64) + d * r[:, None]).astype(np.float32), inside
