#!/usr/bin/env python3
"""Times the triangle-to-mesh distance query (pt_query_triangle_distance) on the Cornell box and prints ONE JSON line (also written to
--out, default profiles/tridist_timing.json).

Per size n, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of --repeats), all
with max_radius = +inf:
    small            triangles whose second and third vertex lie 2 % of the scene box's diagonal from the first in fixed random
                     directions, the first at the cell centres of a grid of n cells over the scene box, x fastest
    large            three vertices uniform in the scene box (no coherent order exists)
    segments_*       what a caller did before this query: pt_query_segments on the 3 n edges of the same triangles, in the same order
                     (it misses a scene edge that pierces the query's face and a scene vertex over it)
    any_*            pt_query_triangles_any on the same triangles: the yes / no answer
and, from the counting twin of the kernel (pt_debug_triangle_distance_visits), per set with the walk's second box bound — the
separation along the query triangle's normal — on and off: the mean and the largest number of inner nodes visited and triangles
tested per query, and the twin's own time.  The twin with the bound off still forms the normal (its coefficients are zero), so its
time is an upper bound of a kernel without it.

    python tools/tridist_timing.py [--sizes 262144,2000000] [--repeats 20] [--out profiles/tridist_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nearest_timing import grid_shape          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="262144,2000000")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tridist_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "tridist_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    try:
        info = pt.getBvhInfo(state)
        lo, hi = np.array([float(x) for x in info.scene_lo], np.float32), np.array([float(x) for x in info.scene_hi], np.float32)
        diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
        for size in a.sizes.split(","):
            n = int(size)
            bufs = []
            try:
                for nbytes in (n * 48, n * 96, n * 96, n * 8):          # triangles, their 3 n edges, records (of either query), visit counts
                    q = C.c_void_p()
                    assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0
                    bufs.append(q.value)
                d_tris, d_segs, d_out, d_visits = bufs

                def timed(fn):
                    assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
                    ts = []
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        rc = fn()
                        ts.append((time.perf_counter() - t0) * 1e3)
                        assert rc == 0, L.pt_last_error(state.context)
                    return float(np.median(ts))

                rng = np.random.default_rng(7)
                shape = grid_shape(n)
                start = pt.distanceFieldPoints(shape, lo.tolist(), hi.tolist())[:n]
                m = start.shape[0]
                assert m == n, (m, n, shape)

                def unit():
                    d = rng.normal(size=(n, 3)).astype(np.float32)
                    return d * (np.float32(0.02 * diag) / np.sqrt((d * d).sum(axis=1, keepdims=True)))

                ext = hi - lo
                sets = {"small": np.stack([start, start + unit(), start + unit()], axis=1).astype(np.float32),
                        "large": np.stack([lo + rng.random((n, 3)).astype(np.float32) * ext for _ in range(3)], axis=1).astype(np.float32)}
                ms, visits, answers = {}, {}, {}
                for name, tri in sets.items():
                    g = np.zeros((n, 3, 4), np.float32)
                    g[:, :, :3] = tri
                    g[:, 0, 3] = np.inf
                    edges = np.zeros((n, 3, 8), np.float32)
                    for k, (p, q) in enumerate(((0, 1), (0, 2), (1, 2))):
                        edges[:, k, 0:3], edges[:, k, 3], edges[:, k, 4:7] = tri[:, p], np.inf, tri[:, q]
                    assert L.pt_copy_to_device(state.context, d_tris, g.ctypes.data, g.nbytes) == 0
                    assert L.pt_copy_to_device(state.context, d_segs, edges.ctypes.data, edges.nbytes) == 0
                    ms["segments_" + name] = timed(lambda: L.pt_query_segments(state.context, d_segs, 3 * n, d_out))
                    seg = np.zeros((n, 3, 8), np.float32)
                    assert L.pt_copy_to_host(state.context, seg.ctypes.data, d_out, seg.nbytes) == 0
                    ms["any_" + name] = timed(lambda: L.pt_query_triangles_any(state.context, d_tris, n, d_out))
                    ms[name] = timed(lambda: L.pt_query_triangle_distance(state.context, d_tris, n, d_out))
                    rec = np.zeros((n, 12), np.float32)
                    assert L.pt_copy_to_host(state.context, rec.ctypes.data, d_out, rec.nbytes) == 0
                    visits[name] = {}
                    for flag, key in ((0, "plane_on"), (1, "plane_off")):
                        t = timed(lambda: L.pt_debug_triangle_distance_visits(state.context, d_tris, n, d_out, d_visits, flag))
                        counts = np.zeros((n, 2), np.uint32); rec2 = np.zeros((n, 12), np.float32)
                        assert L.pt_copy_to_host(state.context, counts.ctypes.data, d_visits, counts.nbytes) == 0
                        assert L.pt_copy_to_host(state.context, rec2.ctypes.data, d_out, rec2.nbytes) == 0
                        assert np.array_equal(rec2.view(np.uint32), rec.view(np.uint32)), "the counting twin's records differ"
                        visits[name][key] = {"twin_ms": round(t, 4), "nodes_mean": round(float(counts[:, 0].mean()), 2), "triangles_mean": round(float(counts[:, 1].mean()), 2),
                                             "nodes_max": int(counts[:, 0].max()), "triangles_max": int(counts[:, 1].max())}
                    feat = rec[:, 2].astype(np.int64)
                    group = np.searchsorted(np.array([3, 6, 15, 18]), feat, side="right")
                    by_edges = seg[:, :, 0].min(axis=1)
                    answers[name] = {"found_share": round(float((rec.view(np.uint32)[:, 1] != 0xFFFFFFFF).mean()), 4), "distance_median": round(float(np.median(rec[:, 0])), 6),
                                     "distance_0_share": round(float((rec[:, 0] == 0).mean()), 4),
                                     "group_shares": [round(float((group == k).mean()), 4) for k in range(5)],
                                     # what the three segment calls get wrong: a positive distance for an intersecting pair, a larger distance
                                     "edges_miss_an_intersection_share": round(float(((rec[:, 0] == 0) & (by_edges > 0)).mean()), 4),
                                     "edges_farther_share": round(float((by_edges > rec[:, 0]).mean()), 4)}
                out["sizes"].append({
                    "queries": n, "grid": list(shape), "triangles": int(info.n_tris), "stack_entries": int(info.stack_entries),
                    "ms": {k: round(v, 4) for k, v in ms.items()},
                    "mqueries_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                    "visits": visits, "answers": answers,
                    "over_three_segment_calls": {k: round(ms[k] / ms["segments_" + k], 3) for k in sets},
                    "over_triangles_any": {k: round(ms[k] / ms["any_" + k], 3) for k in sets},
                    "plane_off_over_on_twin": {k: round(visits[k]["plane_off"]["twin_ms"] / visits[k]["plane_on"]["twin_ms"], 3) for k in sets},
                })
            finally:
                for b in bufs:
                    L.pt_device_free(state.context, b)
    finally:
        pt.CleanAllTheThings(state)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
