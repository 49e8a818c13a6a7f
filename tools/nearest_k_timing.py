#!/usr/bin/env python3
"""Times the K-closest and within-radius queries (pt_query_nearest_k, pt_query_within_any) on the Cornell box and prints ONE JSON line
(also written to --out, default profiles/nearest_k_timing.json).

Per size n, the points are the cell centres of a grid of n cells over the scene box, x fastest (`coherent`), and the same points in
a fixed random permutation (`permuted`).  Host wall time of each call (every one returns synchronised; one process, a warm-up call,
the median of --repeats):
    k1, k4, k8              pt_query_nearest_k without counts, max_radius = +inf: the walk cut at entry max_k - 1
    k8_counts_r2, _r8       max_k = 8 with counts at a radius of 2 % and 8 % of the scene box's diagonal: nothing pruned at a candidate
    within_r2, within_r8    pt_query_within_any at those radii
    nearest                 the scale: pt_query_nearest on the same points, max_radius = +inf; k1 is the same walk, reported as a ratio
    nearest_r2, nearest_r8  pt_query_nearest at the two radii: what pt_query_within_any replaces
and, from the counting twin (pt_debug_nearest_k_visits), per form the mean and the largest number of inner nodes visited and
triangles tested per query, with the twin's records, counts and bytes checked against the product kernels'.

    python tools/nearest_k_timing.py [--sizes 262144,2073600] [--repeats 30] [--out profiles/nearest_k_timing.json]
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
    ap.add_argument("--sizes", default="262144,2073600")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_k_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "nearest_k_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    try:
        info = pt.getBvhInfo(state)
        lo, hi = np.array([float(x) for x in info.scene_lo], np.float32), np.array([float(x) for x in info.scene_hi], np.float32)
        diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
        radii = {"inf": np.inf, "r2": 0.02 * diag, "r8": 0.08 * diag}
        for size in a.sizes.split(","):
            n = int(size)
            bufs = []
            try:
                for nbytes in (n * 16, n * 8 * 32, n * 8 * 32, n * 4, n * 4, n, n, n * 8):
                    q = C.c_void_p()
                    assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0
                    bufs.append(q.value)
                d_points, d_out, d_out2, d_counts, d_counts2, d_hit, d_hit2, d_visits = bufs

                def timed(fn):
                    assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
                    ts = []
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        rc = fn()
                        ts.append((time.perf_counter() - t0) * 1e3)
                        assert rc == 0, L.pt_last_error(state.context)
                    return float(np.median(ts)), float(np.percentile(ts, 75) - np.percentile(ts, 25))

                def read(ptr, shape, dtype):
                    x = np.zeros(shape, dtype)
                    assert L.pt_copy_to_host(state.context, x.ctypes.data, ptr, x.nbytes) == 0
                    return x

                shape = grid_shape(n)
                cells = pt.distanceFieldPoints(shape, lo.tolist(), hi.tolist())
                orders = {"coherent": cells, "permuted": cells[np.random.default_rng(1).permutation(n)]}
                result = {}
                for order, pts in orders.items():
                    ms, iqr, visits, answers = {}, {}, {}, {}

                    def upload(radius):
                        p = np.empty((n, 4), np.float32)
                        p[:, 0:3], p[:, 3] = pts, radius
                        assert L.pt_copy_to_device(state.context, d_points, p.ctypes.data, p.nbytes) == 0

                    def twin(key, k, counts, within=False):
                        """the counting twin of the form just timed, its answers checked against the product kernel's in d_out / d_counts / d_hit"""
                        rc = L.pt_debug_nearest_k_visits(state.context, d_points, n, k, None if within else d_out2, d_counts2 if counts else None,
                                                         d_hit2 if within else None, d_visits)
                        assert rc == 0, L.pt_last_error(state.context)
                        if within:
                            assert np.array_equal(read(d_hit, n, np.uint8), read(d_hit2, n, np.uint8)), "the counting twin's bytes differ"
                        else:
                            assert np.array_equal(read(d_out, (n, k, 8), np.uint32), read(d_out2, (n, k, 8), np.uint32)), "the counting twin's records differ"
                        if counts:
                            assert np.array_equal(read(d_counts, n, np.uint32), read(d_counts2, n, np.uint32)), "the counting twin's counts differ"
                        v = read(d_visits, (n, 2), np.uint32)
                        visits[key] = {"nodes_mean": round(float(v[:, 0].mean()), 2), "triangles_mean": round(float(v[:, 1].mean()), 2),
                                       "nodes_max": int(v[:, 0].max()), "triangles_max": int(v[:, 1].max())}

                    upload(radii["inf"])
                    ms["nearest"], iqr["nearest"] = timed(lambda: L.pt_query_nearest(state.context, d_points, n, d_out))
                    for k in (1, 4, 8):
                        key = "k%d" % k
                        ms[key], iqr[key] = timed(lambda: L.pt_query_nearest_k(state.context, d_points, n, k, d_out, None))
                        twin(key, k, False)
                    for rk in ("r2", "r8"):
                        upload(radii[rk])
                        ms["nearest_" + rk], iqr["nearest_" + rk] = timed(lambda: L.pt_query_nearest(state.context, d_points, n, d_out))
                        key = "k8_counts_" + rk
                        ms[key], iqr[key] = timed(lambda: L.pt_query_nearest_k(state.context, d_points, n, 8, d_out, d_counts))
                        twin(key, 8, True)
                        c = read(d_counts, n, np.uint32)
                        answers[rk] = {"found_share": round(float((c != 0).mean()), 4), "count_mean": round(float(c.mean()), 2), "count_max": int(c.max()),
                                       "more_than_8_share": round(float((c > 8).mean()), 4)}
                        key = "within_" + rk
                        ms[key], iqr[key] = timed(lambda: L.pt_query_within_any(state.context, d_points, n, d_hit))
                        twin(key, 0, False, within=True)
                        assert np.array_equal(read(d_hit, n, np.uint8) != 0, c != 0), "the byte and the count disagree"
                    result[order] = {
                        "ms": {k: round(v, 4) for k, v in ms.items()}, "interquartile_ms": {k: round(v, 4) for k, v in iqr.items()},
                        "mqueries_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                        "visits": visits, "answers": answers,
                        "k1_over_nearest": round(ms["k1"] / ms["nearest"], 3),
                        "over_nearest": {k: round(ms[k] / ms["nearest"], 3) for k in ("k4", "k8")},
                        "within_over_nearest_at_radius": {rk: round(ms["within_" + rk] / ms["nearest_" + rk], 3) for rk in ("r2", "r8")},
                        "k8_counts_over_nearest_at_radius": {rk: round(ms["k8_counts_" + rk] / ms["nearest_" + rk], 3) for rk in ("r2", "r8")},
                    }
                out["sizes"].append({"queries": n, "grid": list(shape), "triangles": int(info.n_tris), "stack_entries": int(info.stack_entries),
                                     "radius_r2": round(radii["r2"], 4), "radius_r8": round(radii["r8"], 4), "orders": result,
                                     "permuted_over_coherent": {k: round(result["permuted"]["ms"][k] / result["coherent"]["ms"][k], 3) for k in result["coherent"]["ms"]}})
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
