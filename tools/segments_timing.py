#!/usr/bin/env python3
"""Times the segment-to-mesh distance query (pt_query_segments) on the Cornell box and prints ONE JSON line (also written to --out,
default profiles/segments_timing.json).

Per size n, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of --repeats), all
with max_radius = +inf:
    short            segments of 2 % of the scene box's diagonal in a fixed random direction, starting at the cell centres of a grid of n
                     cells over the scene box, x fastest
    short_permuted   the same segments in a fixed random permutation: what incoherence costs
    long             both ends uniform in the scene box (no coherent order exists)
    nearest_*        the scale: pt_query_nearest on the same segments' midpoints, in the same order
and, from the counting twin of the kernel (pt_debug_segments_visits), per set with the walk's second box bound — the three axes
perpendicular to the segment — on and off: the mean and the largest number of inner nodes visited and triangles tested per query,
and the twin's own time.  The twin with the bound off still computes the three axes (their coefficients are zero), so its time is an
upper bound of a kernel without them.

    python tools/segments_timing.py [--sizes 262144,2073600] [--repeats 30] [--out profiles/segments_timing.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "segments_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    try:
        info = pt.getBvhInfo(state)
        lo, hi = np.array([float(x) for x in info.scene_lo], np.float32), np.array([float(x) for x in info.scene_hi], np.float32)
        diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
        for size in a.sizes.split(","):
            n = int(size)
            bufs = []
            try:
                for _ in range(4):          # segments, midpoints, records, visit counts
                    q = C.c_void_p()
                    assert L.pt_device_malloc(state.context, C.byref(q), n * 32) == 0
                    bufs.append(q.value)
                d_segs, d_points, d_out, d_visits = bufs

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
                start = pt.distanceFieldPoints(shape, lo.tolist(), hi.tolist())
                d = rng.normal(size=(n, 3)).astype(np.float32)
                d *= np.float32(0.02 * diag) / np.sqrt((d * d).sum(axis=1, keepdims=True))
                short = np.concatenate([start, start + d], axis=1).astype(np.float32)
                ext = hi - lo
                long_ = np.concatenate([lo + rng.random((n, 3)).astype(np.float32) * ext, lo + rng.random((n, 3)).astype(np.float32) * ext], axis=1).astype(np.float32)
                sets = {"short": short, "short_permuted": short[np.random.default_rng(1).permutation(n)], "long": long_}
                ms, visits, answers = {}, {}, {}
                for name, segs in sets.items():
                    g = np.zeros((n, 8), np.float32)
                    g[:, 0:3], g[:, 3], g[:, 4:7] = segs[:, 0:3], np.inf, segs[:, 3:6]
                    mid = np.empty((n, 4), np.float32)
                    mid[:, 0:3], mid[:, 3] = np.float32(0.5) * (segs[:, 0:3] + segs[:, 3:6]), np.inf
                    assert L.pt_copy_to_device(state.context, d_segs, g.ctypes.data, g.nbytes) == 0
                    assert L.pt_copy_to_device(state.context, d_points, mid.ctypes.data, mid.nbytes) == 0
                    ms[name] = timed(lambda: L.pt_query_segments(state.context, d_segs, n, d_out))
                    rec = np.zeros((n, 8), np.float32)
                    assert L.pt_copy_to_host(state.context, rec.ctypes.data, d_out, rec.nbytes) == 0
                    ms["nearest_" + name] = timed(lambda: L.pt_query_nearest(state.context, d_points, n, d_out))
                    visits[name] = {}
                    for flag, key in ((0, "axes_on"), (1, "axes_off")):
                        t = timed(lambda: L.pt_debug_segments_visits(state.context, d_segs, n, d_out, d_visits, flag))
                        counts = np.zeros((n, 2), np.uint32); rec2 = np.zeros((n, 8), np.float32)
                        assert L.pt_copy_to_host(state.context, counts.ctypes.data, d_visits, counts.nbytes) == 0
                        assert L.pt_copy_to_host(state.context, rec2.ctypes.data, d_out, rec2.nbytes) == 0
                        assert np.array_equal(rec2.view(np.uint32), rec.view(np.uint32)), "the counting twin's records differ"
                        visits[name][key] = {"twin_ms": round(t, 4), "nodes_mean": round(float(counts[:, 0].mean()), 2), "triangles_mean": round(float(counts[:, 1].mean()), 2),
                                             "nodes_max": int(counts[:, 0].max()), "triangles_max": int(counts[:, 1].max())}
                    feat = rec[:, 3]
                    answers[name] = {"found_share": round(float((rec.view(np.uint32)[:, 1] != 0xFFFFFFFF).mean()), 4), "distance_median": round(float(np.median(rec[:, 0])), 6),
                                     "feature_shares": [round(float((feat == k).mean()), 4) for k in range(6)]}
                out["sizes"].append({
                    "queries": n, "grid": list(shape), "triangles": int(info.n_tris), "stack_entries": int(info.stack_entries),
                    "ms": {k: round(v, 4) for k, v in ms.items()},
                    "mqueries_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                    "visits": visits, "answers": answers,
                    "over_nearest": {k: round(ms[k] / ms["nearest_" + k], 3) for k in sets},
                    "permuted_over_coherent_short": round(ms["short_permuted"] / ms["short"], 3),
                    "axes_off_over_on_twin": {k: round(visits[k]["axes_off"]["twin_ms"] / visits[k]["axes_on"]["twin_ms"], 3) for k in sets},
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
