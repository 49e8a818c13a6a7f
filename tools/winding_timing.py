#!/usr/bin/env python3
"""Times the generalised winding number (pt_query_winding) on the Cornell box and prints ONE JSON line (also written to --out,
default profiles/winding_timing.json).

Per size n, the points are the cell centres of a grid of n cells over the scene box, x fastest (`coherent`), and the same points in
a fixed random permutation (`permuted`).  Host wall time of each call (every one returns synchronised; one process, a warm-up call,
the median of --repeats with the interquartile range):
    beta2, beta3, exact     pt_query_winding at beta = 2, 3 and +inf
    nearest                 the scale: pt_query_nearest on the same points, max_radius = +inf
    parity3                 what pointsInside(method="parity") costs on the device: pt_query_multi, counts alone, three rays per point
and, from the counting twin (pt_debug_winding_visits, its values checked against the product kernel's bits), the mean and the largest
number of dipoles taken and triangles evaluated per point; the first call's time with the moment build in it, taken once on a fresh
scene; and the largest difference of each beta's answer from the exact sum's.

    python tools/winding_timing.py [--sizes 262144,2073600] [--repeats 30] [--out profiles/winding_timing.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "winding_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    try:
        info = pt.getBvhInfo(state)
        lo, hi = np.array([float(x) for x in info.scene_lo], np.float32), np.array([float(x) for x in info.scene_hi], np.float32)
        betas = {"beta2": 2.0, "beta3": 3.0, "exact": float("inf")}
        directions = np.asarray(pt.INSIDE_DIRECTIONS, np.float32)
        first = True
        for size in a.sizes.split(","):
            n = int(size)
            bufs = []
            try:
                for nbytes in (n * 16, n * 4, n * 4, n * 8, n * 32, n * 3 * 32, n * 3 * 4):
                    q = C.c_void_p()
                    assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0
                    bufs.append(q.value)
                d_points, d_out, d_out2, d_visits, d_near, d_rays, d_counts = bufs

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
                    p = np.empty((n, 4), np.float32)
                    p[:, 0:3], p[:, 3] = pts, np.inf
                    assert L.pt_copy_to_device(state.context, d_points, p.ctypes.data, p.nbytes) == 0
                    rays = np.empty((n, 3, 8), np.float32)
                    rays[:, :, 0:3], rays[:, :, 3:6], rays[:, :, 6], rays[:, :, 7] = pts[:, None, :], directions[None, :, :], 0.0, np.inf
                    assert L.pt_copy_to_device(state.context, d_rays, rays.ctypes.data, rays.nbytes) == 0
                    del rays
                    if first:       # the first call on the scene builds the moments
                        assert not pt.getWindingInfo(state)["built"]
                        t0 = time.perf_counter()
                        assert L.pt_query_winding(state.context, d_points, 1, 2.0, d_out) == 0, L.pt_last_error(state.context)
                        out["first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
                        t0 = time.perf_counter()
                        assert L.pt_query_winding(state.context, d_points, 1, 2.0, d_out) == 0
                        out["second_call_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
                        out["moments"] = pt.getWindingInfo(state)
                        first = False
                    ms["nearest"], iqr["nearest"] = timed(lambda: L.pt_query_nearest(state.context, d_points, n, d_near))
                    ms["parity3"], iqr["parity3"] = timed(lambda: L.pt_query_multi(state.context, d_rays, 3 * n, 0, None, d_counts))
                    w = {}
                    for key, beta in betas.items():
                        ms[key], iqr[key] = timed(lambda: L.pt_query_winding(state.context, d_points, n, beta, d_out))
                        assert L.pt_debug_winding_visits(state.context, d_points, n, beta, d_out2, d_visits) == 0, L.pt_last_error(state.context)
                        w[key] = read(d_out, n, np.float32)
                        assert np.array_equal(w[key].view(np.uint32), read(d_out2, n, np.uint32)), "the counting twin's values differ"
                        v = read(d_visits, (n, 2), np.uint32)
                        visits[key] = {"dipoles_mean": round(float(v[:, 0].mean()), 2), "triangles_mean": round(float(v[:, 1].mean()), 2),
                                       "dipoles_max": int(v[:, 0].max()), "triangles_max": int(v[:, 1].max())}
                    for key in ("beta2", "beta3"):
                        answers[key] = {"max_abs_difference_from_exact": round(float(np.abs(w[key].astype(np.float64) - w["exact"]).max()), 6),
                                        "inside_disagrees_share": round(float(((w[key] > 0.5) != (w["exact"] > 0.5)).mean()), 6)}
                    answers["inside_share"] = round(float((w["exact"] > 0.5).mean()), 4)
                    result[order] = {
                        "ms": {k: round(v, 4) for k, v in ms.items()}, "interquartile_ms": {k: round(v, 4) for k, v in iqr.items()},
                        "mqueries_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                        "visits": visits, "answers": answers,
                        "over_nearest": {k: round(ms[k] / ms["nearest"], 3) for k in betas},
                        "over_parity3": {k: round(ms[k] / ms["parity3"], 3) for k in betas},
                    }
                out["sizes"].append({"queries": n, "grid": list(shape), "triangles": int(info.n_tris), "stack_entries": int(info.stack_entries),
                                     "orders": result,
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
