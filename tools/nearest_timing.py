#!/usr/bin/env python3
"""Times the closest-point query (pt_query_nearest) on the Cornell box and prints ONE JSON line (also written to --out, default
profiles/nearest_timing.json).

Per size n, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of --repeats), all
with max_radius = +inf:
    nearest_surface         first-hit points of the camera rays of a view with n pixels, o + t d (distance ~ 0); a ray that hits
                            nothing is replaced by another ray's point
    nearest_grid            the cell centres of a distance-field grid of n cells over the scene box, x fastest
    nearest_grid_permuted   the same cells in a fixed random permutation: what incoherence costs
    query_closest           the scale: pt_query_closest on the n camera rays
and, from the counting twin of the kernel (pt_debug_nearest_visits, one call per set, not timed), the mean inner nodes visited and
triangles tested per query.

    python tools/nearest_timing.py [--sizes 512x512,1920x1080] [--repeats 30] [--out profiles/nearest_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def grid_shape(n):
    """(nz, ny, nx) with nz * ny * nx == n, as close to a cube as the divisors of n allow"""
    best = None
    for nz in range(1, int(round(n ** (1.0 / 3.0))) + 2):
        if n % nz:
            continue
        m = n // nz
        for ny in range(nz, int(m ** 0.5) + 1):
            if m % ny == 0 and (best is None or m // ny - nz < best[2] - best[0]):
                best = (nz, ny, m // ny)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import denoise_ref as dr
    L = _native.hip()
    out = {"tool": "nearest_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=4, spp=1)
        bufs = []
        try:
            n = w * h
            p = state.params
            info = pt.getBvhInfo(state)
            rays = dr.pixel_rays(w, h, p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple())
            for _ in range(4):          # rays, points, records, visit counts
                q = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(q), n * 32) == 0
                bufs.append(q.value)
            d_rays, d_points, d_out, d_visits = bufs
            assert L.pt_copy_to_device(state.context, d_rays, rays.ctypes.data, rays.nbytes) == 0

            def timed(fn):
                assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            ms, visits, found = {}, {}, {}
            ms["query_closest"] = timed(lambda: L.pt_query_closest(state.context, d_rays, n, d_out))
            hits = np.zeros((n, 8), np.float32)
            assert L.pt_copy_to_host(state.context, hits.ctypes.data, d_out, hits.nbytes) == 0
            hit = hits.view(np.uint32)[:, 1] != 0xFFFFFFFF
            surface = (rays[:, 0:3] + hits[:, 0:1] * rays[:, 3:6]).astype(np.float32)
            surface[~hit] = surface[hit][np.arange(int((~hit).sum())) % int(hit.sum())]
            shape = grid_shape(n)
            grid = pt.distanceFieldPoints(shape, [float(x) for x in info.scene_lo], [float(x) for x in info.scene_hi])
            sets = {"nearest_surface": surface, "nearest_grid": grid, "nearest_grid_permuted": grid[np.random.default_rng(1).permutation(n)]}
            for name, pts in sets.items():
                points = np.empty((n, 4), np.float32)
                points[:, 0:3] = pts
                points[:, 3] = np.inf
                assert L.pt_copy_to_device(state.context, d_points, points.ctypes.data, points.nbytes) == 0
                ms[name] = timed(lambda: L.pt_query_nearest(state.context, d_points, n, d_out))
                assert L.pt_debug_nearest_visits(state.context, d_points, n, d_out, d_visits) == 0, L.pt_last_error(state.context)
                counts = np.zeros((n, 2), np.uint32); rec = np.zeros((n, 8), np.float32)
                assert L.pt_copy_to_host(state.context, counts.ctypes.data, d_visits, counts.nbytes) == 0
                assert L.pt_copy_to_host(state.context, rec.ctypes.data, d_out, rec.nbytes) == 0
                visits[name] = {"nodes_mean": round(float(counts[:, 0].mean()), 2), "triangles_mean": round(float(counts[:, 1].mean()), 2),
                                "nodes_max": int(counts[:, 0].max()), "triangles_max": int(counts[:, 1].max())}
                found[name] = {"found_share": round(float((rec.view(np.uint32)[:, 1] != 0xFFFFFFFF).mean()), 4), "distance_median": round(float(np.median(rec[:, 0])), 6)}
            out["sizes"].append({
                "width": w, "height": h, "queries": n, "grid": list(shape), "triangles": int(info.n_tris), "stack_entries": int(info.stack_entries),
                "camera_hit_share": round(float(hit.mean()), 4),
                "ms": {k: round(v, 4) for k, v in ms.items()},
                "mqueries_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                "visits": visits, "answers": found,
                "surface_over_query_closest": round(ms["nearest_surface"] / ms["query_closest"], 3),
                "grid_over_query_closest": round(ms["nearest_grid"] / ms["query_closest"], 3),
                "permuted_over_coherent_grid": round(ms["nearest_grid_permuted"] / ms["nearest_grid"], 3),
            })
        finally:
            for b in bufs:
                L.pt_device_free(state.context, b)
            pt.CleanAllTheThings(state)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
