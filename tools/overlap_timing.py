#!/usr/bin/env python3
"""Times the box-overlap queries (pt_query_overlap_any, pt_query_overlap) on the Cornell box and prints ONE JSON line (also written to
--out, default profiles/overlap_timing.json).

Per size n, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of --repeats) of
pt_query_overlap_any, pt_query_overlap with max_prims = 0 (counts alone) and pt_query_overlap with max_prims = 8 and counts, each on:
    grid            the cells of an occupancy grid of n cells over the scene box, x fastest (pathtracer.occupancyBoxes)
    grid_permuted   the same cells in a fixed random permutation: what incoherence costs
    surface         boxes of the cells' half extent centred on the first-hit points of the camera rays of a view with n pixels; a ray
                    that hits nothing is replaced by another ray's point
and, as the scale beside them, the closest-point query on the same centres with max_radius equal to the cells' half diagonal
(pt_query_nearest: what a caller had to use for "is this cell empty" before), and from the counting twin (pt_debug_overlap_visits, one
call per set, not timed) the mean and maximum inner nodes visited and triangles tested per box.

    python tools/overlap_timing.py [--sizes 512x512,1920x1080] [--repeats 30] [--out profiles/overlap_timing.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import denoise_ref as dr
    from nearest_timing import grid_shape
    L = _native.hip()
    out = {"tool": "overlap_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=4, spp=1)
        bufs = []
        try:
            n = w * h
            p = state.params
            info = pt.getBvhInfo(state)
            rays = dr.pixel_rays(w, h, p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple())
            for _ in range(5):          # rays / points, boxes, prims / records, counts, visit counts
                q = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(q), n * 32) == 0
                bufs.append(q.value)
            d_in, d_boxes, d_out, d_counts, d_visits = bufs
            assert L.pt_copy_to_device(state.context, d_in, rays.ctypes.data, rays.nbytes) == 0

            def timed(fn):
                assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            assert L.pt_query_closest(state.context, d_in, n, d_out) == 0
            hits = np.zeros((n, 8), np.float32)
            assert L.pt_copy_to_host(state.context, hits.ctypes.data, d_out, hits.nbytes) == 0
            hit = hits.view(np.uint32)[:, 1] != 0xFFFFFFFF
            surface = (rays[:, 0:3] + hits[:, 0:1] * rays[:, 3:6]).astype(np.float32)
            surface[~hit] = surface[hit][np.arange(int((~hit).sum())) % int(hit.sum())]
            shape = grid_shape(n)
            grid = pt.occupancyBoxes(shape, [float(x) for x in info.scene_lo], [float(x) for x in info.scene_hi])
            half = grid[0, 3:6].copy()
            on_surface = grid.copy()
            on_surface[:, 0:3] = surface
            sets = {"grid": grid, "grid_permuted": grid[np.random.default_rng(1).permutation(n)], "surface": on_surface}
            radius = float(np.sqrt((half.astype(np.float64) ** 2).sum()))
            ms, visits, answers = {}, {}, {}
            for name, boxes in sets.items():
                boxes = np.ascontiguousarray(boxes, np.float32)
                assert L.pt_copy_to_device(state.context, d_boxes, boxes.ctypes.data, boxes.nbytes) == 0
                ms["any_" + name] = timed(lambda: L.pt_query_overlap_any(state.context, d_boxes, n, d_out))
                ms["count_" + name] = timed(lambda: L.pt_query_overlap(state.context, d_boxes, n, 0, None, d_counts))
                ms["list8_" + name] = timed(lambda: L.pt_query_overlap(state.context, d_boxes, n, 8, d_out, d_counts))
                points = np.empty((n, 4), np.float32)
                points[:, 0:3] = boxes[:, 0:3]
                points[:, 3] = radius
                assert L.pt_copy_to_device(state.context, d_in, points.ctypes.data, points.nbytes) == 0
                ms["nearest_" + name] = timed(lambda: L.pt_query_nearest(state.context, d_in, n, d_out))
                assert L.pt_debug_overlap_visits(state.context, d_boxes, n, d_counts, d_visits) == 0, L.pt_last_error(state.context)
                vis = np.zeros((n, 2), np.uint32); counts = np.zeros(n, np.uint32)
                assert L.pt_copy_to_host(state.context, vis.ctypes.data, d_visits, vis.nbytes) == 0
                assert L.pt_copy_to_host(state.context, counts.ctypes.data, d_counts, counts.nbytes) == 0
                visits[name] = {"nodes_mean": round(float(vis[:, 0].mean()), 2), "triangles_mean": round(float(vis[:, 1].mean()), 2),
                                "nodes_max": int(vis[:, 0].max()), "triangles_max": int(vis[:, 1].max())}
                answers[name] = {"occupied_share": round(float((counts != 0).mean()), 4), "count_mean": round(float(counts.mean()), 3), "count_max": int(counts.max())}
            out["sizes"].append({
                "width": w, "height": h, "boxes": n, "grid": list(shape), "half_extent": [float(x) for x in half], "nearest_radius": radius,
                "triangles": int(info.n_tris), "stack_entries": int(info.stack_entries), "camera_hit_share": round(float(hit.mean()), 4),
                "ms": {k: round(v, 4) for k, v in ms.items()},
                "mboxes_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                "visits": visits, "answers": answers,
                "any_grid_over_nearest_grid": round(ms["any_grid"] / ms["nearest_grid"], 3),
                "permuted_over_coherent_any": round(ms["any_grid_permuted"] / ms["any_grid"], 3),
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
