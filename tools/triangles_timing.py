#!/usr/bin/env python3
"""Times the triangle-against-mesh queries (pt_query_triangles_any, pt_query_triangles) on the Cornell box and prints ONE JSON line
(also written to --out, default profiles/triangles_timing.json).

Per size n, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of --repeats) of
pt_query_triangles_any, pt_query_triangles with max_prims = 0 (counts alone) and pt_query_triangles with max_prims = 8 and counts,
each on:
    surface            n small triangles (vertices within --size of the scene box's diagonal) around the first-hit points of the
                       camera rays of a view with n pixels, in pixel order; a ray that hits nothing is replaced by another ray's point
    surface_permuted   the same triangles in a fixed random permutation: what incoherence costs
and, as the scale beside each figure, the box query (pt_query_overlap_any / pt_query_overlap with the same max_prims) on the same
triangles' bounding boxes — what a caller had before, the broad phase alone —, and from the counting twins (pt_debug_triangles_visits,
pt_debug_overlap_visits, one call per set, not timed) the mean and maximum inner nodes visited and triangles tested per query.

    python tools/triangles_timing.py [--sizes 512x512,1920x1080] [--size 0.01] [--repeats 30] [--out profiles/triangles_timing.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--size", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangles_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import denoise_ref as dr
    L = _native.hip()
    out = {"tool": "triangles_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=4, spp=1)
        bufs = []
        try:
            n = w * h
            p = state.params
            info = pt.getBvhInfo(state)
            rays = dr.pixel_rays(w, h, p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple())
            for nbytes in (n * 48, n * 32, n * 32, n * 4, n * 8):          # triangles / rays, boxes, prims / records, counts, visit counts
                q = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0
                bufs.append(q.value)
            d_tris, d_boxes, d_out, d_counts, d_visits = bufs
            assert L.pt_copy_to_device(state.context, d_tris, rays.ctypes.data, rays.nbytes) == 0

            def timed(fn):
                assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            assert L.pt_query_closest(state.context, d_tris, n, d_out) == 0
            hits = np.zeros((n, 8), np.float32)
            assert L.pt_copy_to_host(state.context, hits.ctypes.data, d_out, hits.nbytes) == 0
            hit = hits.view(np.uint32)[:, 1] != 0xFFFFFFFF
            surface = (rays[:, 0:3] + hits[:, 0:1] * rays[:, 3:6]).astype(np.float32)
            surface[~hit] = surface[hit][np.arange(int((~hit).sum())) % int(hit.sum())]
            lo, hi = np.array([float(x) for x in info.scene_lo]), np.array([float(x) for x in info.scene_hi])
            size = np.float32(a.size * np.sqrt(((hi - lo) ** 2).sum()))
            rng = np.random.default_rng(7)
            recs = np.zeros((n, 3, 4), np.float32)
            recs[:, :, :3] = surface[:, None, :] + size * rng.uniform(-1.0, 1.0, (n, 3, 3)).astype(np.float32)
            recs = recs.reshape(n, 12)
            sets = {"surface": recs, "surface_permuted": recs[np.random.default_rng(1).permutation(n)]}
            ms, visits, answers = {}, {}, {}
            for name, r in sets.items():
                r = np.ascontiguousarray(r, np.float32)
                v = r.reshape(n, 3, 4)[:, :, :3]
                boxes = np.zeros((n, 8), np.float32)
                qlo, qhi = v.min(axis=1).astype(np.float64), v.max(axis=1).astype(np.float64)
                boxes[:, 0:3] = 0.5 * (qlo + qhi)
                half = 0.5 * (qhi - qlo) + np.abs(boxes[:, 0:3].astype(np.float64) - 0.5 * (qlo + qhi))
                boxes[:, 3:6] = np.nextafter(half.astype(np.float32), np.float32(np.inf))       # the box contains the triangle
                assert L.pt_copy_to_device(state.context, d_tris, r.ctypes.data, r.nbytes) == 0
                assert L.pt_copy_to_device(state.context, d_boxes, boxes.ctypes.data, boxes.nbytes) == 0
                ms["any_" + name] = timed(lambda: L.pt_query_triangles_any(state.context, d_tris, n, d_out))
                ms["count_" + name] = timed(lambda: L.pt_query_triangles(state.context, d_tris, n, 0, None, d_counts))
                ms["list8_" + name] = timed(lambda: L.pt_query_triangles(state.context, d_tris, n, 8, d_out, d_counts))
                ms["box_any_" + name] = timed(lambda: L.pt_query_overlap_any(state.context, d_boxes, n, d_out))
                ms["box_count_" + name] = timed(lambda: L.pt_query_overlap(state.context, d_boxes, n, 0, None, d_counts))
                ms["box_list8_" + name] = timed(lambda: L.pt_query_overlap(state.context, d_boxes, n, 8, d_out, d_counts))
                vis = np.zeros((n, 2), np.uint32); counts = np.zeros(n, np.uint32)
                for key, fn, d_in in (("box", L.pt_debug_overlap_visits, d_boxes), ("triangle", L.pt_debug_triangles_visits, d_tris)):
                    assert fn(state.context, d_in, n, d_counts, d_visits) == 0, L.pt_last_error(state.context)
                    assert L.pt_copy_to_host(state.context, vis.ctypes.data, d_visits, vis.nbytes) == 0
                    assert L.pt_copy_to_host(state.context, counts.ctypes.data, d_counts, counts.nbytes) == 0
                    visits[key + "_" + name] = {"nodes_mean": round(float(vis[:, 0].mean()), 2), "triangles_mean": round(float(vis[:, 1].mean()), 2),
                                                "nodes_max": int(vis[:, 0].max()), "triangles_max": int(vis[:, 1].max())}
                    answers[key + "_" + name] = {"hit_share": round(float((counts != 0).mean()), 4), "count_mean": round(float(counts.mean()), 3), "count_max": int(counts.max())}
            out["sizes"].append({
                "width": w, "height": h, "queries": n, "triangle_size": float(size), "triangles": int(info.n_tris), "stack_entries": int(info.stack_entries),
                "camera_hit_share": round(float(hit.mean()), 4),
                "ms": {k: round(v, 4) for k, v in ms.items()},
                "mqueries_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                "visits": visits, "answers": answers,
                "over_box": {k: round(ms[k + "_surface"] / ms["box_" + k + "_surface"], 3) for k in ("any", "count", "list8")},
                "permuted_over_coherent_any": round(ms["any_surface_permuted"] / ms["any_surface"], 3),
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
