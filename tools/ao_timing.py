#!/usr/bin/env python3
"""Times the fused ambient-occlusion stage (pt_ao_image) on the Cornell box against its yardstick and prints ONE JSON line (also
written to --out, default profiles/ao_timing.json).

Per size, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of 2 x --repeats calls, the two paths
alternated in two passes):
    ao_image      pt_ao_image on pt_render_features' buffer, K rays per pixel: rays generated, traced and counted in the kernel
    query_any     the yardstick: pt_query_any on the very rays tests/ao_ref.py materialises for the same call, point-major, already in
                  device memory — the query alone, without the ray generation before it and the reduction after it
and the ratio DESIGN.md section 23 quotes (allowance: 1.25 at 1920 x 1080).  The counts of the two paths are compared as well.

    python tools/ao_timing.py [--sizes 512x512,1920x1080] [--samples 16] [--repeats 30] [--out profiles/ao_timing.json]
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
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ao_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import ao_ref as ar
    L = _native.hip()
    K = a.samples
    disk = pt.aoSamples(K)
    out = {"tool": "ao_timing", "repeats": a.repeats, "samples": K, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=4, spp=1)
        bufs = []
        try:
            n = w * h
            p = state.params
            radius, bias = pt.pathtracer._ao_reach(state, None, None, "ao_timing")
            params = {"radius": float(np.float32(radius)), "bias": float(np.float32(bias)), "seed": 0}
            for nbytes in (n * 16, n * 16, n * 4, n * 4, n * K * 32, n * K):      # albedo, normal_depth, visible, ao, rays, occluded
                q = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0
                bufs.append(q.value)
            d_alb, d_nd, d_vis, d_ao, d_rays, d_occ = bufs
            assert L.pt_render_features(state.context, C.byref(p), d_alb, d_nd) == 0
            nd = np.zeros((h, w, 4), np.float32)
            assert L.pt_copy_to_host(state.context, nd.ctypes.data, d_nd, nd.nbytes) == 0
            P, N = ar.image_points(nd, (p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple()), w, h)
            traceable = np.zeros(n * K, bool)
            step = 1 << 17                                   # the rays of 128 Ki points at a time: 64 MiB
            for first in range(0, n, step):
                r = ar.rays(P[first:first + step], N[first:first + step], disk, params, first=first)
                traceable[first * K:first * K + r.shape[0]] = np.isfinite(r[:, 0:6]).all(axis=1)
                assert L.pt_copy_to_device(state.context, d_rays + first * K * 32, r.ctypes.data, r.nbytes) == 0
            ap_ = _native.AoParams(K, params["radius"], params["bias"], 0, 0, K, (C.c_uint32 * 2)(0, 0))

            def timed(fn):
                assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return ts

            # alternated, so that a drift of the machine's state falls on both
            runs = {"ao_image": lambda: L.pt_ao_image(state.context, C.byref(p), d_nd, disk.ctypes.data, C.byref(ap_), d_vis, d_ao),
                    "query_any": lambda: L.pt_query_any(state.context, d_rays, n * K, d_occ)}
            first_pass = {k: timed(fn) for k, fn in runs.items()}
            second_pass = {k: timed(fn) for k, fn in reversed(list(runs.items()))}
            ms = {k: float(np.median(first_pass[k] + second_pass[k])) for k in runs}      # the median of 2 x --repeats calls
            vis = np.zeros(n, np.uint32); occ = np.zeros(n * K, np.uint8)
            assert L.pt_copy_to_host(state.context, vis.ctypes.data, d_vis, vis.nbytes) == 0
            assert L.pt_copy_to_host(state.context, occ.ctypes.data, d_occ, occ.nbytes) == 0
            same = bool(np.array_equal(vis, (K - (occ.astype(bool) & traceable).reshape(n, K).sum(axis=1)).astype(np.uint32)))
            surface = ar.surface(P, N)
            out["sizes"].append({
                "width": w, "height": h, "points": n, "rays": n * K, "radius": params["radius"], "bias": params["bias"],
                "stack_entries": int(pt.getBvhInfo(state).stack_entries), "surface_share": round(float(surface.mean()), 4),
                "occluded_share": round(float(occ[np.repeat(surface, K)].mean()), 4), "counts_equal": same,
                "ms": {k: round(v, 4) for k, v in ms.items()},
                "ms_pass_medians": {k: [round(float(np.median(first_pass[k])), 4), round(float(np.median(second_pass[k])), 4)] for k in runs},
                "ms_min_max": {k: [round(min(first_pass[k] + second_pass[k]), 4), round(max(first_pass[k] + second_pass[k]), 4)] for k in runs},
                "mrays_per_s": {k: round(n * K / v / 1e3, 1) for k, v in ms.items()},
                "ao_over_query_any": round(ms["ao_image"] / ms["query_any"], 3),
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
