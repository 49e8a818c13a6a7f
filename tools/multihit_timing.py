#!/usr/bin/env python3
"""Times pt_query_multi on the Cornell box's camera rays against pt_query_closest and prints ONE JSON line (also written to --out,
default profiles/multihit_timing.json).

Per size, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of --repeats):
    query_closest                    the yardstick: the first hit alone
    multi_1 / _2 / _4 / _8           max_hits 1, 2, 4, 8 without counts: the walk cut behind the last kept hit
    multi_4_counts                   max_hits 4 with counts: nothing pruned at a hit
    count_only                       max_hits 0: the same walk without a list
    peel_4                           what the call replaces: four pt_query_closest calls, call j on rays whose tmin is the t of layer
                                     j - 1 (a miss keeps its ray).  The four ray arrays are made ahead of the clock, so this is the
                                     launches and walks alone, without the caller's pass that moves tmin
    ..._permuted                     query_closest, multi_4 and multi_4_counts on the same rays in a fixed random permutation
and the ratios DESIGN.md section 25 quotes.

    python tools/multihit_timing.py [--sizes 512x512,1920x1080] [--repeats 30] [--out profiles/multihit_timing.json]
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
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multihit_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import denoise_ref as dr
    L = _native.hip()
    out = {"tool": "multihit_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=4, spp=1)
        bufs = []

        def alloc(nbytes):
            q = C.c_void_p()
            assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0, L.pt_last_error(state.context)
            bufs.append(q.value)
            return q.value

        def upload(x):
            d = alloc(x.nbytes)
            assert L.pt_copy_to_device(state.context, d, x.ctypes.data, x.nbytes) == 0
            return d

        try:
            n = w * h
            p = state.params
            rays = dr.pixel_rays(w, h, p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple())
            d_rays = upload(rays)
            d_perm = upload(np.ascontiguousarray(rays[np.random.default_rng(1).permutation(n)]))
            d_hits, d_counts = alloc(n * 8 * 32), alloc(n * 4)
            # the layers of the peel, and what the rays go through
            layers, layer = [d_rays], rays
            for _ in range(3):
                got = pt.queryRays(state, layer)
                layer = layer.copy()
                hit = got["prim"] != 0xFFFFFFFF
                layer[hit, 6] = got["t"][hit]
                layers.append(upload(layer))
            count = pt.queryRaysMulti(state, rays, max_hits=0, counts=True)["count"]

            def timed(fn):
                assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            def multi(d, k, counts):
                return lambda: L.pt_query_multi(state.context, d, n, k, d_hits if k else None, d_counts if counts else None)

            def peel():
                rc = 0
                for d in layers:
                    rc |= L.pt_query_closest(state.context, d, n, d_hits)
                return rc

            ms = {"query_closest": timed(lambda: L.pt_query_closest(state.context, d_rays, n, d_hits))}
            for k in (1, 2, 4, 8):
                ms["multi_%d" % k] = timed(multi(d_rays, k, False))
            ms["multi_4_counts"] = timed(multi(d_rays, 4, True))
            ms["count_only"] = timed(multi(d_rays, 0, True))
            ms["peel_4"] = timed(peel)
            ms["query_closest_permuted"] = timed(lambda: L.pt_query_closest(state.context, d_perm, n, d_hits))
            ms["multi_4_permuted"] = timed(multi(d_perm, 4, False))
            ms["multi_4_counts_permuted"] = timed(multi(d_perm, 4, True))
            out["sizes"].append({
                "width": w, "height": h, "rays": n, "stack_entries": int(pt.getBvhInfo(state).stack_entries),
                "hits_per_ray": {"mean": round(float(count.mean()), 3), "max": int(count.max()), "none": round(float((count == 0).mean()), 4),
                                 "two_or_more": round(float((count >= 2).mean()), 4), "more_than_four": round(float((count > 4).mean()), 4)},
                "ms": {k: round(v, 4) for k, v in ms.items()},
                "mrays_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                "over_query_closest": {k: round(v / ms["query_closest"], 3) for k, v in ms.items() if not k.endswith("_permuted") and k != "query_closest"},
                "multi_4_over_peel_4": round(ms["multi_4"] / ms["peel_4"], 3),
                "permuted_over_coherent": {k: round(ms[k + "_permuted"] / ms[k], 3) for k in ("query_closest", "multi_4", "multi_4_counts")},
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
