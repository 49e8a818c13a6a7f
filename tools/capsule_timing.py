#!/usr/bin/env python3
"""Times the swept-capsule casts (pt_query_capsule_cast, pt_query_capsule_cast_any) on the Cornell box and prints ONE JSON line (also
written to --out, default profiles/capsule_timing.json).

One process, one warm-up call per configuration, then the median of --repeats synchronised calls with [min, max] beside it.  Per
kind of capsule — tests/capsule_ref.py's "upright" (a character: the axis along the scene's up direction, 2 to 4 radii long, moving
near-horizontally) and "links" (robot links: the axis 20 to 50 % of the scene's diagonal, diagonal to the walls), --casts of each:
    record, byte                    pt_query_capsule_cast and pt_query_capsule_cast_any
    mode0, mode1                    the counting twin (pt_debug_capsule_cast_visits) with the product's walk and without the plane axis:
                                    the two arms of that decision, with the mean and maximum inner nodes and triangles per cast
    sphere                          pt_query_sweep on (p0, d, r) of the same casts: what one sphere costs (the yardstick)
    five_spheres                    five pt_query_sweep calls on spheres along the axis, the route callers have had, and the share of
                                    casts whose earliest sphere reports no impact or a later one than the capsule cast

    python tools/capsule_timing.py [--casts 2097152] [--repeats 30] [--out profiles/capsule_timing.json]
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
    ap.add_argument("--casts", type=int, default=2097152)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capsule_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import capsule_ref as cr
    import kernel_meta
    L = _native.hip()
    n = a.casts
    vgprs = {k["name"].split("(")[0].replace("void ptd::", ""): k["vgpr_count"] for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_query_capsule" in k["name"]}
    out = {"tool": "capsule_timing", "repeats": a.repeats, "casts": n, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "vgpr_count": vgprs, "kinds": {}}
    state, obj = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    bufs = []
    try:
        info = pt.getBvhInfo(state)
        out["triangles"], out["stack_entries"] = int(info.n_tris), int(info.stack_entries)
        for nbytes in (n * 48, n * 32, n * 8, n * 32):          # casts, records / bytes, visit counts, sweeps
            q = C.c_void_p()
            assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0
            bufs.append(q.value)
        d_in, d_out, d_visits, d_sweeps = bufs

        def timed(fn):
            assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                rc = fn()
                ts.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0, L.pt_last_error(state.context)
            return [round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), round(float(np.max(ts)), 4)]

        def records():
            rec = np.zeros((n, 8), np.float32)
            assert L.pt_copy_to_host(state.context, rec.ctypes.data, d_out, rec.nbytes) == 0
            return rec

        for kind in ("upright", "links"):
            casts = cr.cast_set(kind, obj.getVerticesFloat(), obj.getIndexBuffer(), n=n)
            assert L.pt_copy_to_device(state.context, d_in, casts.ctypes.data, casts.nbytes) == 0
            ms, visits = {}, {}
            ms["record"] = timed(lambda: L.pt_query_capsule_cast(state.context, d_in, n, d_out))
            t_capsule = records()[:, 0].copy()
            ms["byte"] = timed(lambda: L.pt_query_capsule_cast_any(state.context, d_in, n, d_out))
            for mode in (0, 1):
                ms["mode%d" % mode] = timed(lambda: L.pt_debug_capsule_cast_visits(state.context, d_in, n, d_out, d_visits, mode))
                vis = np.zeros((n, 2), np.uint32)
                assert L.pt_copy_to_host(state.context, vis.ctypes.data, d_visits, vis.nbytes) == 0
                assert np.array_equal(records()[:, 0].view(np.uint32), t_capsule.view(np.uint32))
                visits["mode%d" % mode] = {"nodes_mean": round(float(vis[:, 0].mean()), 2), "triangles_mean": round(float(vis[:, 1].mean()), 2),
                                           "nodes_max": int(vis[:, 0].max()), "triangles_max": int(vis[:, 1].max())}
            # the sphere at p0, and five spheres along the axis
            earliest = np.full(n, np.inf, np.float32)
            five = [0.0, 0.0, 0.0]
            for j in range(5):
                o = casts[:, 0:3] + (casts[:, 4:7] - casts[:, 0:3]) * np.float32(j / 4.0)
                sweeps = np.ascontiguousarray(np.concatenate([o, casts[:, 8:11], casts[:, 3:4], casts[:, 7:8]], axis=1), np.float32)
                assert L.pt_copy_to_device(state.context, d_sweeps, sweeps.ctypes.data, sweeps.nbytes) == 0
                one = timed(lambda: L.pt_query_sweep(state.context, d_sweeps, n, d_out))
                if j == 0:
                    ms["sphere"] = one
                five = [round(x + y, 4) for x, y in zip(five, one)]
                t = records()[:, 0]
                earliest = np.where((t >= 0) & (t < earliest), t, earliest)
            ms["five_spheres"] = five
            hit = t_capsule >= 0
            wrong = hit & (earliest > t_capsule)                 # +inf where no sphere touches anything
            out["kinds"][kind] = {
                "ms": ms, "mcasts_per_s": {k: round(n / v[0] / 1e3, 1) for k, v in ms.items()}, "visits": visits,
                "hit_share": round(float(hit.mean()), 4), "start_overlap_share": round(float((t_capsule == 0).mean()), 4),
                "five_spheres_wrong_share": round(float(wrong.mean()), 4), "five_spheres_none_share": round(float((hit & ~np.isfinite(earliest)).mean()), 4),
                "mode0_over_mode1": round(ms["mode0"][0] / ms["mode1"][0], 3), "record_over_sphere": round(ms["record"][0] / ms["sphere"][0], 3),
                "record_over_five_spheres": round(ms["record"][0] / ms["five_spheres"][0], 3),
            }
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
