#!/usr/bin/env python3
"""Times the swept oriented-box casts (pt_query_box_cast, pt_query_box_cast_any) on the Cornell box and prints ONE JSON line (also
written to --out, default profiles/boxcast_timing.json).

One process, one warm-up call per configuration, then the median of --repeats synchronised calls with [min, max] beside it.  Per
kind of box — tests/boxcast_ref.py's "cells" (cubes in any rotation) and "links" (long and thin: one half extent 5 to 20 % of the
scene's diagonal, the other two 0.2 to 2 %), --casts of each:
    record, byte                    pt_query_box_cast and pt_query_box_cast_any
    mode0, mode1                    the counting twin (pt_debug_box_cast_visits) with the six extra axes and on the slab alone: the
                                    two arms of that decision, with the mean and maximum inner nodes and triangles per cast
    twelve_triangles                the route it replaces: pt_query_triangle_cast on the 12 n triangles of the boxes' surfaces (twelve
                                    calls of n) and the reduction to the earliest on the host (timed apart), with the share of casts
                                    for which that route reports no impact or a later one
    capsule                         pt_query_capsule_cast on the inscribed capsule (the longest box axis, the smallest half extent as
                                    its radius): the cost scale
    overlap_oriented_any            pt_query_overlap_oriented_any on the first sixteen floats: the cast at d = 0

    python tools/boxcast_timing.py [--casts 2097152] [--repeats 30] [--out profiles/boxcast_timing.json]
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
    ap.add_argument("--casts", type=int, default=2097152)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxcast_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import boxcast_ref as br
    import kernel_meta
    L = _native.hip()
    n = a.casts
    vgprs = {k["name"].split("(")[0].replace("void ptd::", ""): k["vgpr_count"] for k in kernel_meta.kernel_table(_native.hip_library_path()) if "k_query_obox_toi" in k["name"]}
    out = {"tool": "boxcast_timing", "repeats": a.repeats, "casts": n, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "vgpr_count": vgprs, "kinds": {}}
    state, obj = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    bufs = []
    try:
        info = pt.getBvhInfo(state)
        out["triangles"], out["stack_entries"] = int(info.n_tris), int(info.stack_entries)
        for nbytes in (n * 80, n * 48, n * 8, n * 64):          # casts, records / bytes, visit counts, the other queries' records
            q = C.c_void_p()
            assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0
            bufs.append(q.value)
        d_in, d_out, d_visits, d_other = bufs

        def timed(fn):
            assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                rc = fn()
                ts.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0, L.pt_last_error(state.context)
            return [round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), round(float(np.max(ts)), 4)]

        def read(shape, dtype=np.float32):
            rec = np.zeros(shape, dtype)
            assert L.pt_copy_to_host(state.context, rec.ctypes.data, d_out, rec.nbytes) == 0
            return rec

        for kind in ("cells", "links"):
            casts = br.cast_set(kind, obj.getVerticesFloat(), obj.getIndexBuffer(), n=n)
            assert L.pt_copy_to_device(state.context, d_in, casts.ctypes.data, casts.nbytes) == 0
            ms, visits = {}, {}
            ms["record"] = timed(lambda: L.pt_query_box_cast(state.context, d_in, n, d_out))
            t_box = read((n, 12))[:, 0].copy()
            ms["byte"] = timed(lambda: L.pt_query_box_cast_any(state.context, d_in, n, d_out))
            for mode in (0, 1):
                ms["mode%d" % mode] = timed(lambda: L.pt_debug_box_cast_visits(state.context, d_in, n, d_out, d_visits, mode))
                vis = np.zeros((n, 2), np.uint32)
                assert L.pt_copy_to_host(state.context, vis.ctypes.data, d_visits, vis.nbytes) == 0
                assert np.array_equal(read((n, 12))[:, 0].view(np.uint32), t_box.view(np.uint32))
                visits["mode%d" % mode] = {"nodes_mean": round(float(vis[:, 0].mean()), 2), "triangles_mean": round(float(vis[:, 1].mean()), 2),
                                           "nodes_max": int(vis[:, 0].max()), "triangles_max": int(vis[:, 1].max())}
            # the route it replaces: the 12 surface triangles, one call per triangle of the cube, the earliest on the host
            A, c, h, d, tmax = br.parts(casts)
            sign = np.array([[(-1.0, 1.0)[(k >> b) & 1] for b in range(3)] for k in range(8)], np.float32)
            corners = (c[:, None, :] + np.einsum("nkj,ncj->nck", A, sign[None] * h[:, None, :])).astype(np.float32)
            earliest = np.full(n, np.inf, np.float32)
            twelve, reduce_ms = [0.0, 0.0, 0.0], 0.0
            recs = np.zeros((n, 16), np.float32)
            recs[:, 12:15], recs[:, 3] = casts[:, 16:19], casts[:, 19]
            for tri in br._CUBE_TRIS:
                recs[:, 0:3], recs[:, 4:7], recs[:, 8:11] = corners[:, tri[0]], corners[:, tri[1]], corners[:, tri[2]]
                assert L.pt_copy_to_device(state.context, d_other, recs.ctypes.data, recs.nbytes) == 0
                one = timed(lambda: L.pt_query_triangle_cast(state.context, d_other, n, d_out))
                twelve = [round(x + y, 4) for x, y in zip(twelve, one)]
                t = read((n, 8))[:, 0]
                t0 = time.perf_counter()
                earliest = np.where((t >= 0) & (t < earliest), t, earliest)
                reduce_ms += (time.perf_counter() - t0) * 1e3
            ms["twelve_triangles"] = twelve
            hit = t_box >= 0
            with np.errstate(invalid="ignore"):
                wrong = hit & (earliest > t_box * np.float32(1.0 + 2.0 ** -12) + np.float32(2.0 ** -12))          # +inf where no surface triangle touches anything
            # the inscribed capsule
            rows = np.arange(n)
            long_axis = np.argmax(h, axis=1)
            radius = np.min(h, axis=1)
            half = (h[rows, long_axis] - radius)[:, None] * A[rows, :, long_axis]
            cap = np.zeros((n, 12), np.float32)
            cap[:, 0:3], cap[:, 3], cap[:, 4:7], cap[:, 7], cap[:, 8:11] = c - half, radius, c + half, tmax, d
            assert L.pt_copy_to_device(state.context, d_other, cap.ctypes.data, cap.nbytes) == 0
            ms["capsule"] = timed(lambda: L.pt_query_capsule_cast(state.context, d_other, n, d_out))
            boxes = np.ascontiguousarray(casts[:, :16])
            assert L.pt_copy_to_device(state.context, d_other, boxes.ctypes.data, boxes.nbytes) == 0
            ms["overlap_oriented_any"] = timed(lambda: L.pt_query_overlap_oriented_any(state.context, d_other, n, d_out))
            static = read((n,), np.uint8)
            assert np.array_equal(static != 0, t_box == 0)             # t == 0 iff the static query's byte
            out["kinds"][kind] = {
                "ms": ms, "mcasts_per_s": {k: round(n / v[0] / 1e3, 1) for k, v in ms.items()}, "visits": visits, "twelve_triangles_reduce_ms": round(reduce_ms, 2),
                "hit_share": round(float(hit.mean()), 4), "start_overlap_share": round(float((t_box == 0).mean()), 4),
                "twelve_triangles_wrong_share": round(float(wrong.mean()), 4), "twelve_triangles_none_share": round(float((hit & ~np.isfinite(earliest)).mean()), 4),
                "mode0_over_mode1": round(ms["mode0"][0] / ms["mode1"][0], 3), "record_over_capsule": round(ms["record"][0] / ms["capsule"][0], 3),
                "record_over_twelve_triangles": round(ms["record"][0] / ms["twelve_triangles"][0], 3),
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
