#!/usr/bin/env python3
"""Times the complete lists in CSR form (pt_list_offsets, pt_query_overlap_lists, pt_query_triangles_lists) on the Cornell box and
prints ONE JSON line (also written to --out, default profiles/lists_timing.json).

Per size n, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of --repeats):
    cells            bakeOccupancy's grid cells over the scene box, n of them, x fastest (pt_query_overlap_lists)
    self             the scene's own triangles, tiled to n queries (pt_query_triangles_lists): what a collision pass sees at contact
and per set
    count            the capped call with max_prims = 0: the counts
    scan             pt_list_offsets
    fill, sort       the two launches of the list call, each on its own (the test hook pt_debug_list_phases; the sort alone runs on
                     lists that are sorted already: the network is the same, the exchanges are fewer)
    fill_sort        the list call as the product runs it
    total            count + scan + fill_sort: the caller's sequence without the allocation
    capped           the capped call with max_prims = 8 and counts on the same queries, in the same run: the parent's code, unchanged
    no_registers_*   the list call with the fill that keeps no sorted register list (every slice of two words or more goes through
                     the sort): what the register list of the slices of at most 8 words buys

    python tools/lists_timing.py [--sizes 262144,2000000] [--repeats 20] [--out profiles/lists_timing.json]
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
    ap.add_argument("--sizes", default="262144,2000000")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "lists_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    state, obj = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    ctx = state.context
    bufs = []

    def dev(nbytes):
        q = C.c_void_p()
        assert L.pt_device_malloc(ctx, C.byref(q), max(nbytes, 4)) == 0, L.pt_last_error(ctx)
        bufs.append(q.value)
        return q.value

    def timed(fn):
        assert fn() == 0, L.pt_last_error(ctx)      # warm-up: code object load, first-use allocations
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            rc = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0, L.pt_last_error(ctx)
        return float(np.median(ts))

    try:
        info = pt.getBvhInfo(state)
        lo, hi = [float(x) for x in info.scene_lo], [float(x) for x in info.scene_hi]
        mesh = pt.triangleRecords(np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4), np.asarray(obj.getIndexBuffer(), np.uint32).reshape(-1, 3))
        for size in a.sizes.split(","):
            n = int(size)
            shape = grid_shape(n)
            cells = pt.occupancyBoxes(shape, lo, hi)[:n]
            assert cells.shape[0] == n, (cells.shape, n, shape)
            sets = {"cells": (cells, L.pt_query_overlap, L.pt_query_overlap_lists),
                    "self": (np.ascontiguousarray(np.tile(mesh, ((n + mesh.shape[0] - 1) // mesh.shape[0], 1))[:n]), L.pt_query_triangles, L.pt_query_triangles_lists)}
            entry = {"queries": n, "grid": list(shape), "triangles": int(info.n_tris), "sets": {}}
            for name, (recs, count_fn, lists_fn) in sets.items():
                del bufs[:]
                try:
                    d_recs, d_counts, d_offsets, d_found, d_capped = dev(recs.nbytes), dev(n * 4), dev((n + 1) * 4), dev(n * 4), dev(n * 32)
                    assert L.pt_copy_to_device(ctx, d_recs, recs.ctypes.data, recs.nbytes) == 0
                    ms = {}
                    ms["capped"] = timed(lambda: count_fn(ctx, d_recs, n, 8, d_capped, d_counts))
                    ms["count"] = timed(lambda: count_fn(ctx, d_recs, n, 0, None, d_counts))
                    total = C.c_uint64(0)
                    ms["scan"] = timed(lambda: L.pt_list_offsets(ctx, d_counts, n, d_offsets, C.byref(total)))
                    words = int(total.value)
                    d_prims = dev(words * 4)
                    counts = np.zeros(n, np.uint32)
                    assert L.pt_copy_to_host(ctx, counts.ctypes.data, d_counts, counts.nbytes) == 0
                    call = lambda: lists_fn(ctx, d_recs, n, d_offsets, d_prims, words, d_found)          # noqa: E731
                    ms["fill_sort"] = timed(call)
                    want = np.zeros(words, np.uint32)
                    assert L.pt_copy_to_host(ctx, want.ctypes.data, d_prims, want.nbytes) == 0
                    for phases, key in ((1, "fill"), (2, "sort"), (7, "no_registers_fill_sort"), (5, "no_registers_fill"), (6, "no_registers_sort")):
                        assert L.pt_debug_list_phases(ctx, phases) == 0
                        ms[key] = timed(call)
                        if phases in (2, 7, 6):          # the sort ran last: the lists are the product's
                            got = np.zeros(words, np.uint32)
                            assert L.pt_copy_to_host(ctx, got.ctypes.data, d_prims, got.nbytes) == 0
                            assert np.array_equal(got, want), "phases %d: the lists differ" % phases
                    assert L.pt_debug_list_phases(ctx, 3) == 0
                    ms["total"] = ms["count"] + ms["scan"] + ms["fill_sort"]
                    entry["sets"][name] = {
                        "list_words": words, "mean_length": round(words / n, 3), "longest": int(counts.max()), "over_8_share": round(float((counts > 8).mean()), 4),
                        "ms": {k: round(v, 4) for k, v in ms.items()},
                        "total_over_capped": round(ms["total"] / ms["capped"], 3), "fill_sort_over_capped": round(ms["fill_sort"] / ms["capped"], 3),
                        "no_registers_over_registers": round(ms["no_registers_fill_sort"] / ms["fill_sort"], 3)}
                finally:
                    for b in bufs:
                        L.pt_device_free(ctx, b)
                    del bufs[:]
            out["sizes"].append(entry)
    finally:
        L.pt_debug_list_phases(ctx, 3)
        pt.CleanAllTheThings(state)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
