#!/usr/bin/env python3
"""Times the swept-sphere casts (pt_query_sweep, pt_query_sweep_any) on the Cornell box and prints ONE JSON line (also written to --out,
default profiles/sweep_timing.json).

Per size w x h, host wall time of each call (every one returns synchronised; one process, a warm-up call, the median of --repeats) on
the n = w * h camera rays of the view as sweeps with tmax = +inf:
    sweep_r0, sweep_r1, sweep_r5          pt_query_sweep with the radius at 0, at 1 % and at 5 % of the scene box's diagonal
    sweep_r1_permuted                     the 1 % sweeps in a fixed random permutation: what incoherence costs
    any_r0, any_r1, any_r5                pt_query_sweep_any on the same sweeps
    closest                               pt_query_closest on the same rays (tmin 0): the scale beside them
and from the counting twin (pt_debug_sweep_visits, one call per radius and one for the permutation, not timed) the mean and maximum
inner nodes visited and triangles tested per sweep.

    python tools/sweep_timing.py [--sizes 512x512,1920x1080] [--repeats 30] [--out profiles/sweep_timing.json]
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

RADII = (("r0", 0.0), ("r1", 0.01), ("r5", 0.05))       # of the scene box's diagonal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import denoise_ref as dr
    L = _native.hip()
    out = {"tool": "sweep_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=4, spp=1)
        bufs = []
        try:
            n = w * h
            p = state.params
            info = pt.getBvhInfo(state)
            lo, hi = np.array([float(x) for x in info.scene_lo]), np.array([float(x) for x in info.scene_hi])
            diag = float(np.sqrt(((hi - lo) ** 2).sum()))
            rays = dr.pixel_rays(w, h, p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple())
            rays[:, 6], rays[:, 7] = 0.0, np.inf
            for nbytes in (n * 32, n * 32, n * 8):          # sweeps / rays, records / bytes, visit counts
                q = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(q), nbytes) == 0
                bufs.append(q.value)
            d_in, d_out, d_visits = bufs

            def timed(fn):
                assert fn() == 0, L.pt_last_error(state.context)      # warm-up: code object load, first-use allocations
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            def counted(name):
                assert L.pt_debug_sweep_visits(state.context, d_in, n, d_out, d_visits) == 0, L.pt_last_error(state.context)
                vis = np.zeros((n, 2), np.uint32); rec = np.zeros((n, 8), np.float32)
                assert L.pt_copy_to_host(state.context, vis.ctypes.data, d_visits, vis.nbytes) == 0
                assert L.pt_copy_to_host(state.context, rec.ctypes.data, d_out, rec.nbytes) == 0
                visits[name] = {"nodes_mean": round(float(vis[:, 0].mean()), 2), "triangles_mean": round(float(vis[:, 1].mean()), 2),
                                "nodes_max": int(vis[:, 0].max()), "triangles_max": int(vis[:, 1].max())}
                answers[name] = {"hit_share": round(float((rec[:, 0] >= 0).mean()), 4), "start_overlap_share": round(float((rec[:, 0] == 0).mean()), 4)}

            ms, visits, answers = {}, {}, {}
            assert L.pt_copy_to_device(state.context, d_in, rays.ctypes.data, rays.nbytes) == 0
            ms["closest"] = timed(lambda: L.pt_query_closest(state.context, d_in, n, d_out))
            for name, share in RADII:
                sweeps = rays.copy()
                sweeps[:, 6] = share * diag
                assert L.pt_copy_to_device(state.context, d_in, sweeps.ctypes.data, sweeps.nbytes) == 0
                ms["sweep_" + name] = timed(lambda: L.pt_query_sweep(state.context, d_in, n, d_out))
                ms["any_" + name] = timed(lambda: L.pt_query_sweep_any(state.context, d_in, n, d_out))
                counted(name)
                if name == "r1":
                    sweeps = np.ascontiguousarray(sweeps[np.random.default_rng(1).permutation(n)])
                    assert L.pt_copy_to_device(state.context, d_in, sweeps.ctypes.data, sweeps.nbytes) == 0
                    ms["sweep_r1_permuted"] = timed(lambda: L.pt_query_sweep(state.context, d_in, n, d_out))
                    counted("r1_permuted")
            out["sizes"].append({
                "width": w, "height": h, "sweeps": n, "diagonal": diag, "radii": {name: share * diag for name, share in RADII},
                "triangles": int(info.n_tris), "stack_entries": int(info.stack_entries),
                "ms": {k: round(v, 4) for k, v in ms.items()},
                "msweeps_per_s": {k: round(n / v / 1e3, 1) for k, v in ms.items()},
                "visits": visits, "answers": answers,
                "sweep_r0_over_closest": round(ms["sweep_r0"] / ms["closest"], 3),
                "sweep_r1_over_closest": round(ms["sweep_r1"] / ms["closest"], 3),
                "sweep_r5_over_closest": round(ms["sweep_r5"] / ms["closest"], 3),
                "permuted_over_coherent_r1": round(ms["sweep_r1_permuted"] / ms["sweep_r1"], 3),
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
