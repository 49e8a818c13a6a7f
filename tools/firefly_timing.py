#!/usr/bin/env python3
"""Times the firefly filter (pt_firefly_filter) against pt_display_transform in manual mode and prints ONE JSON line (also written to
profiles/firefly_timing.json with --write).

Per size, in one process and on the same buffers: host wall time of each synchronised call (median of --repeats after a warm-up) of
    r1, r2   pt_firefly_filter with radius 1 and 2 (rank 1, ratio 16, info asked for): one 16-byte read per pixel times the halo
             factor (18 / 16)^2 or (20 / 16)^2, one 16-byte store: 36.25 or 41 B per pixel
    display  pt_display_transform, manual exposure, ACES, out_rgba and the frame buffer: one kernel, a 16-byte read, a 16-byte store
             and a 4-byte store, 36 B per pixel — the yardstick
The source is the accumulation of one 8-spp Cornell box launch.  The three calls are timed in interleaved rounds.

    python tools/firefly_timing.py [--sizes 512x512,1920x1080] [--repeats 30] [--write]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    assert a.repeats >= 20
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "firefly_timing", "repeats": a.repeats, "kernel_source_hash": L.pt_kernel_source_hash().decode(), "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        n = w * h
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=8, direct_lighting=True,
                            importance_sampling=True, spp=8)
        bufs = []
        try:
            for nbytes in (n * 16, n * 4):
                p = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(p), nbytes) == 0
                bufs.append(p.value)
            dst, fb = bufs
            pt.LaunchCurrentFrame(None, state)
            src = state.params.accumulationBuffer
            info = _native.FireflyInfo()
            manual = _native.DisplayParams(_native.TONE_ACES, 1.0, 0.18, 4.0, 100, 900, 2.0 ** -16, 2.0 ** 16, 0.0, 1.0)
            calls = {"r1": lambda: L.pt_firefly_filter(state.context, src, w, h, C.byref(_native.FireflyParams(16.0, 0.01, 1, 1)), dst, C.byref(info)),
                     "r2": lambda: L.pt_firefly_filter(state.context, src, w, h, C.byref(_native.FireflyParams(16.0, 0.01, 1, 2)), dst, C.byref(info)),
                     "display": lambda: L.pt_display_transform(state.context, src, n, C.byref(manual), dst, fb, None)}
            ts = {k: [] for k in calls}
            for k, fn in calls.items():
                assert fn() == 0, L.pt_last_error(state.context)          # warm-up: code object load, the context's record
            for _ in range(a.repeats):
                for k, fn in calls.items():
                    t0 = time.perf_counter()
                    rc = fn()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            spread = {k: float(np.percentile(v, 75) - np.percentile(v, 25)) for k, v in ts.items()}
            model = {"r1": 16.0 * (18.0 / 16.0) ** 2 + 16.0, "r2": 16.0 * (20.0 / 16.0) ** 2 + 16.0, "display": 36.0}
            row = {"width": w, "height": h, "clamped_pixels": int(info.clamped_pixels), "model_bytes_per_pixel": model}
            for k in calls:
                row[k + "_ms"] = round(med[k], 4)
                row[k + "_iqr_ms"] = round(spread[k], 4)
            for k in ("r1", "r2"):
                row[k + "_over_display"] = round(med[k] / med["display"], 4)
                row[k + "_model_ratio"] = round(model[k] / model["display"], 4)
            out["sizes"].append(row)
        finally:
            for b in bufs:
                L.pt_device_free(state.context, b)
            pt.CleanAllTheThings(state)
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "firefly_timing.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
