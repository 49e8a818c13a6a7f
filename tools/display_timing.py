#!/usr/bin/env python3
"""Times the display transform (pt_display_transform) against pt_resolve_framebuffer and prints ONE JSON line.

Per size and image, in one process and on the same buffers: host wall time of each call (all return synchronised; median of
--repeats after a warm-up) of
    auto     pt_display_transform, automatic exposure, ACES, out_rgba and the frame buffer: three kernels, about 52 B per pixel
             (16 read by the histogram; 16 read, 16 + 4 written by the apply pass)
    manual   the same with a manual exposure: the apply kernel alone, 36 B per pixel
    resolve  pt_resolve_framebuffer: one kernel, 20 B per pixel — the yardstick
Images: the accumulation of a Cornell box launch (many bins per wave) and a flat grey image (all 64 lanes of every wave in one
bin); flat_over_cornell is what the contention in the LDS histogram costs.  Per-kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/display_timing.py` (k_display_histogram, k_display_meter, k_display_apply).

    python tools/display_timing.py [--sizes 512x512,1920x1080] [--repeats 30]
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
    ap.add_argument("--spp", type=int, default=8)
    a = ap.parse_args()
    assert a.repeats >= 20
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "display_timing", "repeats": a.repeats, "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        n = w * h
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=8, direct_lighting=True,
                            importance_sampling=True, spp=a.spp)
        bufs = []
        try:
            state.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(None, state)
            for nbytes in (n * 16, n * 16, n * 4):
                p = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(p), nbytes) == 0
                bufs.append(p.value)
            flat, dst, fb = bufs
            grey = np.full((n, 4), 0.5, np.float32)
            assert L.pt_copy_to_device(state.context, flat, grey.ctypes.data, grey.nbytes) == 0

            def timed(fn):
                fn()                                        # warm-up: code object load, the context's record
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            def params(exposure):
                return _native.DisplayParams(_native.TONE_ACES, exposure, 0.18, 4.0, 100, 900, 2.0 ** -16, 2.0 ** 16, 0.0, 1.0)

            row = {"width": w, "height": h, "model_bytes": {"auto": n * 52, "manual": n * 36, "resolve": n * 20}}
            for name, src in (("cornell", state.params.accumulationBuffer), ("flat", flat)):
                auto, manual = params(0.0), params(1.0)
                info = _native.DisplayInfo()
                t = {"auto_ms": timed(lambda: L.pt_display_transform(state.context, src, n, C.byref(auto), dst, fb, C.byref(info))),
                     "manual_ms": timed(lambda: L.pt_display_transform(state.context, src, n, C.byref(manual), dst, fb, None)),
                     "resolve_ms": timed(lambda: L.pt_resolve_framebuffer(state.context, src, fb, n))}
                t["auto_over_resolve"] = t["auto_ms"] / t["resolve_ms"]
                t["manual_over_resolve"] = t["manual_ms"] / t["resolve_ms"]
                t["bins_in_use"] = int(np.count_nonzero(np.array(info.histogram)))
                t["exposure"] = float(info.exposure)
                row[name] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()}
            row["flat_over_cornell"] = round(row["flat"]["auto_ms"] / row["cornell"]["auto_ms"], 4)
            out["sizes"].append(row)
        finally:
            for b in bufs:
                L.pt_device_free(state.context, b)
            pt.CleanAllTheThings(state)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
