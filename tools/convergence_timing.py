#!/usr/bin/env python3
"""Times the convergence estimate (pt_convergence_update) against pt_display_transform and prints ONE JSON line.

Per size, in one process and on the same buffers: host wall time of each call (both return synchronised; median of --repeats after
a warm-up) of
    full     pt_convergence_update with out_error, out_tiles and info: two kernels, about 52 B per pixel (16 + 16 read, 16 + 4
             written, plus 4 B per tile)
    bare     the same with the three optional outputs NULL: 48 B per pixel
    display  pt_display_transform, automatic exposure, ACES, out_rgba and the frame buffer, info NULL: three kernels, about 52 B per pixel —
             the yardstick
The accumulation is that of two Cornell box launches; the state holds the first one's observation, so every timed call is a
measured update (step 3 of include/acgpt.h, the whole arithmetic) of the second: the state is restored from a host copy before
every call, outside the timed span.  Per-kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/convergence_timing.py` (k_convergence_update, k_convergence_meter).

    python tools/convergence_timing.py [--sizes 512x512,1920x1080] [--repeats 30]
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
    out = {"tool": "convergence_timing", "repeats": a.repeats, "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        n = w * h
        tiles = ((w + 15) // 16) * ((h + 15) // 16)
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=8, direct_lighting=True,
                            importance_sampling=True, spp=a.spp)
        bufs = []
        try:
            for nbytes in (n * 16, n * 16, n * 4, tiles * 4, n * 16, n * 4):
                p = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(p), nbytes) == 0
                bufs.append(p.value)
            st, st0, err, til, dst, fb = bufs
            assert L.pt_device_memset(state.context, st0, 0, n * 16) == 0
            cp = _native.ConvergenceParams(0.01, 0.02, 950, 0)
            info = _native.ConvergenceInfo()
            state.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(None, state)
            assert L.pt_convergence_update(state.context, C.byref(state.params), 1, C.byref(cp), st0, None, None, None) == 0
            state.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(None, state)

            def timed(fn, before=None):
                if before:
                    before()
                fn()                                        # warm-up: code object load, the context's record
                ts = []
                for _ in range(a.repeats):
                    if before:
                        before()
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            # the state of one observation, put back before every call so that every timed call measures
            host_state = np.zeros((n, 4), np.float32)
            assert L.pt_copy_to_host(state.context, host_state.ctypes.data, st0, host_state.nbytes) == 0

            def restore_from_host():
                assert L.pt_copy_to_device(state.context, st, host_state.ctypes.data, host_state.nbytes) == 0

            auto = _native.DisplayParams(_native.TONE_ACES, 0.0, 0.18, 4.0, 100, 900, 2.0 ** -16, 2.0 ** 16, 0.0, 1.0)
            t = {"full_ms": timed(lambda: L.pt_convergence_update(state.context, C.byref(state.params), 2, C.byref(cp), st, err, til, C.byref(info)), restore_from_host)}
            measured = int(info.measured_pixels)
            t["bare_ms"] = timed(lambda: L.pt_convergence_update(state.context, C.byref(state.params), 2, C.byref(cp), st, None, None, None), restore_from_host)
            t["display_ms"] = timed(lambda: L.pt_display_transform(state.context, state.params.accumulationBuffer, n, C.byref(auto), dst, fb, None))
            t["full_over_display"] = t["full_ms"] / t["display_ms"]
            t["bare_over_display"] = t["bare_ms"] / t["display_ms"]
            row = {"width": w, "height": h, "model_bytes": {"full": n * 52 + tiles * 4, "bare": n * 48, "display": n * 52}, "measured_pixels": measured,
                   "bins_in_use": int(np.count_nonzero(np.array(info.histogram))), "quantile_error": float(info.quantile_error)}
            row.update({k: round(v, 4) for k, v in t.items()})
            out["sizes"].append(row)
        finally:
            for b in bufs:
                L.pt_device_free(state.context, b)
            pt.CleanAllTheThings(state)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
