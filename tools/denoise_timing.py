#!/usr/bin/env python3
"""Times the denoised preview (pt_render_features + pt_denoise) on the Cornell box and prints ONE JSON line.

Per size: host wall time of each call (both return synchronised; median of --repeats after a warm-up) and the byte model of the
filter: per pixel and a-trous iteration 25 taps x 32 B ({c, var} and {normal, depth}) + 9 x 4 B (variance blur) read from the
caches, 48 B of unique HBM traffic (two float4 in, one out).  Per-kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/denoise_timing.py` (k_dn_features, k_dn_variance, k_dn_atrous).

    python tools/denoise_timing.py [--sizes 512x512,1920x1080] [--iterations 5] [--repeats 20]
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
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "denoise_timing", "iterations": a.iterations, "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=8, direct_lighting=True,
                            importance_sampling=True, spp=a.spp)
        bufs = []
        try:
            state.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(None, state)
            launch_ms = pt.getStats(state).launch_ms
            for _ in range(3):
                p = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(p), w * h * 16) == 0
                bufs.append(p.value)
            alb, nd, dst = bufs

            def timed(fn):
                fn()                                        # warm-up: code object load, scratch allocation
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            f_ms = timed(lambda: L.pt_render_features(state.context, C.byref(state.params), alb, nd))
            d_ms = timed(lambda: L.pt_denoise(state.context, C.byref(state.params), alb, nd, dst, a.iterations))
            px = w * h
            out["sizes"].append({
                "width": w, "height": h, "spp_launch_ms": round(launch_ms, 3), "spp": a.spp,
                "features_ms": round(f_ms, 4), "denoise_ms": round(d_ms, 4),
                "model_cache_bytes_per_iteration": px * (25 * 32 + 9 * 4),
                "model_cache_bytes_variance_pass": px * 25 * 48,
                "model_hbm_bytes_per_iteration": px * 48,
            })
        finally:
            for b in bufs:
                L.pt_device_free(state.context, b)
            pt.CleanAllTheThings(state)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
