#!/usr/bin/env python3
"""Times the bloom (pt_bloom) against pt_display_transform and prints ONE JSON line.

Per size, in one process and on the same image: host wall time of each call (both return synchronised; median of --repeats after a
warm-up) of
    bloom_L   pt_bloom with the defaults and L = 1, 4, 6, 8 levels requested, info NULL: 2 n + 1 kernels for the n levels built.  The
              byte model: the source read twice (prefilter, composite) and the output written once, 48 B per pixel, plus the pyramid:
              level 1 (a quarter frame, 4 B per pixel) written, read by the next down step, read, written and read again on the way
              up, and a third of that again for the further levels: about 4/3 * 20 B, 27 B per pixel at full depth, 8 B at one level
    display   pt_display_transform, automatic exposure, ACES, out_rgba and the frame buffer, info NULL: three kernels, about 52 B per
              pixel — the yardstick
The image is the accumulation of one Cornell box launch.  Per-kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/bloom_timing.py` (k_bloom_down<true>, k_bloom_down<false>, k_bloom_up,
k_bloom_finish).

    python tools/bloom_timing.py [--sizes 512x512,1920x1080] [--repeats 30] [--json profiles/bloom_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = (1, 4, 6, 8)


def levels_of(w, h, levels):
    out = []
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
        if w == 1 and h == 1:
            break
    return out


def model_bytes(w, h, levels):
    """what one call moves: the source twice and the output once; every level written by its down step and read by the composite or
    the up step below it; every level but the last read by the next down step and read and written in place by its own up step"""
    lv = [a * b for a, b in levels_of(w, h, levels)]
    return 48 * w * h + sum(16 * t * 2 for t in lv) + sum(16 * t * 3 for t in lv[:-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert a.repeats >= 20
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "bloom_timing", "repeats": a.repeats, "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        n = w * h
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=8, direct_lighting=True,
                            importance_sampling=True, spp=a.spp)
        bufs = []
        try:
            for nbytes in (n * 16, n * 4):
                p = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(p), nbytes) == 0
                bufs.append(p.value)
            dst, fb = bufs
            state.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(None, state)
            src = state.params.accumulationBuffer

            def timed(fn):
                fn()                                        # warm-up: code object load, the context's record and pyramid
                ts = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                return float(np.median(ts))

            auto = _native.DisplayParams(_native.TONE_ACES, 0.0, 0.18, 4.0, 100, 900, 2.0 ** -16, 2.0 ** 16, 0.0, 1.0)
            d = pt.BLOOM_DEFAULTS
            t = {"display_ms": timed(lambda: L.pt_display_transform(state.context, src, n, C.byref(auto), dst, fb, None))}
            row = {"width": w, "height": h, "model_bytes": {"display": n * 52}, "levels_built": {}}
            for lv in LEVELS:
                bp = _native.BloomParams(d["threshold"], d["knee"], d["clamp"], d["intensity"], d["spread"], lv)
                info = _native.BloomInfo()
                assert L.pt_bloom(state.context, src, w, h, C.byref(bp), dst, C.byref(info)) == 0, L.pt_last_error(state.context)
                row["levels_built"][str(lv)] = int(info.levels)
                row["bright_pixels"] = int(info.bright_pixels)
                t["bloom_%d_ms" % lv] = timed(lambda: L.pt_bloom(state.context, src, w, h, C.byref(bp), dst, None))
                t["bloom_%d_over_display" % lv] = t["bloom_%d_ms" % lv] / t["display_ms"]
                row["model_bytes"]["bloom_%d" % lv] = model_bytes(w, h, lv)
                row["model_bytes"]["bloom_%d_over_display" % lv] = round(model_bytes(w, h, lv) / (n * 52), 4)
            t["display_again_ms"] = timed(lambda: L.pt_display_transform(state.context, src, n, C.byref(auto), dst, fb, None))
            row.update({k: round(v, 4) for k, v in t.items()})
            out["sizes"].append(row)
        finally:
            for b in bufs:
                L.pt_device_free(state.context, b)
            pt.CleanAllTheThings(state)
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
