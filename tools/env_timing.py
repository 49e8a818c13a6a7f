#!/usr/bin/env python3
"""Cost of the environment map in the render kernel; prints ONE JSON line.  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/env_timing.py` (per-kernel times: k_render_pw, k_render_env, k_env_rows, k_env_marginal).

Per scene (bench.py config 2: the diffuse Cornell box at 1920 x 1080, 128 spp per step, 8 bounces, both toggles on; and the
1.31 M-triangle stress scene of config 5), launches of --fuse steps each, kernel time (HIP events, pt_stats.kernel_ms) and rays:
  default      no map: today's kernel (variant 7 / 9);
  env_black    ENV (or ENV deep) with an all-black map: the cost of the map's code paths with nothing to look up (the "outside" pixel
               class is off in the ENV kernels, so the camera rays that miss the scene box are now shaded misses);
  env_map      ENV with a 1024 x 512 map: the lookups of every miss, camera rays past the scene box included;
  lights       light mode 1 without a map (variant 8), and
  lights_env   light mode 1 with the map (LIGHTS ENV): the map's binary searches in every diffuse light sample.
Also the host wall time of pt_set_environment for the 1024 x 512 map (upload + the two CDF kernels).

    python tools/env_timing.py [--launches 3] [--fuse 2] [--skip-stress]
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


def sky(h=512, w=1024):
    import numpy as np
    v = (np.arange(h) + 0.5) / h
    img = np.zeros((h, w, 3), np.float32)
    img[...] = (0.3 + 0.5 * (1 - v))[:, None, None] * np.array([0.6, 0.8, 1.0], np.float32)
    img[h // 5:h // 5 + 6, w // 3:w // 3 + 6] = (5000.0, 4600.0, 4000.0)       # a sun
    return img


def run(L, pt, state, launches, fuse):
    ms, rays = [], 0
    for _ in range(launches):
        state.params.currentFrameIdx = 0
        assert L.pt_launch_frames(state.context, C.byref(state.params), fuse) == 0, L.pt_last_error(state.context)
        st = pt.getStats(state)
        ms.append(float(st.kernel_ms))
        rays = int(st.radiance_rays + st.shadow_rays)
    best = min(ms)
    return {"variant": int(st.variant), "kernel_ms_per_step": best / fuse, "Mray_per_s": rays / (best * 1e-3) / 1e6,
            "culled_rays": int(st.culled_rays)}


def scene(pt, bench, config, launches, fuse, img):
    import numpy as np
    name, _, depth, w, h, dl, is_ = bench.PRESETS[config]
    state, _ = pt.setup(bench.scene_path(pt, name), width=w, height=h, max_depth=depth, direct_lighting=bool(dl),
                        importance_sampling=bool(is_), spp=bench.SPP_PER_LAUNCH)
    L = pt._native.hip()
    out = {"scene": name, "size": [w, h], "spp_per_step": bench.SPP_PER_LAUNCH, "steps_per_launch": fuse}
    try:
        out["default"] = run(L, pt, state, launches, fuse)
        pt.setEnvironment(state, np.zeros((4, 8, 3), np.float32))
        out["env_black"] = run(L, pt, state, launches, fuse)
        t0 = time.perf_counter()
        pt.setEnvironment(state, img)
        out["set_environment_ms_1024x512"] = (time.perf_counter() - t0) * 1e3
        out["env_map"] = run(L, pt, state, launches, fuse)
        pt.setEnvironment(state, None)
        pt.setLightMode(state, 1)
        out["lights"] = run(L, pt, state, launches, fuse)
        pt.setEnvironment(state, img)
        out["lights_env"] = run(L, pt, state, launches, fuse)
        out["variant_names"] = {str(v): L.pt_variant_name(v).decode() for v in sorted({out[k]["variant"] for k in ("default", "env_black", "env_map", "lights", "lights_env")})}
    finally:
        pt.CleanAllTheThings(state)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--fuse", type=int, default=2)
    ap.add_argument("--skip-stress", action="store_true")
    a = ap.parse_args()
    import bench
    import acgpathtracing_amd as pt
    img = sky()
    res = {"tool": "env_timing", "config2": scene(pt, bench, 2, a.launches, a.fuse, img)}
    if not a.skip_stress:
        res["config5"] = scene(pt, bench, 5, a.launches, 1, img)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
