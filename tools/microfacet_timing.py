#!/usr/bin/env python3
"""Cost of the microfacet material model (pt_set_material_model) in the light-mode-1 render kernels; prints ONE JSON line.  Meant to
run under `rocprofv3 --kernel-trace --stats -- python tools/microfacet_timing.py` (per-kernel times: k_render_pw / k_render_env rows 8
and 12 against k_render_ggx / k_render_ggx_env).

Per scene (the Cornell box with its purple metal, Pr 0.2, and its glass, at 1920 x 1080, 128 spp per step, 8 bounces, both toggles on;
and the 1.31 M-triangle stress scene of bench.py config 5), launches of --fuse steps each, kernel time (HIP events, pt_stats.kernel_ms):
  lights         light mode 1, the reference's materials (LIGHTS, row 8);
  lights_ggx     light mode 1, PT_MATERIALS_MICROFACET (LIGHTS GGX, row 13): rough metal takes light samples;
  lights_env     ... with a 1024 x 512 sun-and-sky map (LIGHTS ENV, row 12);
  lights_ggx_env ... and the microfacet model (LIGHTS GGX ENV, row 14).

    python tools/microfacet_timing.py [--launches 3] [--fuse 2] [--skip-stress]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from env_timing import run, sky  # noqa: E402


def scene(pt, bench, name, depth, launches, fuse, img):
    state, _ = pt.setup(bench.scene_path(pt, name), width=1920, height=1080, max_depth=depth, direct_lighting=True,
                        importance_sampling=True, spp=bench.SPP_PER_LAUNCH)
    L = pt._native.hip()
    out = {"scene": name, "size": [1920, 1080], "spp_per_step": bench.SPP_PER_LAUNCH, "steps_per_launch": fuse}
    try:
        pt.setLightMode(state, 1)
        out["lights"] = run(L, pt, state, launches, fuse)
        pt.setMaterialModel(state, "microfacet")
        out["lights_ggx"] = run(L, pt, state, launches, fuse)
        pt.setEnvironment(state, img)
        out["lights_ggx_env"] = run(L, pt, state, launches, fuse)
        pt.setMaterialModel(state, "reference")
        out["lights_env"] = run(L, pt, state, launches, fuse)
        for a, b in (("lights_ggx", "lights"), ("lights_ggx_env", "lights_env")):
            out[a + "_over_" + b] = out[a]["kernel_ms_per_step"] / out[b]["kernel_ms_per_step"]
        out["variant_names"] = {str(v): L.pt_variant_name(v).decode() for v in sorted({out[k]["variant"] for k in ("lights", "lights_ggx", "lights_env", "lights_ggx_env")})}
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
    res = {"tool": "microfacet_timing", "cornell": scene(pt, bench, "cornell_box.obj", 8, a.launches, a.fuse, img)}
    if not a.skip_stress:
        res["stress"] = scene(pt, bench, bench.PRESETS[5][0], bench.PRESETS[5][2], a.launches, 1, img)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
