#!/usr/bin/env python3
"""Times the temporal reprojection (pt_temporal_blend, pt_temporal_blend_motion) on the Cornell box and prints ONE JSON line.

Per size: a history at the reference camera and an accumulation at the camera of acgpt_main --orbit 20,0, both one launch of --spp,
with their features (pt_render_features).  Host wall time of the first call (it builds the per-triangle bsdfType array: one memset
and the k_tp_tri_bsdf scatter) and the median of --repeats later calls (all return synchronised), the share of pixels that take
history, and the byte model of k_tp_blend: per pixel 48 B of the current view (accumulation + two feature buffers), up to four
taps x 48 B of the previous one (history + two feature buffers), 16 B written.  Per-kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/temporal_timing.py` (k_tp_blend<false>, k_tp_blend<true>, k_tp_tri_bsdf).

The motion call runs on the same views with every vertex of the previous positions jittered (seeded), so that every diffuse hit pays
for the motion step: the same medians for clip_gamma 0 (motion_ms) and the default (motion_clip_ms), the first motion call (it uploads
the index buffer), and the added bytes per diffuse hit: 12 B of indices and six 16-B vertex loads, plus nine 16-B accumulation taps
with the clip.

    python tools/temporal_timing.py [--sizes 512x512,1920x1080] [--repeats 20] [--spp 8]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import temporal_ref as tr
    L = _native.hip()
    out = {"tool": "temporal_timing", "cap": pt.TEMPORAL_HISTORY_CAP, "sizes": []}
    for wh in a.sizes.split(","):
        w, h = (int(v) for v in wh.split("x"))
        state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=w, height=h, max_depth=8, direct_lighting=True,
                            importance_sampling=True, spp=a.spp)
        bufs = []
        try:
            for _ in range(5):
                p = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(p), w * h * 16) == 0
                bufs.append(p.value)
            hist, alb0, nd0, alb1, nd1 = bufs
            prev = pt.PathTraceParams()
            C.memmove(C.byref(prev), C.byref(state.params), C.sizeof(prev))
            prev.accumulationBuffer, prev.currentFrameIdx = hist, 0
            assert L.pt_launch(state.context, C.byref(prev)) == 0
            assert L.pt_render_features(state.context, C.byref(prev), alb0, nd0) == 0
            tr.set_camera(state.params, *tr.orbit_camera(w, h, 20, 0))
            state.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(None, state)
            launch_ms = pt.getStats(state).launch_ms
            assert L.pt_render_features(state.context, C.byref(state.params), alb1, nd1) == 0
            dst = C.c_void_p()
            assert L.pt_device_malloc(state.context, C.byref(dst), w * h * 16) == 0
            bufs.append(dst.value)

            def call():
                return L.pt_temporal_blend(state.context, C.byref(state.params), a.spp, alb1, nd1, C.byref(prev), hist, alb0, nd0,
                                           pt.TEMPORAL_HISTORY_CAP, dst.value)

            t0 = time.perf_counter()
            assert call() == 0, L.pt_last_error(state.context)
            first_ms = (time.perf_counter() - t0) * 1e3
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                rc = call()
                ts.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0, L.pt_last_error(state.context)
            res = np.zeros((h, w, 4), np.float32)
            assert L.pt_copy_to_host(state.context, res.ctypes.data, dst.value, res.nbytes) == 0
            px = w * h
            # the motion call: the scene's positions now and a jittered copy as the previous view's
            verts = np.ascontiguousarray(state._scene_verts, np.float32)
            jit = verts.copy()
            jit[:, :3] += np.random.default_rng(7).normal(scale=0.5, size=(verts.shape[0], 3)).astype(np.float32)
            vd = []
            for arr in (verts, jit):
                p = C.c_void_p()
                assert L.pt_device_malloc(state.context, C.byref(p), arr.nbytes) == 0
                bufs.append(p.value)
                vd.append(p.value)
                assert L.pt_copy_to_device(state.context, p.value, arr.ctypes.data, arr.nbytes) == 0

            def call_motion(gamma):
                return L.pt_temporal_blend_motion(state.context, C.byref(state.params), a.spp, alb1, nd1, C.byref(prev), hist, alb0, nd0,
                                                  vd[0], vd[1], verts.shape[0], pt.TEMPORAL_HISTORY_CAP, gamma, dst.value)

            t0 = time.perf_counter()
            assert call_motion(0.0) == 0, L.pt_last_error(state.context)
            first_motion_ms = (time.perf_counter() - t0) * 1e3
            motion = {}
            for name, gamma in (("motion_ms", 0.0), ("motion_clip_ms", pt.TEMPORAL_CLIP_GAMMA)):
                ts_m = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rc = call_motion(gamma)
                    ts_m.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, L.pt_last_error(state.context)
                motion[name] = round(float(np.median(ts_m)), 4)
            res_m = np.zeros((h, w, 4), np.float32)
            assert L.pt_copy_to_host(state.context, res_m.ctypes.data, dst.value, res_m.nbytes) == 0
            alb = np.zeros((h, w, 4), np.float32)
            assert L.pt_copy_to_host(state.context, alb.ctypes.data, alb1, alb.nbytes) == 0
            prim = alb[..., 3].view(np.uint32)
            bsdf = tr.tri_bsdf(pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj")))
            diffuse_hits = int((bsdf[prim[prim < bsdf.size]] == 0).sum())
            out["sizes"].append({
                "width": w, "height": h, "spp": a.spp, "spp_launch_ms": round(launch_ms, 3),
                "first_call_ms": round(first_ms, 4), "blend_ms": round(float(np.median(ts)), 4),
                "take_history": round(float((res[..., 3] != a.spp).mean()), 4),
                "n_tris": pt.getBvhInfo(state).n_tris,
                "model_bytes": px * (48 + 4 * 48 + 16),
                "first_motion_call_ms": round(first_motion_ms, 4), **motion,
                "motion_take_history": round(float((res_m[..., 3] != a.spp).mean()), 4),
                "diffuse_hits": diffuse_hits,
                "motion_model_bytes": px * (48 + 4 * 48 + 16) + diffuse_hits * (12 + 6 * 16),
                "motion_clip_model_bytes": px * (48 + 4 * 48 + 16) + diffuse_hits * (12 + 6 * 16 + 9 * 16),
            })
        finally:
            for b in bufs:
                L.pt_device_free(state.context, b)
            pt.CleanAllTheThings(state)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
