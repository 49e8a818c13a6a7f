#!/usr/bin/env python3
"""Times in-place vertex updates (pt_update_vertices, PT_UPDATE_REFIT) against pt_set_scene and sweeps the tree quality a refit
leaves behind; prints ONE JSON line.

1. Update cost.  The Cornell box (1 264 triangles) and the 1.31 M-triangle stress scene (scenes/make_scenes.py --stress): host wall
   time of pt_set_scene (upload + build in the default build mode) and of a refit (pt_update_info.ms: upload of the vertices plus the
   kernels), first call (it also uploads the index buffer and measures the built tree's area) and the median of --repeats later ones,
   each to a fresh seeded 1 % jitter.  Byte model of the refit: the vertices up (16 B each), the leaf pass (index 12 B, record 48 B
   read + 48 B written, shade record 16 B read + 16 B written per triangle), the node pass (node 64 B written, two 16 B boxes written and
   read, parents 4 B per node and leaf) and the fp16 re-encode (64 B read, 32 B written per node).  Per-kernel times come from running
   this under `rocprofv3 --kernel-trace --stats -- python tools/update_timing.py` (k_rf_leaves, k_rf_parents, k_rf_refit, k_rf_stats,
   k_hc_nodes).
2. Threshold curve.  On the stress scene, every sphere is translated by a seeded random vector of length up to --sweep units; the tree
   of the original scene is refitted to it.  Per step: area_ratio, and the render rate (Mray/s, 512 x 512, --spp samples, depth 6,
   direct lighting and importance sampling) of the refitted tree next to that of a fresh build of the same vertices.

    python tools/update_timing.py [--repeats 10] [--spp 8] [--sweep 0,1,3,10,30,60,100,200] [--skip-stress]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def object_vertices(path, prefix):
    """{object name: 0-based vertex indices its faces reference} for the OBJ objects whose name starts with prefix."""
    out, obj, nv = {}, "", 0
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "o":
            obj = t[1]
        elif t[0] == "v":
            nv += 1
        elif t[0] == "f" and obj.startswith(prefix):
            s = out.setdefault(obj, set())
            for w in t[1:]:
                k = int(w.split("/")[0])
                s.add(k - 1 if k > 0 else nv + k)
    return {k: sorted(v) for k, v in out.items()}


class Scene:
    def __init__(self, L, obj):
        import numpy as np
        self.L = L
        self.ctx = C.c_void_p()
        assert L.pt_create(C.byref(self.ctx), 0) == 0
        self.idx = np.ascontiguousarray(obj.getIndexBuffer(), np.uint32)
        self.mid = np.ascontiguousarray(obj.getMaterialIndices(), np.uint32)
        self.mats = obj.getMaterials()

    def set_scene(self, v):
        t0 = time.perf_counter()
        assert self.L.pt_set_scene(self.ctx, v.ctypes.data, v.size // 4, self.idx.ctypes.data, self.idx.size // 3, self.mid.ctypes.data,
                                   C.addressof(self.mats), len(self.mats)) == 0, self.L.pt_last_error(self.ctx)
        return (time.perf_counter() - t0) * 1e3

    def refit(self, v):
        from acgpathtracing_amd import _native
        info = _native.UpdateInfo()
        assert self.L.pt_update_vertices(self.ctx, v.ctypes.data, v.size // 4, _native.UPDATE_REFIT, C.byref(info)) == 0, \
            self.L.pt_last_error(self.ctx)
        return info

    def mrays(self, spp):
        """Mray/s of one 512 x 512 launch (median of three after a warm-up)."""
        import numpy as np
        from acgpathtracing_amd import _native
        from scene_utils import make_params
        L, ctx = self.L, self.ctx
        acc = C.c_void_p()
        assert L.pt_device_malloc(ctx, C.byref(acc), 512 * 512 * 16) == 0
        try:
            q = make_params(512, 512, spp, 6, True, True)
            q.accumulationBuffer, q.frameBuffer, q.handle = acc.value, None, L.pt_scene_handle(ctx)
            rates = []
            for i in range(4):
                q.currentFrameIdx = i
                assert L.pt_launch(ctx, C.byref(q)) == 0, L.pt_last_error(ctx)
                st = _native.Stats()
                assert L.pt_get_stats(ctx, C.byref(st)) == 0
                if i:
                    rates.append((st.radiance_rays + st.shadow_rays) / st.kernel_ms / 1e3)
            return float(np.median(rates))
        finally:
            L.pt_device_free(ctx, acc)

    def close(self):
        self.L.pt_destroy(self.ctx)


def cost(L, name, path, repeats):
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    obj = pt.TinyObjWrapper(path)
    v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    s = Scene(L, obj)
    try:
        builds = [s.set_scene(v) for _ in range(3)]
        ext = float((v[:, :3].max(axis=0) - v[:, :3].min(axis=0)).max())
        rng = np.random.default_rng(1)

        def jitter():
            w = v.copy()
            w[:, :3] += rng.uniform(-0.01 * ext, 0.01 * ext, size=(len(v), 3)).astype(np.float32)
            return w

        first = s.refit(jitter())
        later = [s.refit(jitter()) for _ in range(repeats)]
        b = _native.BvhInfo()
        assert L.pt_get_bvh_info(s.ctx, C.byref(b)) == 0
        n, m, nv = int(b.n_tris), int(b.n_nodes), len(v)
        return {"scene": name, "n_tris": n, "n_verts": nv, "set_scene_ms": round(float(np.median(builds)), 3),
                "refit_first_ms": round(first.ms, 3), "refit_ms": round(float(np.median([i.ms for i in later])), 3),
                "area_ratio_1pct_jitter": round(float(np.median([i.area_ratio for i in later])), 4),
                "model_bytes": {"upload": nv * 16, "leaf_pass": n * (12 + 48 + 48 + 16 + 16) + nv * 16,
                                "node_pass": m * (64 + 32 + 32 + 4) + n * 4, "fp16_encode": m * (64 + 32)}}
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--sweep", default="0,1,3,10,30,60,100,200")
    ap.add_argument("--skip-stress", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "update_timing", "auto_area_ratio": _native.UPDATE_AUTO_AREA_RATIO, "cost": [], "sweep": []}
    out["cost"].append(cost(L, "cornell_box", os.path.join(pt.SCENES, "cornell_box.obj"), a.repeats))
    if not a.skip_stress:
        sys.path.insert(0, pt.SCENES)
        import make_scenes
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "stress.obj")
            make_scenes.stress_scene(path)
            out["cost"].append(cost(L, "stress_1m", path, a.repeats))
            obj = pt.TinyObjWrapper(path)
            v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
            spheres = list(object_vertices(path, "s").values())
            rng = np.random.default_rng(5)
            dirs = rng.normal(size=(len(spheres), 3))
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            lens = rng.uniform(0.0, 1.0, size=len(spheres))
            upd, fresh = Scene(L, obj), Scene(L, obj)
            try:
                upd.set_scene(v)
                base = upd.mrays(a.spp)
                for amp in (float(x) for x in a.sweep.split(",")):
                    w = v.copy()
                    for k, ids in enumerate(spheres):
                        w[ids, :3] += (dirs[k] * lens[k] * amp).astype(np.float32)
                    info = upd.refit(w)
                    fresh.set_scene(w)
                    out["sweep"].append({"displacement": amp, "area_ratio": round(info.area_ratio, 4), "refit_ms": round(info.ms, 3),
                                         "mrays_refit": round(upd.mrays(a.spp), 1), "mrays_fresh": round(fresh.mrays(a.spp), 1)})
                out["mrays_built"] = round(base, 1)
            finally:
                upd.close()
                fresh.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
