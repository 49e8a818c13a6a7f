#!/usr/bin/env python3
"""Times material edits (pt_update_materials) against pt_set_scene; prints ONE JSON line.

The Cornell box (1 264 triangles) and the 1.31 M-triangle stress scene (scenes/make_scenes.py stress_scene, the scene
tools/make_big_scene.py --spheres 64 --subdiv 5 writes).  Per scene: the host wall time of pt_set_scene (upload + build in the default
build mode, median of three), and pt_update_info.ms (host wall time of the whole call) of three kinds of edit, first call and median of
--repeats later ones, each a fresh seeded change:
  table          a new table, ids kept (a recolour of every material);
  table_ids      a new table and a new id for every triangle (every triangle's id drawn among the scene's non-emissive materials);
  table_ids_lit  the same with every 8th triangle given the emissive material: light mode 1's list holds an eighth of the scene.
Byte model per call: the table up (32 B per material), ids up (4 B per triangle, table_ids only), the leaf pass (record 16 B read +
16 B written, shade record 16 B read + 4 B written, id 4 B read, material 16 B read per triangle; 4 B of slot index per triangle when
the scene has lights), the gather (36 B per emissive triangle down to the host).  Per-kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/material_timing.py` (k_mt_slots, k_mt_gather).

    python tools/material_timing.py [--repeats 10] [--skip-stress]
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


def cost(L, name, path, repeats):
    import numpy as np
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    obj = pt.TinyObjWrapper(path)
    v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32)
    idx = np.ascontiguousarray(obj.getIndexBuffer(), np.uint32)
    mid = np.ascontiguousarray(obj.getMaterialIndices(), np.uint32)
    base = [_native.Material.from_buffer_copy(m) for m in obj.getMaterials()]
    table0 = (_native.Material * len(base))(*base)
    emissive = [i for i, m in enumerate(base) if (m.emission.x, m.emission.y, m.emission.z) != (0.0, 0.0, 0.0)]
    dark = np.array([i for i in range(len(base)) if i not in emissive], np.uint32)
    ctx = C.c_void_p()
    assert L.pt_create(C.byref(ctx), 0) == 0
    rng = np.random.default_rng(1)
    try:
        builds = []
        for _ in range(3):
            t0 = time.perf_counter()
            assert L.pt_set_scene(ctx, v.ctypes.data, v.size // 4, idx.ctypes.data, idx.size // 3, mid.ctypes.data, C.addressof(table0),
                                  len(table0)) == 0, L.pt_last_error(ctx)
            builds.append((time.perf_counter() - t0) * 1e3)

        def edit(kind):
            mats = [_native.Material.from_buffer_copy(m) for m in base]
            for m in mats:
                c = rng.uniform(0.05, 0.95, 3)
                m.diffuse = _native.Float3(*c)
            table = (_native.Material * len(mats))(*mats)
            ids = None
            if kind != "table":
                ids = np.ascontiguousarray(dark[rng.integers(0, len(dark), size=len(mid))], np.uint32)
                if kind == "table_ids_lit" and emissive:
                    ids[::8] = emissive[0]
            info = _native.UpdateInfo()
            rc = L.pt_update_materials(ctx, C.addressof(table), len(table), None if ids is None else ids.ctypes.data,
                                       0 if ids is None else ids.size, C.byref(info))
            assert rc == 0, L.pt_last_error(ctx)
            return info.ms

        out = {"scene": name, "n_tris": int(len(mid)), "n_mats": len(base), "set_scene_ms": round(float(np.median(builds)), 3)}
        for kind in ("table", "table_ids", "table_ids_lit"):
            first = edit(kind)
            later = [edit(kind) for _ in range(repeats)]
            out[kind] = {"first_ms": round(first, 3), "ms": round(float(np.median(later)), 3)}
        b = _native.BvhInfo()
        assert L.pt_get_bvh_info(ctx, C.byref(b)) == 0
        n = int(b.n_tris)
        out["model_bytes"] = {"table": 32 * len(base), "ids": 4 * n, "leaf_pass": n * (16 + 16 + 16 + 4 + 4 + 16)}
        return out
    finally:
        L.pt_destroy(ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--skip-stress", action="store_true")
    a = ap.parse_args()
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    out = {"tool": "material_timing", "cost": []}
    out["cost"].append(cost(L, "cornell_box", os.path.join(pt.SCENES, "cornell_box.obj"), a.repeats))
    if not a.skip_stress:
        sys.path.insert(0, pt.SCENES)
        import make_scenes
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "stress.obj")
            make_scenes.stress_scene(path)
            out["cost"].append(cost(L, "stress_1m", path, a.repeats))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
