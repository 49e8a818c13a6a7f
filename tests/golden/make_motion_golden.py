#!/usr/bin/env python3
"""Generate tests/golden/motion_cornell_128.npz: the converged images of the moved scene that tests/test_motion_host.py measures the
motion blend (pt_temporal_blend_motion) against.

The CPU oracle (oracle/oracle_pt.cpp) renders cornell_box_diffuse.obj with its sphere (material glass, Lambertian in this scene)
moved by motion_ref.SPHERE_MOVE = (-40, 0, +30) — on the floor, clear of both blocks, about 10 px at 128 x 128 —, at 128 x 128,
maxDepth 8, direct lighting and importance sampling on, 32 progressive frames of 256 samples per pixel (8192 in all), twice: at the
reference's camera (ref) and at the camera of acgpt_main --orbit 20,0 (ref_orbit).  About two minutes per image on eight cores.
Deterministic.

    python tests/golden/make_motion_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
os.environ.setdefault("ACGPT_TORCH_FIRST", "0")
import acgpathtracing_amd as pt  # noqa: E402
import motion_ref as mr  # noqa: E402
import oracle_lib  # noqa: E402
import temporal_ref as tr  # noqa: E402
from scene_utils import copy_params, make_params  # noqa: E402

SIZE, DEPTH, FRAMES, SPP = 128, 8, 32, 256
ORBIT = (20, 0)


def main():
    path = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
    obj = pt.TinyObjWrapper(path)
    verts = mr.translated(obj.getVerticesFloat(), mr.object_vertices(path, "glass_sphere"), mr.SPHERE_MOVE)
    orc = oracle_lib.load()
    sc = orc.scene(verts.reshape(-1), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    refs = []
    for orbit in ((0, 0), ORBIT):
        cam = tr.orbit_camera(SIZE, SIZE, *orbit)
        acc = None
        for f in range(FRAMES):
            p = tr.set_camera(make_params(SIZE, SIZE, SPP, DEPTH, True, True, frame=f), *cam)
            acc, _, _, _ = sc.render(copy_params(p), accumulation=acc)
        refs.append(np.ascontiguousarray(acc[..., :3], np.float32))
    out = os.path.join(HERE, "motion_cornell_128.npz")
    np.savez_compressed(out, ref=refs[0], ref_orbit=refs[1],
                        meta=np.array([SIZE, SIZE, DEPTH, FRAMES, SPP, ORBIT[0], ORBIT[1]], np.int32),
                        move=np.array(mr.SPHERE_MOVE, np.float32))
    print("wrote", out)


if __name__ == "__main__":
    main()
