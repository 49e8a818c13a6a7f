#!/usr/bin/env python3
"""Generate tests/golden/temporal_cornell_128.npz: the converged image of the orbited view that tests/test_temporal_host.py measures
the temporal blend against.  The twin of denoise_cornell_128.npz, which is the same render at the unmoved camera.

The CPU oracle (oracle/oracle_pt.cpp) renders cornell_box.obj at 128 x 128, maxDepth 8, direct lighting and importance sampling
on, 32 progressive frames of 256 samples per pixel (8192 in all), at the camera of acgpt_main --orbit 20,0 (10 degrees about the
look-at point; temporal_ref.orbit_camera).  About two minutes on eight cores.  Deterministic.

    python tests/golden/make_temporal_golden.py
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
import oracle_lib  # noqa: E402
import temporal_ref as tr  # noqa: E402
from scene_utils import copy_params, make_params  # noqa: E402

SIZE, DEPTH, FRAMES, SPP = 128, 8, 32, 256
ORBIT = (20, 0)


def main():
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj"))
    orc = oracle_lib.load()
    sc = orc.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    cam = tr.orbit_camera(SIZE, SIZE, *ORBIT)
    acc = None
    for f in range(FRAMES):
        p = tr.set_camera(make_params(SIZE, SIZE, SPP, DEPTH, True, True, frame=f), *cam)
        acc, _, _, _ = sc.render(copy_params(p), accumulation=acc)
    out = os.path.join(HERE, "temporal_cornell_128.npz")
    np.savez_compressed(out, ref=np.ascontiguousarray(acc[..., :3], np.float32),
                        meta=np.array([SIZE, SIZE, DEPTH, FRAMES, SPP, ORBIT[0], ORBIT[1]], np.int32))
    print("wrote", out)


if __name__ == "__main__":
    main()
