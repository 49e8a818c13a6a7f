"""The scenes on which the builders are held to tests/build_ref.py, and the reference results per scene, computed once per process
(tests/test_build_ref_host.py and tests/test_gpu_build_ref.py share them).  Scenes are (verts [n, 4] f32, idx [t, 3] u32, mat_ids, materials)."""
import functools

import numpy as np

import build_ref as br
import query_scenes as qs
from test_gpu_tree import _soup

F = np.float32
SOUPS = (2, 3, 17, 18, 255, 256, 257, 1025, 2049)
MODE1 = tuple("soup%d" % n for n in SOUPS) + ("box", "sphere", "strip", "copies")        # PLOC alone
HOST_PASS = ("box", "soup255", "soup257", "soup2049")                                       # mode 2 up to kOptimizeMaxTris triangles
REINSERTED = ("soup16385", "copies", "sphere")                                              # mode 2 above it: the device's reinsertion
HOST_ONLY = ("same",)                                                                       # CPU tests only


@functools.lru_cache(maxsize=None)
def strip(quads=1500):
    """tools/degenerate_scenes.py `strip`: identical unit quads at integer spacing, two triangles each; every merged area ties with its
    mirror image"""
    i = np.arange(quads + 1)
    v = np.zeros((2 * (quads + 1), 4), F)
    v[0::2, 0], v[1::2, 0], v[1::2, 1] = i, i, 1.0
    a = 2 * np.arange(quads)
    idx = np.stack([np.stack([a, a + 2, a + 3], axis=1), np.stack([a, a + 3, a + 1], axis=1)], axis=1).reshape(-1, 3)
    return qs._frozen(v, idx, np.zeros(len(idx), np.uint32), qs.box()[3])


@functools.lru_cache(maxsize=None)
def same(n=1500):
    """n copies of one triangle over three shared vertices"""
    v = np.array([[100, 100, 100, 0], [300, 100, 100, 0], [100, 300, 100, 0]], F)
    return qs._frozen(v, np.tile(np.arange(3, dtype=np.uint32), (n, 1)), np.zeros(n, np.uint32), qs.box()[3])


def scene(name):
    if name.startswith("soup"):
        return _soup(int(name[4:]))
    return {"box": qs.box, "sphere": qs.sphere, "copies": qs.copies, "strip": strip, "same": same}[name]()


@functools.lru_cache(maxsize=None)
def leaves(name):
    """(lo, hi, prims) of the scene's triangles in this module's Morton order"""
    v, idx = scene(name)[:2]
    prims = br.morton_order(v, idx)[1]
    return br.leaf_boxes(v, idx, prims) + (prims,)


@functools.lru_cache(maxsize=None)
def ploc(name, alter=None):
    lo, hi, _ = leaves(name)
    return br.ploc(lo, hi, alter)


@functools.lru_cache(maxsize=None)
def host_pass(name, max_passes=8, alter=None):
    return br.insertion_pass(ploc(name)[0], max_passes, alter=alter)


@functools.lru_cache(maxsize=None)
def reinserted(name, alter=None, rounds=br.K_REINSERT_ITERATIONS):
    return br.reinsert(ploc(name)[0], rounds, alter)
