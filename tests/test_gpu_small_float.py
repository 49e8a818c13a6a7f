"""The fp32 shape of the small-scene render path (csrc/render_small.hip): the 1024-thread workgroup stages the fp16 nodes as fp32 (64
bytes a node, four ds_read_b128 and twelve full-rate fmas a visit), the 256-thread workgroup holds no copy and reads the fp16 nodes
from global memory.  Every comparison is against variant 7 named through pt_set_tuning on the same context: accumulation bytes,
framebuffer bytes and the radiance / shadow / path / culled counters, with the path (pt_debug_small_kernel_path) and the shape
(pt_debug_small_shape) asserted — both grids and each alone, both math modes, glass and metal, trees of four stack sizes up to the
largest node array, an image on which both grids trace side by side, the fp16 fallback (by budget and by the hook), a refit; and the
staging function's output word for word."""
import ctypes as C

import numpy as np
import pytest

import small_kernel_cases as sk
from acgpathtracing_amd import _native
from scene_utils import make_params
from test_gpu_small_kernel import AUTO, BIG, BOTH, CU_LDS, DIFFUSE, FAST, FULL, IEEE, LITTLE, OLD, ONLY_BIG, ONLY_LITTLE, _budget, same
from test_gpu_small_kernel_cases import ALL_MODES, PATH_OF, STACK_SCENES, H, Scene, W, _loaded_image, _stack_scene, obj_scene, params

pytestmark = pytest.mark.gpu

NONE, HALF, FLOAT = 0, 1, 2                       # pt_debug_small_shape
# a room with a tail and 1300 coincident copies in build mode 0: N 1327 at S 28 — 163 520 bytes as two fp16 copies (eligible), and as
# fp32 147 648 + 15 872 = 163 520 that count as 145 + 16 KB: one of the 20 pairs that miss the CU's 160 KB by rounding
FALLBACK_TREE = (lambda: sk.tail(18, 1300), 0, lambda: sk.tail_camera(18, W, H))


def shape(c, force=-1):
    return c.L.pt_debug_small_shape(c.ctx, force)


def float_fits(c):
    b = c.info()
    out = np.zeros(4, np.uint64)
    assert c.L.pt_debug_small_float_budget(b.n_nodes, b.stack_entries, CU_LDS, out.ctypes.data) == 0
    return bool(out[3])


def check(c, p, modes, want=None, expect=FLOAT, **kw):
    """variant 7's answer on c (or `want`), and every mode's path, shape and answer held to it; returns variant 7's answer"""
    if want is None:
        want = c.render(p, "v7", **kw)
        assert shape(c) == NONE
    assert want[3] == OLD
    for mode in modes:
        got = c.render(p, mode, **kw)
        assert got[3] == PATH_OF[mode] and shape(c) == expect, (mode, got[3], shape(c))
        assert same(got, want), (mode, got[2], want[2], int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()))
    return want


@pytest.fixture(scope="module")
def boxes():
    """a context per Cornell scene and math mode, with variant 7's answer at 96 x 64, 16 spp, depth 8"""
    out = {}
    for scene in (DIFFUSE, FULL):
        for math in (IEEE, FAST):
            c = obj_scene(scene, math=math)
            out[scene, math] = (c, c.render(make_params(W, H, 16, 8, True, True), "v7"))
    yield out
    for c, _ in out.values():
        c.close()


@pytest.mark.parametrize("math", [IEEE, FAST], ids=["ieee", "fast"])
@pytest.mark.parametrize("mode", ALL_MODES, ids=["auto", "big", "little"])
@pytest.mark.parametrize("scene", [DIFFUSE, FULL], ids=["diffuse", "glass-metal"])
def test_matches_variant_7(boxes, scene, mode, math):
    c, want = boxes[scene, math]
    assert float_fits(c) and c.info().n_nodes == 1263 and c.info().stack_entries == 24
    check(c, make_params(W, H, 16, 8, True, True), (mode,), want=want)
    assert int(want[2][0]) > W * H * 16 and int(want[2][1]) > 0


@pytest.mark.parametrize("name", list(STACK_SCENES))
def test_stack_sizes_and_the_largest_node_array(name):
    """S 16 / 20 / 24 / 28; the lattice's 1567 nodes are the largest array of the cases: 100 288 bytes as fp32, node addresses beyond
    64 KB from 16-bit references"""
    c, cam = _stack_scene(name)
    try:
        b = c.info()
        print("%s: N %d, S %d" % (name, b.n_nodes, b.stack_entries))
        assert b.stack_entries == {"lattice": 16, "blob": 20, "box": 24, "tail": 28}[name]
        assert _budget(b.n_nodes, b.stack_entries) and float_fits(c)
        if name == "lattice":
            assert b.n_nodes == 1567 and b.n_nodes * 64 > 65536
        else:
            assert b.n_nodes < 1567
        for math in (FAST, IEEE):
            assert c.L.pt_set_math_mode(c.ctx, math) == 0
            want = check(c, params(cam, depth=8), ALL_MODES)
            assert int(want[2][0]) > int(want[2][3]) and int(want[2][3]) < W * H * 16 // 2       # most camera rays enter the tree
    finally:
        c.close()


def test_both_grids_side_by_side(boxes):
    """an image of 1280 n_cus x 64 items (the rule of test_grids_as_large_as_the_device): every wave of both grids comes back to the
    queue many times, so the LDS-fp32 and the global-fp16 workgroups trace at the same time on every CU"""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    spp = 16
    cs = sk.shifts(spp, 0, 1, pixels=1 << 21)[0]
    w, h = _loaded_image(n_cus, cs, 1, 2046)
    c, _ = boxes[DIFFUSE, FAST]
    p = params("reference", w=w, h=h, spp=spp)
    check(c, p, (AUTO,))
    st = _native.Stats()
    assert c.L.pt_get_stats(c.ctx, C.byref(st)) == 0 and st.grid_blocks == 2 * n_cus


def test_fallback_by_budget():
    """a tree the two-copy budget admits and the fp32 budget does not: the path is taken, in the fp16 shape, with variant 7's bytes"""
    c, cam = _stack_scene(FALLBACK_TREE)
    try:
        b = c.info()
        print("fallback tree: N %d, S %d" % (b.n_nodes, b.stack_entries))
        assert _budget(b.n_nodes, b.stack_entries) and not float_fits(c), (b.n_nodes, b.stack_entries)
        check(c, params(cam, depth=8), ALL_MODES, expect=HALF)
    finally:
        c.close()


@pytest.mark.parametrize("scene", [DIFFUSE, FULL], ids=["diffuse", "glass-metal"])
def test_fallback_by_the_hook(boxes, scene):
    c, want = boxes[scene, FAST]
    p = make_params(W, H, 16, 8, True, True)
    try:
        assert shape(c, 1) >= 0
        check(c, p, ALL_MODES, want=want, expect=HALF)
        assert shape(c, 0) == HALF
        check(c, p, (AUTO,), want=want, expect=FLOAT)
    finally:
        assert shape(c, 0) >= 0
    assert shape(c, 2) == -1 and shape(c, -2) == -1


def test_refit_reaches_both_grids():
    """pt_update_vertices (refit) of the short block: the 1024-thread grid restages the refitted nodes at its next launch and the
    256-thread grid reads the refitted array, each alone; the image differs from the one before the refit"""
    from test_gpu_small_kernel_cases import _box_arrays
    from test_gpu_update import _object_vertices
    v, idx, mats, ids = _box_arrays()
    moved = v.copy(); moved[_object_vertices(DIFFUSE, "short_block"), :3] += np.float32([-90.0, 60.0, 120.0])
    p = params("reference")
    c = Scene(v, idx, mats, ids)
    try:
        first = check(c, p, ALL_MODES)
        info = c.update(moved)
        assert info.rebuilt == 0
        after = check(c, p, (ONLY_BIG, ONLY_LITTLE, AUTO))
        assert not np.array_equal(after[0], first[0])
        fresh = Scene(moved, idx, mats, ids)
        try:
            assert same(fresh.render(p, "v7"), after)
        finally:
            fresh.close()
    finally:
        c.close()


@pytest.mark.parametrize("scene", [DIFFUSE, FULL], ids=["diffuse", "glass-metal"])
def test_staged_nodes_word_for_word(boxes, scene):
    """the staging function itself, over the device's own fp16 nodes: every float is the fp16 number, every child word the local form
    of small_ref.h, every pad word 0"""
    c, _ = boxes[scene, FAST]
    L = c.L
    info = _native.TreeInfo()
    assert L.pt_debug_read_tree(c.ctx, 0, None, 0, C.byref(info)) == 0
    n = info.n_nodes
    nodes = np.zeros((n * 2, 4), np.uint32)                       # a 16-byte half per child
    assert L.pt_debug_read_tree(c.ctx, 3, nodes.ctypes.data, nodes.nbytes, None) == 0, c.err()
    staged = np.full((n * 2, 2, 4), 0xDEADBEEF, np.uint32)        # two 16-byte records per half
    assert L.pt_debug_small_staged(c.ctx, staged.ctypes.data, staged.nbytes - 1) != 0      # a byte short: refused
    assert L.pt_debug_small_staged(c.ctx, staged.ctypes.data, staged.nbytes) == 0, c.err()
    centre = (nodes[:, :3] & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
    half = (nodes[:, :3] >> 16).astype(np.uint16).view(np.float16).astype(np.float32)
    assert np.array_equal(staged[:, 0, :3], centre.view(np.uint32)) and np.array_equal(staged[:, 1, :3], half.view(np.uint32))
    assert np.isfinite(centre).all() and np.isfinite(half).all() and len(np.unique(centre)) > 100
    refs = nodes[:, 3].view(np.int32).copy()
    enc, dec, loc = np.zeros(len(refs), np.uint16), np.zeros(len(refs), np.int32), np.zeros(len(refs), np.int32)
    assert L.pt_debug_small_ref(refs.ctypes.data, len(refs), enc.ctypes.data, dec.ctypes.data, loc.ctypes.data) == 0
    assert np.array_equal(staged[:, 0, 3].view(np.int32), loc)
    assert np.array_equal(loc, np.minimum(refs >> 1, refs))       # what the 256-thread workgroup computes from the wide word
    assert (loc[refs >= 0] << 2 == (refs[refs >= 0] // 32) * 64).all()      # an inner node's address in the fp32 array
    assert not staged[:, 1, 3].any()
