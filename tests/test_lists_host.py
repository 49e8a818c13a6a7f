"""The complete lists in CSR form without a GPU: tests/lists_ref.py against the capped lists of overlap_ref / tritri_ref, the ladder's
properties, the list-length classes of the existing box and triangle sets on both Cornell fixtures (held as recorded), the argument
checks of queryOverlapLists, queryTrianglesLists and meshCollisions(pairs="all") that need no device, the build lists, the header and
the bindings, and the scratch and spill figures of the built kernels."""
import os
import re
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import lists_ref as lr
import overlap_ref as ov
import tritri_ref as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = ((278.0, 273.0, -900.0), (-616.7, 0.0, 0.0), (0.0, 387.8, 0.0), (0.0, 0.0, 1230.0))         # close to the default view at 97 x 61
LADDER_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 20000)

# Queries per class of list length (0, 1-8, 9-64, 65-256, above 256) of every 1 000-query set, by the brute force; the same on both
# Cornell fixtures, which share their geometry.  With them: the longest list and the sum of the counts.
BOX_CLASSES = {"random": ((675, 297, 22, 5, 1), 388, 2100), "grid": ((663, 316, 20, 1, 0), 75, 944), "centroids": ((0, 967, 32, 1, 0), 97, 2116),
               "first_hits": ((527, 472, 1, 0, 0), 10, 524), "wall_faces": ((171, 519, 260, 47, 3), 855, 14124), "far": ((547, 451, 2, 0, 0), 10, 911),
               "whole": ((0, 0, 0, 0, 1000), 1264, 1264000), "outside": ((1000, 0, 0, 0, 0), 0, 0)}
TRI_CLASSES = {"random": ((694, 280, 24, 2, 0), 80, 1237), "self": ((0, 25, 975, 0, 0), 29, 13230), "edge": ((0, 58, 942, 0, 0), 39, 10973),
               "coplanar": ((287, 682, 31, 0, 0), 27, 2651), "wall_touch": ((204, 735, 53, 8, 0), 93, 3327), "whole": ((0, 192, 614, 194, 0), 158, 36052),
               "degenerate": ((574, 426, 0, 0, 0), 4, 439), "far": ((601, 399, 0, 0, 0), 1, 399), "outside": ((1000, 0, 0, 0, 0), 0, 0)}


@pytest.fixture(scope="module")
def cornell():
    """scene file -> ({box set: matrix}, {triangle set: matrix}): the brute force, computed once, shared, never written"""
    out = {}
    for scene in ("cornell_box.obj", "cornell_box_diffuse.obj"):
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
        verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
        boxes = {name: ov.overlap_matrix(ov.box_set(name, verts, idx, camera=CAM), verts, idx) for name in ov.BOX_SETS}
        tris = {name: tt.intersect_matrix(tt.query_set(name, verts, idx, camera=CAM), verts, idx) for name in tt.QUERY_SETS}
        for m in list(boxes.values()) + list(tris.values()):
            m.setflags(write=False)
        out[scene] = (boxes, tris)
    return out


def test_offsets_of():
    assert lr.offsets_of([]).tolist() == [0] and lr.offsets_of([]).dtype == np.uint64
    assert lr.offsets_of(np.array([3, 0, 0, 5], np.uint32)).tolist() == [0, 3, 3, 3, 8]
    big = lr.offsets_of(np.full(3, 0xFFFFFFFF, np.uint32))
    assert big.tolist() == [0, 0xFFFFFFFF, 2 * 0xFFFFFFFF, 3 * 0xFFFFFFFF]          # the sums do not wrap at 32 bits


def test_csr_against_the_capped_lists(cornell):
    """At K = 8 the first min(count, 8) entries of every slice are the capped reference's list, and the counts are its counts"""
    for scene, (boxes, tris) in cornell.items():
        for name, m in list(boxes.items()) + list(tris.items()):
            offsets, prims, counts = lr.csr_of_matrix(m)
            c8, p8, _ = ov.lists_of_matrix(m, 8)
            assert np.array_equal(counts, c8) and offsets[-1] == prims.size == int(c8.sum(dtype=np.uint64)), (scene, name)
            assert np.array_equal(offsets, lr.offsets_of(c8))
            for i in range(m.shape[0]):
                s = prims[int(offsets[i]):int(offsets[i + 1])]
                k = min(int(counts[i]), 8)
                assert np.array_equal(s[:k], p8[i, :k]) and (p8[i, k:] == 0xFFFFFFFF).all(), (scene, name, i)
                assert (np.diff(s.astype(np.int64)) > 0).all()


def test_length_classes_of_the_existing_sets(cornell):
    """The sets' coverage of the list-length classes as a checked fact, with the figures held as recorded"""
    for scene, (boxes, tris) in cornell.items():
        union_b, union_t = np.zeros(5, np.int64), np.zeros(5, np.int64)
        for name, m in boxes.items():
            counts = m.sum(axis=1)
            assert (lr.class_shares(counts), int(counts.max()), int(counts.sum())) == BOX_CLASSES[name], (scene, name, lr.class_shares(counts), counts.max(), counts.sum())
            union_b += lr.class_shares(counts)
        for name, m in tris.items():
            counts = m.sum(axis=1)
            assert (lr.class_shares(counts), int(counts.max()), int(counts.sum())) == TRI_CLASSES[name], (scene, name, lr.class_shares(counts), counts.max(), counts.sum())
            union_t += lr.class_shares(counts)
        assert (union_b > 0).all(), (scene, union_b)                 # 0, 1-8, 9-64, 65-256 and above 256
        assert (union_t[:4] > 0).all(), (scene, union_t)             # up to 65-256
    # the hole the capped calls leave is the common case of a collision pass
    assert TRI_CLASSES["self"][0][2] / 1000.0 > 0.9 and BOX_CLASSES["whole"][0][4] == 1000


def test_ladder():
    v, idx = lr.ladder()
    T = lr.LADDER_T
    assert v.shape == (3 * T, 4) and idx.shape == (T, 3) and v.dtype == np.float32 and idx.dtype == np.uint32
    perm = lr.ladder_perm()
    assert np.array_equal(np.sort(perm), np.arange(T))
    # the triangle at position p has index perm[p]
    x = v.reshape(T, 3, 4)[:, 2, 0]
    assert np.array_equal(x[perm], np.arange(T, dtype=np.float32))
    # a sort that does nothing would not pass: for every k >= 2 used the list in position order is not ascending
    for k in LADDER_LENGTHS:
        if k >= 2:
            assert (np.diff(perm[:k].astype(np.int64)) < 0).any(), k
    # the brute force decides the lengths, and they are the ones asked for; the lists are the construction's
    want = lr.ladder_expected(LADDER_LENGTHS)
    for m in (ov.overlap_matrix(lr.ladder_boxes(LADDER_LENGTHS), v, idx.reshape(-1)), tt.intersect_matrix(lr.ladder_triangles(LADDER_LENGTHS), v, idx.reshape(-1))):
        got = lr.csr_of_matrix(m)
        assert got[2].tolist() == list(LADDER_LENGTHS)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    assert ov.searchable(lr.ladder_boxes(LADDER_LENGTHS)).all() and tt.searchable(lr.ladder_triangles(LADDER_LENGTHS)).all()


def test_build_lists_header_and_bindings():
    assert "lists.hip" in _build.HIP_SOURCES and {"lists.h", "overlap_device.h", "tritri_device.h", "bvh_walk.h", "query_launch.h"} <= set(_build.HIP_HEADERS)
    for name in ("lists.hip", "lists.h", "overlap_device.h", "tritri_device.h", "bvh_walk.h", "query_launch.h", "overlap.hip", "tritri.hip", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    assert _native.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for name, proto in (("pt_list_offsets", "int pt_list_offsets(pt_ctx* ctx, const uint32_t* counts, size_t n, uint32_t* offsets, uint64_t* total);"),
                        ("pt_query_overlap_lists", "int pt_query_overlap_lists(pt_ctx* ctx, const float* boxes, size_t n, const uint32_t* offsets, uint32_t* prims, size_t capacity, uint32_t* found);"),
                        ("pt_query_triangles_lists", "int pt_query_triangles_lists(pt_ctx* ctx, const float* tris, size_t n, const uint32_t* offsets, uint32_t* prims, size_t capacity, uint32_t* found);")):
        assert name in _native.ABI_SYMBOLS and proto in flat, name
    # the cuts the GPU test reads from the bindings are the kernels'
    src = open(os.path.join(_build.CSRC, "lists.h")).read()
    for c_name, value in (("kListRegister", _native.LIST_REGISTER), ("kListSortLds", _native.LIST_SORT_LDS), ("kListScanTile", _native.LIST_SCAN_TILE),
                          ("kListScanRuns", _native.LIST_SCAN_RUNS)):
        assert re.search(r"constexpr uint32_t %s = %du;" % (c_name, value), src), c_name
    assert _native.LIST_REGISTER == ov.MAX_PRIMS == tt.MAX_PRIMS


def test_list_kernels_use_no_scratch_memory_and_spill_nothing(built):
    """The three scan kernels, the eight fills (two node formats, boxes and triangles, with the register list and, for the timing tool,
    without) and the sort: no private segment, no spilled vector or scalar register"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if re.search(r"\bk_(list_|fill_lists|sort_lists)", k["name"])]
    assert len(rows) == 12, [k["name"] for k in rows]
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


def test_wrappers_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the device is touched
    for bad in (np.zeros((4, 7), np.float32), np.zeros(8, np.float32), np.zeros((4, 3), np.float32)):
        with pytest.raises(pt.PathTracerError, match="expected|need half_extents"):
            pt.queryOverlapLists(state, bad)
    with pytest.raises(pt.PathTracerError, match="half_extents must be None"):
        pt.queryOverlapLists(state, np.zeros((4, 8), np.float32), half_extents=1.0)
    with pytest.raises(pt.PathTracerError, match="non-negative"):
        pt.queryOverlapLists(state, np.zeros((4, 3), np.float32), half_extents=-1.0)
    for bad in (np.zeros((4, 8), np.float32), np.zeros(12, np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(pt.PathTracerError, match="expected"):
            pt.queryTrianglesLists(state, bad)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.queryTrianglesLists(state, np.zeros((2, 9), np.complex64))
    # no queries: nothing to do, and the library is never asked
    for got in (pt.queryOverlapLists(state, np.zeros((0, 8), np.float32)), pt.queryOverlapLists(state, np.zeros((0, 3)), half_extents=1.0),
                pt.queryTrianglesLists(state, np.zeros((0, 3, 3), np.float32))):
        assert sorted(got) == ["count", "offsets", "prim"]
        assert got["offsets"].tolist() == [0] and got["prim"].shape == (0,) and got["count"].shape == (0,)
        assert all(a.dtype == np.uint32 for a in got.values())
    verts = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], np.float64)
    for bad in ("some", "ALL", ""):
        with pytest.raises(pt.PathTracerError, match="pairs is False, True or"):
            pt.meshCollisions(state, verts, [[0, 1, 2]], pairs=bad)
    got = pt.meshCollisions(state, verts, np.zeros((0, 3), np.int32), pairs="all")
    assert got["pairs"].shape == (0, 3) and got["counts"].shape == (1, 0)
    torch = pytest.importorskip("torch")
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.queryOverlapLists(state, torch.zeros((4, 8), dtype=torch.float32))
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.queryTrianglesLists(state, torch.zeros((4, 12), dtype=torch.float32))
