"""The host side of the small-scene render path (csrc/render_small.hip), without a GPU: the 16-bit node references of csrc/small_ref.h
round-trip every reference a Cornell tree can hold and the limit cases; the LDS budget's arithmetic; the new sources stay outside the
hashed kernel sources."""
import ctypes as C
import os

import numpy as np

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native

SENTINEL = 0x7FFFFFFF
MAX_NODES, MAX_TRIS = 2048, 32768
CU_LDS = 160 * 1024


def _codec(refs):
    L = _native.hip()
    refs = np.ascontiguousarray(refs, np.int32)
    enc, dec, loc = np.zeros(len(refs), np.uint16), np.zeros(len(refs), np.int32), np.zeros(len(refs), np.int32)
    assert L.pt_debug_small_ref(refs.ctypes.data, len(refs), enc.ctypes.data, dec.ctypes.data, loc.ctypes.data) == 0
    return enc, dec, loc


def _tree_refs(n_tris):
    """every reference a two-child tree over n_tris triangles holds: n_tris - 1 inner nodes as byte offsets of 32-byte nodes, ~slot per triangle"""
    return np.concatenate([np.arange(n_tris - 1, dtype=np.int64) * 32, ~np.arange(n_tris, dtype=np.int64), [SENTINEL]]).astype(np.int32)


def test_references_round_trip_on_the_cornell_trees():
    for name in ("cornell_box_diffuse.obj", "cornell_box.obj"):
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, name))
        n_tris = obj.getIndexBuffer().size // 3
        assert 2 <= n_tris <= MAX_NODES
        refs = _tree_refs(n_tris)
        enc, dec, loc = _codec(refs)
        assert np.array_equal(dec, refs)
        assert len(np.unique(enc)) == len(refs)                              # no two references share an entry
        assert np.array_equal(loc, enc.view(np.int16).astype(np.int32))      # the kernel's form is the entry, sign-extended
        inner = refs[: n_tris - 1]
        assert np.array_equal(loc[: n_tris - 1] << 1, inner)                  # an inner node's LDS address
        assert np.array_equal(~loc[n_tris - 1:-1], np.arange(n_tris))        # a triangle's slot
        assert loc[-1] == 0x7FFF and enc[-1] == 0x7FFF


def test_references_round_trip_at_the_limits():
    out = np.zeros(5, np.uint64)
    assert _native.hip().pt_debug_small_budget(1, 2, 8, CU_LDS, out.ctypes.data) == 0
    assert (int(out[3]), int(out[4])) == (MAX_NODES, MAX_TRIS)
    refs = np.concatenate([np.arange(MAX_NODES, dtype=np.int64) * 32, ~np.arange(MAX_TRIS, dtype=np.int64), [SENTINEL]]).astype(np.int32)
    enc, dec, loc = _codec(refs)
    assert np.array_equal(dec, refs) and len(np.unique(enc)) == len(refs)
    assert loc[MAX_NODES - 1] == 32752 and loc[MAX_NODES] == -1 and loc[-2] == -32768 and loc[-1] == 0x7FFF
    # inner nodes and the sentinel are what `(uint32_t)node < (uint32_t)sentinel` and `node < 0` tell apart
    assert (loc[:MAX_NODES] >= 0).all() and (loc[:MAX_NODES] < 0x7FFF).all() and (loc[MAX_NODES:-1] < 0).all()
    # one past either limit no longer fits
    _, dec, _ = _codec([MAX_NODES * 32, ~MAX_TRIS])
    assert dec[0] != MAX_NODES * 32 and dec[1] != ~MAX_TRIS


def _budget(n, s):
    big = 16 * s * 128 + n * 32 + 256 + 16 * 320
    little = 4 * s * 128 + n * 32 + 256 + 4 * 320
    return big, little


def test_lds_budget():
    L = _native.hip()
    out = np.zeros(5, np.uint64)

    def ask(n, t, s, lds=CU_LDS):
        assert L.pt_debug_small_budget(n, t, s, lds, out.ctypes.data) == 0
        return int(out[0]), int(out[1]), bool(out[2])

    # the Cornell class: 1263 nodes, 24 entries — 2 x nodes + 20 waves x 64 lanes x 24 x 2 B + 20 books + 2 LCG tables
    big, little, ok = ask(1263, 1264, 24)
    assert (big, little) == _budget(1263, 24) and big + little == 2 * 1263 * 32 + 20 * 64 * 24 * 2 + 20 * 320 + 2 * 256
    assert ok and big + little <= CU_LDS < big + 2 * little
    # both sides of the LDS limit at 24 entries, of the "a second 256-thread workgroup must not fit" rule, and of the reference limits
    kb = lambda b: (b + 1023) // 1024 * 1024
    fits = [n for n in range(1, MAX_NODES + 1) if kb(_budget(n, 24)[0]) + kb(_budget(n, 24)[1]) <= CU_LDS and sum(_budget(n, 24)) + _budget(n, 24)[1] > CU_LDS]
    lo, hi = fits[0], fits[-1]
    assert fits == list(range(lo, hi + 1)) and 1 < lo < 1263 < hi < MAX_NODES
    for n, want in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
        assert ask(n, n + 1, 24)[2] is want, n
    assert not ask(1263, 1264, 24, 64 * 1024)[2]           # a CU with 64 KB of LDS never takes the path
    assert not ask(1263, 1264, 26)[2]                      # entries come in fours
    assert not ask(1263, MAX_TRIS + 1, 24)[2] and ask(1263, MAX_TRIS, 24)[2]
    assert not ask(MAX_NODES + 1, 1264, 8, 1 << 20)[2] and not ask(0, 1, 8)[2]


def test_new_sources_stay_outside_the_kernel_hash():
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    new = {"render_small.hip", "render_small.inc", "render_small.h", "small_ref.h"}
    assert not new & set(_build.KERNEL_SOURCES) and len(_build.KERNEL_SOURCES) == 10
    assert "render_small.hip" in _build.HIP_SOURCES and {"render_small.inc", "render_small.h", "small_ref.h"} <= set(_build.HIP_HEADERS)
    for s in ("pt_debug_small_kernel", "pt_debug_small_kernel_path", "pt_debug_small_ref", "pt_debug_small_budget"):
        assert s in _native.TEST_SYMBOLS
