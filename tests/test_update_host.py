"""pt_update_vertices without a GPU: the export and its declaration, the struct layout, and pathtracer.updateVertices' argument checks,
which refuse a wrongly shaped array before the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _build.build_hip()
    return _native.hip()


def test_exported_and_declared(lib):
    assert hasattr(lib, "pt_update_vertices")
    assert "pt_update_vertices" in _native.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert re.search(r"int\s+pt_update_vertices\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const float\s*\*\s*verts_xyzw,\s*size_t n_verts,\s*int mode,"
                     r"\s*pt_update_info\s*\*\s*info\s*\)", header)
    for name, value in (("PT_UPDATE_REFIT", 0), ("PT_UPDATE_REBUILD", 1), ("PT_UPDATE_AUTO", 2)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), header)
    m = re.search(r"#define PT_UPDATE_AUTO_AREA_RATIO\s+([0-9.]+)f", header)
    assert m and float(m.group(1)) == _native.UPDATE_AUTO_AREA_RATIO
    assert C.sizeof(_native.UpdateInfo) == 16 and [f for f, _ in _native.UpdateInfo._fields_] == ["ms", "area_ratio", "rebuilt", "reserved"]
    assert lib.pt_abi_version() == 4


def test_refused_without_a_context(lib):
    v = np.zeros((3, 4), np.float32)
    assert lib.pt_update_vertices(None, v.ctypes.data, 3, 0, None) != 0
    assert b"null context" in lib.pt_last_error(None)


class _Poison:
    """Stands in for the library: any call is an error."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


@pytest.mark.parametrize("bad", [np.zeros((5, 3), np.float32), np.zeros((2, 4, 4), np.float32), np.zeros(10, np.float32),
                                 np.zeros((0, 4), np.float32)])
def test_wrong_shapes_are_refused_before_the_library(monkeypatch, bad):
    monkeypatch.setattr(_native, "hip", lambda: _Poison())
    state = pt.PathTracerState()
    with pytest.raises(ValueError):
        pt.updateVertices(state, bad)


def test_unknown_mode_and_device_tensor_are_refused(monkeypatch):
    monkeypatch.setattr(_native, "hip", lambda: _Poison())
    state = pt.PathTracerState()
    with pytest.raises(ValueError):
        pt.updateVertices(state, np.zeros((4, 4), np.float32), mode="optimise")

    class _DeviceTensor:
        class device:
            type = "cuda"

        def detach(self):
            return self

    with pytest.raises(ValueError):
        pt.updateVertices(state, _DeviceTensor())


def test_accepts_flat_arrays_and_cpu_tensors(monkeypatch):
    import torch
    seen = []

    class _Lib:
        def pt_update_vertices(self, ctx, ptr, n, mode, info):
            seen.append((n, mode))
            return 0

        def pt_scene_handle(self, ctx):
            return 7

    monkeypatch.setattr(_native, "hip", lambda: _Lib())
    state = pt.PathTracerState()
    v = np.arange(24, dtype=np.float64).reshape(6, 4)
    assert pt.updateVertices(state, v.reshape(-1))["rebuilt"] is False
    pt.updateVertices(state, torch.from_numpy(v.astype(np.float32)), mode="auto")
    pt.updateVertices(state, v, mode="rebuild")
    assert seen == [(6, 0), (6, 2), (6, 1)] and state.params.handle == 7
