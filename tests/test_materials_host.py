"""pt_update_materials without a GPU: the export, its declaration and binding, the refusal of a null context, pathtracer.updateMaterials'
argument checks (they refuse bad shapes and dtypes before the library is called), TemporalHistory's drop rule, and acgpt_main's
--set-material parser, which refuses a malformed spec before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = os.path.join(pt.SCENES, "cornell_box.obj")


@pytest.fixture(scope="module")
def lib():
    _build.build_hip()
    return _native.hip()


def test_exported_declared_and_bound(lib):
    assert hasattr(lib, "pt_update_materials")
    assert "pt_update_materials" in _native.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    assert re.search(r"int\s+pt_update_materials\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const pt_material\s*\*\s*mats,\s*size_t n_mats,"
                     r"\s*const uint32_t\s*\*\s*mat_ids,\s*size_t n_tris,\s*pt_update_info\s*\*\s*info\s*\)", header)
    f = lib.pt_update_materials
    assert f.restype is C.c_int and len(f.argtypes) == 6 and f.argtypes[-1] is C.POINTER(_native.UpdateInfo)
    assert lib.pt_abi_version() == 4


def test_refused_without_a_context(lib):
    m = (_native.Material * 1)()
    assert lib.pt_update_materials(None, C.addressof(m), 1, None, 0, None) != 0
    msg = lib.pt_last_error(None)
    assert b"pt_update_materials" in msg and b"null context" in msg


class _Poison:
    """Stands in for the library: any call is an error."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def _mats(n=3):
    return [_native.Material() for _ in range(n)]


@pytest.mark.parametrize("ids", [np.zeros((4, 2), np.uint32), np.zeros((2, 2, 2), np.int32), np.zeros(4, np.float32),
                                 np.zeros(4, np.bool_), np.array([0, -1, 2], np.int64), np.array([1 << 33], np.int64),
                                 np.array(["a", "b"])])
def test_bad_ids_are_refused_before_the_library(monkeypatch, ids):
    monkeypatch.setattr(_native, "hip", lambda: _Poison())
    state = pt.PathTracerState()
    with pytest.raises(ValueError):
        pt.updateMaterials(state, _mats(), ids)


def test_bad_tables_and_device_tensors_are_refused(monkeypatch):
    monkeypatch.setattr(_native, "hip", lambda: _Poison())
    state = pt.PathTracerState()
    for bad in ([1, 2, 3], [_native.Float3()], (_native.AreaLight * 2)(), "white"):
        with pytest.raises(ValueError):
            pt.updateMaterials(state, bad)
    with pytest.raises(ValueError):
        pt.updateMaterials(state)                               # nothing to change
    with pytest.raises(ValueError):
        pt.updateMaterials(state, material_ids=np.zeros(3, np.uint32))      # no scene: no table to keep

    class _DeviceTensor:
        class device:
            type = "cuda"

        def detach(self):
            return self

    with pytest.raises(ValueError):
        pt.updateMaterials(state, _mats(), _DeviceTensor())


def test_accepts_lists_arrays_and_cpu_tensors(monkeypatch):
    import torch
    seen = []

    class _Lib:
        def pt_update_materials(self, ctx, mats, n_mats, ids, n_tris, info):
            got = None if ids is None else np.ctypeslib.as_array(C.cast(ids, C.POINTER(C.c_uint32)), (n_tris,)).copy()
            seen.append((n_mats, got))
            return 0

        def pt_scene_handle(self, ctx):
            return 9

    monkeypatch.setattr(_native, "hip", lambda: _Lib())
    state = pt.PathTracerState()
    out = pt.updateMaterials(state, _mats(4), np.array([3, 0, 1], np.int64))
    assert out == {"ms": 0.0, "area_ratio": 0.0, "rebuilt": False} and state.params.handle == 9 and state._mats_serial == 1
    pt.updateMaterials(state, material_ids=torch.tensor([2, 2, 1], dtype=torch.int32))      # the table just given is kept
    table = (_native.Material * 2)()
    pt.updateMaterials(state, table)
    assert state._materials is table and state._mats_serial == 3
    assert [n for n, _ in seen] == [4, 4, 2]
    assert seen[0][1].tolist() == [3, 0, 1] and seen[1][1].tolist() == [2, 2, 1] and seen[2][1] is None


def test_temporal_history_drops_on_a_material_edit(monkeypatch):
    class _Lib:
        def pt_scene_handle(self, ctx):
            return 5

    monkeypatch.setattr(_native, "hip", lambda: _Lib())
    state = pt.PathTracerState()
    for motion in (False, True):
        h = pt.TemporalHistory(motion=motion)
        before = h._settings_of(state)
        assert h._settings_of(state) == before
        state._mats_serial += 1
        assert h._settings_of(state) != before


@pytest.mark.parametrize("spec", ["no_such_material:kd=1,1,1", "white", "white:", ":kd=1,1,1", "white:kd=1,1", "white:kd=1,1,1,ke",
                                  "white:kd=1,x,1", "white:ke=1,1,1,1", "white:bsdf=plastic", "white:ior=", "white:ior=nan",
                                  "white:kd=inf,1,1", "white:rough=0.5", "white:kd=1,1,1,kd=0,0,0", "white:kd=1,1,1;"])
def test_cli_rejects_malformed_specs(lib, tmp_path, spec):
    exe = _build.build_main()
    r = subprocess.run([exe, "--obj", BOX, "--width", "8", "--height", "8", "--frames", "1", "--out", str(tmp_path / "a.png"),
                        "--set-material", "red:kd=0.5,0.5,0.5", "--set-material", spec], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--set-material:" in r.stderr
    assert "Using Direct Lighting" not in r.stdout            # refused before the device is touched
    assert not (tmp_path / "a.png").exists()
