"""The fused box test of the small-scene render kernel (csrc/small_slab.h), without a GPU: the eight k_render_small instantiations
still fit five waves per SIMD with nothing spilled; the new header is a dependency of the build and stays outside the hashed kernel
sources."""
import os
import re
import sys

from acgpathtracing_amd import _build, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_small_kernels_keep_96_registers_and_spill_nothing(built):
    lib = _native.hip_library_path()
    if not os.path.exists(lib):
        _build.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(lib) if re.search(r"\bk_render_small<", k["name"])]
    # 1024 threads: nodes as fp16 or fp32 in LDS; 256 threads: fp16 in LDS or in global memory; each in both math modes
    assert len(rows) == 8, [k["name"] for k in rows]
    for k in rows:
        print(k["name"], k["vgpr_count"], k["vgpr_spill_count"], k["private_segment_fixed_size"])
        assert k["vgpr_count"] <= 96, k                     # five waves per SIMD
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k


def test_the_case_generator_keeps_its_hits():
    """the generator of tests/test_gpu_small_slab.py at a size the CPU does in a blink: records of ops 41 / 42 / 43, the shares its
    self-checks ask for, a scale per axis where the set's name says so"""
    import numpy as np
    import small_slab_cases as cases
    sets = cases.case_sets(1 << 14)
    assert list(sets) == ["one_scale", "squeezed", "flat"]
    for name, (rec, must, wide, least) in sets.items():
        assert rec.shape == (1 << 14, 19) and rec.dtype == np.float32 and rec.flags["C_CONTIGUOUS"]
        assert must.mean() > least and (~wide).mean() > 0.05, (name, must.mean(), wide.mean())
        assert not (must & ~wide).any()                     # the inflated box holds the unpadded one
    inv = {name: s[0][0, 15:18] for name, s in sets.items()}
    assert inv["one_scale"][0] == inv["one_scale"][1] == inv["one_scale"][2]
    assert inv["squeezed"][0] > 2.5 * inv["squeezed"][1] > 25 * inv["squeezed"][2] > 0
    assert inv["flat"][2] < 1e-4 * inv["flat"][0]


def test_the_header_is_a_dependency_outside_the_kernel_hash():
    assert "small_slab.h" in _build.HIP_HEADERS and "small_slab.h" not in _build.KERNEL_SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "small_slab.h"))
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b" and len(_build.KERNEL_SOURCES) == 10
    for user in ("render_small.hip", "selftest.hip"):
        assert '#include "small_slab.h"' in open(os.path.join(_build.CSRC, user)).read(), user
