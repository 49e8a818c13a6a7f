"""tests/golden/cast_walk.npz without a GPU: its inputs regenerate from cast_walk_cases' seeds, the CPU references (sweep_ref,
capsule_ref, boxcast_ref, tricast_ref: the statements of include/acgpt.h) reproduce every recorded record and byte, so the file is
tied to the statement and not only to the commit it was recorded from, cast 0 is the exact tie it is there for, and the recorded visit
counts are counts of a pruned walk.  Also that the four units include csrc/cast_walk.h."""
import os
import re

import numpy as np
import pytest

from acgpathtracing_amd import _build
import cast_walk_cases as cw


@pytest.fixture(scope="module")
def golden():
    with np.load(cw.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_file_is_small_and_names_its_commit(golden):
    assert os.path.getsize(cw.GOLDEN) < 256 * 1024
    assert re.fullmatch(r"[0-9a-f]{7,40}", str(golden["recorded_from"]))
    head = open(os.path.join(cw.HERE, "golden", "make_cast_walk_golden.py")).read().split('"""')[1]
    assert str(golden["recorded_from"])[:7] in head
    want = set()
    for key in cw.all_keys():
        part = key.split("/")
        want.add("poses_cast/records" if part[0] == "poses_cast" else "%s/%s/records" % (part[0], part[1]) if part[-1] == "records" else key)
    assert set(golden) == want | {"recorded_from"}


def test_the_inputs_regenerate_from_the_seed():
    for family, f in cw.FAMILIES.items():
        for scene in cw.SCENES:
            a, b = cw.casts_of(family, scene), cw.casts_of(family, scene)
            assert a.shape == (cw.N, f.floats) and a.dtype == np.float32
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (family, scene)
            bad = ~f.ref.castable(a)
            assert bad.sum() == len(f.ref.bad_cases()) and not bad[0], (family, scene)           # every miss before any traversal
            assert bad[:256].any() and bad[256:320].any(), (family, scene)                       # in both workgroups
    assert cw.N == 256 + 64 + 1
    mesh, poses, motions = cw.pose_inputs()
    assert mesh.shape == (12, 12) and poses.shape == (5, 12) and motions.shape == (5, 4)


@pytest.mark.parametrize("scene", list(cw.SCENES))
@pytest.mark.parametrize("family", list(cw.FAMILIES))
def test_the_references_reproduce_the_recorded_records(golden, family, scene):
    f = cw.FAMILIES[family]
    rec = golden["%s/%s/records" % (family, scene)]
    ref = cw.reference(family, scene)
    bad = np.flatnonzero((rec != ref).any(axis=1))
    assert bad.size == 0, (bad[:8], rec[bad[:2]], ref[bad[:2]])
    hit = ref[:, 1] != 0xFFFFFFFF
    assert 0.25 <= hit.mean() <= 0.95                                        # hits and misses both
    casts = cw.casts_of(family, scene)
    assert np.array_equal(ref[~f.ref.castable(casts)], f.ref.miss_records(int((~f.ref.castable(casts)).sum())))
    for fmt in cw.FORMATS:
        assert np.array_equal(golden["%s/%s/%s/any" % (family, scene, fmt)], f.ref.blocked_of(ref)), fmt
    # cast 0: t = 0 on the lower of two triangles that both give it
    v, idx, ids = cw.SCENES[scene][0]()[:3]
    i, j, _ = cw.tied_pair(v, idx)
    assert ref[0, 0] == 0 and ref[0, 1] == i
    if j is not None:
        without = f.records(casts[:1], v, np.delete(idx, i, axis=0).reshape(-1), np.delete(ids, i))
        assert without[0, 0] == 0 and without[0, 1] == j - 1                 # the other one of the pair, one index down


def test_the_reference_reproduces_the_recorded_poses(golden):
    rec = golden["poses_cast/records"]
    assert np.array_equal(rec, cw.pose_reference())
    t = rec[:, 0].view(np.float32)
    assert t[1] == 0 and (t[[0, 2, 4]] > 0).all() and rec[3, 1] == 0xFFFFFFFF and rec[3, 3] == 0xFFFFFFFF      # a start in contact, hits, a tmax that ends short


def test_the_counts_are_counts_of_a_walk(golden):
    """What makes the comparison of the counts worth having: the boxes prune, the deep scene is walked, and the extra admission tests
    (mode 0 of the capsule's and the box's hook) never add a visit"""
    seen = 0
    for key, a in golden.items():
        part = key.split("/")
        if part[-1] != "counts":
            continue
        seen += 1
        n_tris = len(cw.SCENES[part[1]][0]()[1])
        assert a.shape == (cw.N, 2) and a.any(), key
        assert (a[:, 1] <= n_tris).all() and (a[:, 0] <= max(n_tris - 1, 1)).all(), key
        casts = cw.casts_of(part[0], part[1])
        assert not a[~cw.FAMILIES[part[0]].ref.castable(casts)].any(), key       # a miss before any traversal visits nothing
        if part[3] == "visits1":
            with_test = golden["/".join(part[:3] + ["visits0", "counts"])]
            assert (with_test <= a).all(), key
    assert seen == len(cw.SCENES) * len(cw.FORMATS) * sum(len(f.modes) for f in cw.FAMILIES.values())


CSRC = _build.CSRC


def _sources():
    return [n for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".h", ".inc"))]


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_units_include_the_shared_walk():
    """tests/test_capsule_host.py::test_build_lists_and_abi holds the slab, the decode and the tie rule to cast_walk.h alone; here: the
    four units include it, the scene's scale has one accessor, and the render kernels' hash has not moved"""
    assert "cast_walk.h" in _build.HIP_HEADERS and "cast_walk.h" not in _build.KERNEL_SOURCES
    for unit in ("sweep.hip", "capsule.hip", "boxcast.hip", "tricast_device.h"):
        assert '#include "cast_walk.h"' in _src(unit), unit
    assert sum(len(re.findall(r"_scene_scale\(const float scene_lo", _src(n))) for n in _sources()) <= 1
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
