"""The posed-mesh queries without a GPU: tests/poses_ref.py's transform against float64, its reductions against a per-pose loop that
asks the per-triangle references directly, the shares of hit and found poses of every (mesh, pose set) case the GPU tests run (held
as recorded), the ties of the symmetric set, the probe meshes' claim, the wrappers' argument checks, the build lists, the header and
the bindings, and the scratch and spill figures of the built kernels."""
import os
import re
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import poses_ref as pr
import tridist_ref as tr
import tritri_ref as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# (poses, poses that hit, poses that find something at +inf, poses that find something at the set's finite radius) per case, by the
# brute force on the Cornell box
RECORDED = {
    ('single', 'identity'): (1, 1, 1, 1),
    ('single', 'touching'): (4, 4, 4, 2),
    ('single', 'mixed'): (8, 3, 8, 4),
    ('box', 'identity'): (1, 1, 1, 1),
    ('box', 'free'): (8, 0, 8, 0),
    ('box', 'touching'): (4, 4, 4, 4),
    ('box', 'deep'): (6, 4, 6, 4),
    ('box', 'mixed'): (8, 3, 8, 5),
    ('box', 'symmetric'): (2, 0, 2, 1),
    ('box', 'nonrigid'): (6, 2, 6, 5),
    ('box', 'bad'): (7, 1, 4, 3),
    ('strip63', 'mixed'): (8, 3, 8, 3),
    ('strip64', 'mixed'): (8, 3, 8, 3),
    ('strip65', 'mixed'): (8, 3, 8, 3),
    ('strip65', 'bad'): (7, 1, 4, 1),
    ('sphere', 'mixed'): (8, 3, 8, 4),
    ('sphere', 'symmetric'): (2, 0, 2, 1),
    ('coincident', 'touching'): (4, 4, 4, 4),
    ('coincident', 'free'): (2, 0, 2, 0),
    ('probe_last', 'touching'): (4, 4, 4, 4),
    ('probe_last', 'free'): (4, 0, 4, 0),
    ('probe_first', 'touching'): (4, 4, 4, 4),
    ('probe_first', 'free'): (4, 0, 4, 0),
}


def test_every_mesh_and_every_set_is_a_case():
    assert {m for m, _ in pr.CASES} == set(pr.MESHES) and {s for _, s in pr.CASES} == set(pr.POSE_SETS)
    assert set(RECORDED) == set(pr.CASES)
    sizes = {name: pr.mesh(name)[1].shape[0] for name in pr.MESHES}
    assert sizes == {"single": 1, "box": 12, "strip63": 63, "strip64": 64, "strip65": 65, "sphere": 300, "coincident": 300, "probe_last": 40, "probe_first": 40}
    v, idx = pr.mesh("coincident")
    rec = pr.records_of(v, idx)
    assert np.array_equal(rec[3], rec[200]) and np.unique(rec, axis=0).shape[0] == 299


def test_transform_against_float64():
    """Three products and three sums per coordinate, each rounded once: the error is within gamma_4 = 4 u / (1 - 4 u) of
    sum |m| |x| + |t| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), u = 2^-24, plus the subnormal spacing"""
    u = 2.0 ** -24
    gamma = 4 * u / (1 - 4 * u)
    checked = 0
    for mesh_name, set_name in pr.CASES:
        records, poses, _ = pr.case(mesh_name, set_name)
        got = pr.transform(poses, records)
        assert got.dtype == np.float32 and got.shape == (poses.shape[0], records.shape[0], 12)
        assert (got[:, :, 3::4] == 0).all()
        with np.errstate(all="ignore"):
            want, mag = pr.transform_f64(poses, records)
        ok = np.isfinite(want) & (np.abs(want) < 1e38) & (mag < 1e38)
        v = got.reshape(got.shape[0], got.shape[1], 3, 4)[:, :, :, :3].astype(np.float64)
        assert (np.abs(v[ok] - want[ok]) <= gamma * mag[ok] + 2.0 ** -148).all(), (mesh_name, set_name)
        checked += int(ok.sum())
        if set_name == "identity":
            assert np.array_equal(got[0].view(np.uint32) & 0x7FFFFFFF, records.view(np.uint32) & 0x7FFFFFFF)      # x + 0 y + 0 z + 0 is x (up to the sign of a zero)
    assert checked > 10000
    # the bad set: the poses named bad give non-finite coordinates, the others do not
    records, poses, _ = pr.case("box", "bad")
    finite = np.isfinite(pr.transform(poses, records)).all(axis=(1, 2))
    assert finite.tolist() == [True, False, True, False, True, False, True]
    assert np.isfinite(poses[5]).all()                 # finite entries: the transform overflows


def test_reductions_against_a_per_pose_loop():
    verts, idx, mats = pr.cornell_scene()
    for mesh_name, set_name in (("box", "mixed"), ("box", "symmetric"), ("box", "bad"), ("strip65", "mixed"), ("probe_last", "touching")):
        ref = pr.cornell_reference(mesh_name, set_name)
        records, poses, radius = ref["records"], ref["poses"], ref["radius"]
        for p in range(poses.shape[0]):
            posed = pr.transform(poses[p:p + 1], records)[0]
            m = tt.intersect_matrix(posed, verts, idx).any(axis=1)
            assert ref["hit"][p] == int(m.any()) and ref["first"][p] == (np.flatnonzero(m)[0] if m.any() else pr.MISS), (mesh_name, set_name, p)
            for r, out in ((np.inf, ref["out_inf"]), (radius, ref["out_r"])):
                g = posed.copy()
                g[:, 3] = r                                    # the per-triangle reference applies the radius itself
                rec, d2 = tr.triangle_distance_records(g, verts, idx, mats, return_d2=True)
                found = np.flatnonzero(rec[:, 1] != pr.MISS)
                if found.size == 0:
                    assert np.array_equal(out[p], pr.miss_records(1)[0]), (mesh_name, set_name, p, r)
                    continue
                best = min(found, key=lambda t: (float(d2[t]), int(t)))
                want = rec[best].copy()
                want[7] = best
                assert np.array_equal(out[p], want), (mesh_name, set_name, p, r)
    # a NaN and a negative radius: every pose a miss
    ref = pr.cornell_reference("box", "mixed")
    for r in (np.nan, -1.0):
        assert np.array_equal(pr.reduce_distance(ref["rec_inf"], ref["d2"], r), pr.miss_records(ref["poses"].shape[0]))
    assert np.array_equal(pr.reduce_distance(ref["rec_inf"], ref["d2"], 0.0)[:, 1] != pr.MISS, (ref["d2"] == 0).any(axis=1))


def test_shares_of_every_case_as_recorded():
    for key in pr.CASES:
        ref = pr.cornell_reference(*key)
        got = (ref["poses"].shape[0], int(ref["hit"].sum()), int((ref["out_inf"][:, 1] != pr.MISS).sum()), int((ref["out_r"][:, 1] != pr.MISS).sum()))
        assert got == RECORDED[key], (key, got)
        # hit and first go together; a pose that intersects is at distance 0 of what it intersects or of a neighbour
        assert np.array_equal(ref["hit"] != 0, ref["first"] != pr.MISS)
    for key in pr.CASES:
        P, hit, found_inf, found_r = RECORDED[key]
        if key[1] == "mixed":
            assert 0 < hit < P and 0 < found_r < P, key                  # both classes, for both queries
        if key[1] == "free":
            assert hit == 0 and found_r == 0 and found_inf == P, key     # nothing within the radius of anything
        if key[1] in ("touching", "deep"):
            assert hit > 0, key
    # bad poses between good ones: the bad ones find nothing at any radius, their neighbours do
    for mesh_name in ("box", "strip65"):
        ref = pr.cornell_reference(mesh_name, "bad")
        assert (ref["out_inf"][:, 1] != pr.MISS).tolist() == [True, False, True, False, True, False, True]


def test_symmetric_poses_really_tie():
    for mesh_name in ("box", "sphere"):
        ref = pr.cornell_reference(mesh_name, "symmetric")
        for p in range(ref["poses"].shape[0]):
            d2 = ref["d2"][p]
            best = np.nanmin(d2)
            tied = np.flatnonzero(d2.view(np.uint32) == F(best).view(np.uint32))
            assert tied.size >= 2 and ref["out_inf"][p, 7] == tied[0], (mesh_name, p, tied)
    # the box: its -y face 8 (16) units above the floor and its -x face as far from the wall, exactly
    ref = pr.cornell_reference("box", "symmetric")
    assert ref["d2"][0, [0, 1, 2, 3]].tolist() == [64.0] * 4 and ref["d2"][1, [0, 1, 2, 3]].tolist() == [256.0] * 4
    # the coincident triangles: where triangle 3 wins, triangle 200 has the same d2 and loses
    ref = pr.cornell_reference("coincident", "free")
    assert np.array_equal(ref["d2"][:, 3].view(np.uint32), ref["d2"][:, 200].view(np.uint32))
    assert (ref["out_inf"][:, 7] == 3).any() and not (ref["out_inf"][:, 7] == 200).any()


def test_probe_meshes_have_the_property_claimed():
    verts, idx, _ = pr.cornell_scene()
    for mesh_name, needle in (("probe_last", 39), ("probe_first", 0)):
        ref = pr.cornell_reference(mesh_name, "touching")
        posed = pr.transform(ref["poses"], ref["records"])
        for p in pr.PROBE_POSES:
            m = tt.intersect_matrix(posed[p], verts, idx).any(axis=1)
            assert np.flatnonzero(m).tolist() == [needle], (mesh_name, p)
            assert ref["first"][p] == needle and ref["out_inf"][p, 7] == needle and ref["out_r"][p, 7] == needle
            others = np.delete(ref["d2"][p], needle)
            assert ref["d2"][p, needle] == 0 and (others > 100.0).all()


def test_wrappers_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the device is touched
    verts = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], np.float64)
    with pytest.raises(pt.PathTracerError, match="expected"):
        pt.setQueryMesh(state, verts[:, :2], [[0, 1, 2]])
    with pytest.raises(pt.PathTracerError, match="whole numbers"):
        pt.setQueryMesh(state, verts, [[0.0, 1.0, 2.0]])
    with pytest.raises(pt.PathTracerError, match="outside the 4 vertices"):
        pt.setQueryMesh(state, verts, [[0, 1, 4]])
    for call in (pt.posedTriangles, pt.queryPosesAny, pt.queryPosesDistance):
        for bad in (np.zeros((4, 7), np.float32), np.zeros(12, np.float32), np.zeros((2, 2, 4), np.float32), np.zeros((2, 3, 4, 1), np.float32)):
            with pytest.raises(pt.PathTracerError, match="expected"):
                call(state, bad)
        with pytest.raises(pt.PathTracerError, match="numbers"):
            call(state, np.zeros((2, 12), np.complex64))
    for bad in (-1.0, float("nan")):
        with pytest.raises(pt.PathTracerError, match="non-negative"):
            pt.queryPosesDistance(state, np.zeros((1, 12), np.float32), max_radius=bad)
    # the forms of the poses
    m = np.arange(32, dtype=np.float64).reshape(2, 4, 4)
    want = m[:, :3, :].reshape(2, 12).astype(np.float32)
    for form in (m, m[:, :3, :], want):
        got = pt.pathtracer._pose_records("t", state, form)
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want)
    assert np.array_equal(pt.pathtracer._pose_records("t", state, m[0]), want[:1]) and np.array_equal(pt.pathtracer._pose_records("t", state, m[0, :3]), want[:1])
    torch = pytest.importorskip("torch")
    for call in (pt.posedTriangles, pt.queryPosesAny, pt.queryPosesDistance):
        with pytest.raises(pt.PathTracerError, match="the context is on"):
            call(state, torch.zeros((4, 12), dtype=torch.float32))


def test_build_lists_header_and_bindings():
    assert "poses.hip" in _build.HIP_SOURCES and {"poses.h", "tridist_device.h", "tritri_device.h", "bvh_walk.h", "query_launch.h"} <= set(_build.HIP_HEADERS)
    for name in ("poses.hip", "poses.h", "tridist_device.h", "tridist.hip", "tritri_device.h", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    assert _native.ABI_VERSION == 4
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "acgpt.h")).read())
    for name, proto in (("pt_set_query_mesh", "int pt_set_query_mesh(pt_ctx* ctx, const float* tris, size_t ntris);"),
                        ("pt_get_query_mesh", "int pt_get_query_mesh(pt_ctx* ctx, size_t* ntris, size_t* device_bytes);"),
                        ("pt_pose_triangles", "int pt_pose_triangles(pt_ctx* ctx, const float* poses, size_t P, float* tris_out);"),
                        ("pt_query_poses_any", "int pt_query_poses_any(pt_ctx* ctx, const float* poses, size_t P, uint8_t* hit, uint32_t* first);"),
                        ("pt_query_poses_distance", "int pt_query_poses_distance(pt_ctx* ctx, const float* poses, size_t P, float max_radius, pt_pose_distance_hit* out);")):
        assert name in _native.ABI_SYMBOLS and proto in flat, name
    assert "x' = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]" in flat and "no fused multiply-add" in flat
    assert "#define PT_QUERY_MESH_MAX 1048576u" in flat and _native.QUERY_MESH_MAX == 1048576
    test_h = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "acgpt_test.h")).read())
    assert "pt_debug_query_poses" in _native.TEST_SYMBOLS
    assert "int pt_debug_query_poses(pt_ctx* ctx, const float* poses, size_t P, float max_radius, uint8_t* hit, uint32_t* first, pt_pose_distance_hit* out, uint32_t flags);" in test_h
    src = open(os.path.join(_build.CSRC, "poses.h")).read()
    assert re.search(r"kPoseNoEarly = %du;" % _native.POSES_NO_EARLY, src) and re.search(r"kPosePoseMajor = %du;" % _native.POSES_POSE_MAJOR, src)
    assert pt.POSE_DISTANCE_DTYPE.itemsize == 48 and pt.POSE_DISTANCE_DTYPE.fields["query_triangle"][1] == 28 and pt.POSE_DISTANCE_DTYPE.fields["point"][1] == 32
    L = _native.hip()                     # loads, does not touch the GPU
    for name in ("pt_set_query_mesh", "pt_get_query_mesh", "pt_pose_triangles", "pt_query_poses_any", "pt_query_poses_distance", "pt_debug_query_poses"):
        assert hasattr(L, name), name


def test_pose_kernels_use_no_scratch_memory_and_spill_nothing(built):
    """The transform, the four walks of the yes / no query (two node formats, with and without first), its finish, and the two phases of
    the distance query in both node formats: no private segment, no spilled vector or scalar register"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(_native.hip_library_path()) if re.search(r"\bk_pose_", k["name"])]
    assert len(rows) == 10, [k["name"] for k in rows]
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
