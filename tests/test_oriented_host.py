"""pt_query_overlap_oriented without a GPU: the NumPy statement (tests/oriented_ref.py) on hand-checked boxes, the miss rules with the
orthonormality tolerance, the identity set against overlap_ref pair for pair, fp32 against the same algorithm in float64, the box sets'
shares on the Cornell fixtures, pt_pose_boxes' statement, posedMeshBoxes' containment, the build lists, the header, the kernels'
registers, and the wrappers' argument checks that need no device."""
import os
import sys

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build, _native
import nearest_ref as nr
import oriented_ref as ob
import overlap_ref as ov
import poses_ref as pr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fp32 against float64: the share of boxes of a set whose list differs, capped at 1 % (the project's convention).  Measured on the Cornell
# box: identity 2, walls_turned 3, flat 2 of 1 000, 0 on the other sets.  The "far" set is held otherwise: its
# centres are 10 to 100 diagonals out, where v0 - c rounds by an ulp of |c| (3 % of its boxes have a triangle that close to a face);
# every pair on which the two differ there must flip within FAR_DELTA of |c|, the statement's own rounding (csrc/oriented.h: 22 u (S + C),
# below 2^-19 C for C >= S).
FP64_CAP = 0.01
FAR_DELTA = 2.0 ** -19

S2 = float(np.sqrt(0.5))
# A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0)
TRI = (np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 4, 0, 1]], np.float32), np.array([0, 1, 2], np.uint32))
EYE = np.eye(3, dtype=np.float32)
QUARTER_Z = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)       # local x is world y, local y is world -x
EIGHTH_Z = np.array([[S2, -S2, 0], [S2, S2, 0], [0, 0, 1]], np.float32)    # local x is the world diagonal (1, 1, 0) / sqrt 2


def _one(c, h, rot, verts=TRI[0], idx=TRI[1]):
    b = ob.as_oboxes([c], [h], rot)
    m = ob.overlap_matrix(b, verts, idx)
    v0, e1, e2 = nr.records_of_scene(verts, idx)
    A, cc, hh = ob.parts(b)
    groups = ov.conditions(np.zeros(3, np.float32), hh[0], ob.local(A[0], v0[0] - cc[0]), ob.local(A[0], e1[0]), ob.local(A[0], e2[0]))
    return bool(m[0, 0]), tuple(bool(g) for g in groups)


def test_hand_checked_boxes_of_one_triangle():
    """(overlap, (faces, plane, edges)): which group of conditions separates.  The quarter turn is exact in fp32; the eighth turn's
    cases keep a margin of a quarter against its rounding, except where a zero makes them exact."""
    cases = [
        ((1, 1, 0), (0.5, 0.5, 0.5), EYE, True, (True, True, True)),                  # inside the face, as the axis-aligned test has it
        ((1, 1, 0), (0.5, 0.5, 0.5), QUARTER_Z, True, (True, True, True)),
        ((5, 0, 0), (0.5, 2.0, 0.5), EYE, False, (False, True, False)),               # a tall box half a unit past B ...
        ((5, 0, 0), (0.5, 2.0, 0.5), QUARTER_Z, True, (True, True, True)),            # ... laid down by the quarter turn it reaches from x = 3 to 7
        ((6.5, 0, 0), (0.5, 2.0, 0.5), QUARTER_Z, False, (False, True, False)),       # and half a unit short of B
        ((6, 0, 0), (0.5, 2.0, 0.5), QUARTER_Z, True, (True, True, True)),            # touching B with a face: touching is overlap
        ((1, 1, 0.5), (0.25, 0.25, 0.5), QUARTER_Z, True, (True, True, True)),        # resting on the face from above
        ((1, 1, 0.75), (0.25, 0.25, 0.5), QUARTER_Z, False, (False, False, False)),   # a quarter above it
        ((3, 3, 0), (1.0, 0.25, 0.25), EIGHTH_Z, False, (False, True, False)),        # a stick along the diagonal, 1.41 from BC: a unit long it stays 0.41 short
        ((3.5, 3.5, 0), (2.5, 0.25, 0.25), EIGHTH_Z, True, (True, True, True)),       # 2.12 from BC and 2.5 long: it reaches across
        ((3, 3, 0), (1.0, 1.0, 1.0), EYE, True, (True, True, True)),                  # the unturned cube touches BC with its corner (2, 2) ...
        ((3, 3, 0), (1.0, 1.0, 1.0), EIGHTH_Z, False, (False, True, False)),          # ... turned by an eighth its face is 0.41 short
        ((2.5, 3.5, 0), (1.0, 0.25, 0.25), QUARTER_Z, False, (True, True, False)),    # x in [2.25, 2.75], y in [2.5, 4.5]: inside the bounding box, beside BC: only an edge axis separates
        ((1, 1, 0), (0, 0, 0), EIGHTH_Z, True, (True, True, True)),                   # a point box on the triangle
        ((1, 1, 0.25), (0, 0, 0), EIGHTH_Z, False, (False, False, False)),            # a point box off it
        ((1, 1, 0), (0, 0, 3), QUARTER_Z, True, (True, True, True)),                  # a segment piercing it
        ((-1, -1, 0), (2.0, 0, 0), EIGHTH_Z, True, (True, True, True)),               # a segment along the diagonal reaching past A
        ((-1, -1, 0), (1.0, 0, 0), EIGHTH_Z, False, (False, True, False)),            # one that stops 0.41 short of A
        ((1, 1, 0), (1, 1, 0), QUARTER_Z, True, (True, True, True)),                  # a rectangle in the triangle's plane
    ]
    for c, h, rot, want, groups in cases:
        got, g = _one(c, h, rot)
        assert got == want and g == groups, (c, h, rot.tolist(), got, g)
    # the case only the plane axis rejects: a tilted triangle, a small turned box inside its bounding box, beside no edge and off its plane
    verts = np.array([[0, 0, 0, 1], [8, 0, 8, 1], [0, 8, 8, 1]], np.float32)
    assert _one((2, 2, 1), (0.5, 0.5, 0.5), QUARTER_Z, verts) == (False, (True, False, True))
    assert _one((2, 2, 3), (0.5, 0.5, 0.5), QUARTER_Z, verts) == (True, (True, True, True))
    # a mirror is a box like any other
    assert _one((1, 1, 0), (0.5, 0.5, 0.5), np.diag([-1.0, 1.0, 1.0]).astype(np.float32))[0] is True


def test_the_miss_rules():
    good = ob.as_oboxes([[1, 1, 0]], [[0.5, 0.5, 0.5]], EIGHTH_Z)[0]
    assert ob.searchable(good[None]).all() and ob.overlap_records(good[None], *TRI)[0][0] == 1
    bad, why = ob.bad_boxes(good)
    assert bad.shape[0] == 15 * 3 + 6 and not ob.searchable(bad).any(), [w for w, s in zip(why, ob.searchable(bad)) if s]
    counts, prims, hit = ob.overlap_records(bad, *TRI, max_prims=4)
    assert not counts.any() and (prims == 0xFFFFFFFF).all() and not hit.any()
    # the reserved float is ignored; h = -0 is a zero; a mirror passes; so does every signed permutation
    odd = np.stack([good, good, good])
    odd[0, 15] = np.nan
    odd[1, 12:15] = -0.0
    odd[2, :12].reshape(3, 4)[:, :3] = np.diag([1.0, -1.0, 1.0])
    assert ob.searchable(odd).all() and ob.overlap_records(odd, *TRI)[0].tolist() == [1, 1, 1]
    assert ob.searchable(ob.as_oboxes(np.zeros((48, 3)), 1.0, ob.signed_permutations())).all()
    # the orthonormality rule: a uniform scale of 1 + 2^-11.2 passes and 1 + 2^-10.8 does not; likewise a shear; every rotation from a
    # quaternion passes by far; a matrix whose dot products overflow is a miss, not an error
    rot = ob.rotations(np.random.default_rng(7), 1000)
    A = ob.as_oboxes(np.zeros((1000, 3)), 1.0, rot)
    assert ob.searchable(A).all()
    u, v = rot[:, :, 0].astype(np.float64), rot[:, :, 1].astype(np.float64)
    assert np.abs((u * u).sum(axis=1) - 1.0).max() < 2e-7 * 2 and np.abs((u * v).sum(axis=1)).max() < 2e-7 * 2
    for s, ok in ((1.0 + 2.0 ** -11.2, True), (1.0 + 2.0 ** -10.8, False), (1.0 - 2.0 ** -11.2, True), (1.0 - 2.0 ** -10.8, False), (0.0, False), (2.0, False)):
        assert ob.searchable(ob.as_oboxes(np.zeros((1000, 3)), 1.0, rot.astype(np.float64) * s)).all() == ok, s
        assert ob.searchable(ob.as_oboxes(np.zeros((1000, 3)), 1.0, rot.astype(np.float64) * s)).any() == ok, s
    huge = ob.as_oboxes([[0, 0, 0]], 1.0, np.eye(3) * 3e38)
    assert np.isfinite(huge[:, :15]).all() and not ob.searchable(huge).any()
    # a scene without triangles
    counts, prims, hit = ob.overlap_records(odd, np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), max_prims=3)
    assert counts.shape == (3,) and not counts.any() and prims.shape == (3, 3) and (prims == 0xFFFFFFFF).all() and not hit.any()


@pytest.fixture(scope="module")
def cornell():
    """scene file -> (verts, idx, {set: (boxes, fp32 overlap matrix)}): the brute force, computed once, shared, never written"""
    out = {}
    for scene in ("cornell_box.obj", "cornell_box_diffuse.obj"):
        obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, scene))
        verts, idx = obj.getVerticesFloat(), obj.getIndexBuffer()
        sets = {}
        for name in ob.BOX_SETS:
            b = ob.box_set(name, verts, idx)
            m = ob.overlap_matrix(b, verts, idx)
            b.setflags(write=False); m.setflags(write=False)
            sets[name] = (b, m)
        out[scene] = (verts, idx, sets)
    return out


def test_identity_set_equals_overlap_ref_pair_for_pair(cornell):
    for scene, (verts, idx, sets) in cornell.items():
        b, m = sets["identity"]
        aabbs = ob.identity_aabbs(verts, idx)
        assert np.array_equal(b[:, :12].reshape(-1, 3, 4)[:, :, :3], np.broadcast_to(EYE, (b.shape[0], 3, 3)))
        assert np.array_equal(m, ov.overlap_matrix(aabbs, verts, idx)) and m.sum() > 1000
        assert np.array_equal(ob.searchable(b), ov.searchable(aabbs))


def test_fp32_statement_against_float64(cornell):
    verts, idx, sets = cornell["cornell_box.obj"]
    shares = {}
    for name, (b, m32) in sets.items():
        m64 = ob.overlap_matrix(b, verts, idx, np.float64)
        shares[name] = float((m32 != m64).any(axis=1).mean())
        print("%s: %d pairs kept, %d of %d boxes differ from float64" % (name, m32.sum(), (m32 != m64).any(axis=1).sum(), b.shape[0]))
        if name != "far":
            assert shares[name] <= FP64_CAP, (name, shares[name])
    assert max(shares[n] for n in ("walls_turned", "flat", "identity")) > 0.0          # there are contacts, and they are rare
    # far from the scene every pair that differs is a contact within the statement's rounding of |c|
    b, m32 = sets["far"]
    m64 = ob.overlap_matrix(b, verts, idx, np.float64)
    delta = (FAR_DELTA * np.abs(b[:, 3:12:4].astype(np.float64)).max(axis=1))[:, None]
    grown, shrunk = b.copy(), b.copy()
    grown[:, 12:15] = (b[:, 12:15].astype(np.float64) + delta).astype(np.float32)
    shrunk[:, 12:15] = np.maximum(b[:, 12:15].astype(np.float64) - delta, 0.0).astype(np.float32)
    diff = m32 != m64
    assert diff.any() and shares["far"] < 0.10
    assert not (diff & m32 & ~ob.overlap_matrix(grown, verts, idx, np.float64)).any()      # kept by fp32 alone: within delta of the box
    assert not (diff & ~m32 & ob.overlap_matrix(shrunk, verts, idx, np.float64)).any()     # dropped by fp32 alone: not delta inside it


@pytest.mark.parametrize("scene", ["cornell_box.obj", "cornell_box_diffuse.obj"])
def test_box_sets_shares_on_the_reference(cornell, scene):
    """The shares the GPU tests rely on, by the brute force alone"""
    verts, idx, sets = cornell[scene]
    n_tris = len(idx) // 3
    for name in ob.MIXED_SETS:
        b, m = sets[name]
        counts = m.sum(axis=1)
        above = {k: float((counts > k).mean()) for k in (1, 4, 8)}
        print("%s %s: %.3f empty, above 1 / 4 / 8: %.3f / %.3f / %.3f, %d triangles named" % (scene, name, (counts == 0).mean(), above[1], above[4], above[8], m.any(axis=0).sum()))
        assert np.isfinite(b).all() and ob.searchable(b).all()
        assert (counts == 0).mean() >= 0.10 and (counts != 0).mean() >= 0.25, name
        assert min(above.values()) >= 0.01, (name, above)
        assert m.any(axis=0).sum() >= 64, name
    # the links are long and thin; their world AABBs report several times the triangles and call empty boxes occupied
    b, m = sets["links"]
    h = np.sort(b[:, 12:15], axis=1)
    assert (h[:, 2] >= 2.4 * h[:, 1]).all()
    ma = ov.overlap_matrix(ob.world_aabbs(b), verts, idx)
    assert not (m & ~ma).any() and ma.sum() >= 5 * m.sum() and (ma.any(axis=1) & ~m.any(axis=1)).sum() >= 0.05 * ma.any(axis=1).sum()
    for name in ("axis_turns", "walls_turned", "far"):
        b, m = sets[name]
        assert ob.searchable(b).all() and m.any(axis=1).mean() >= 0.25 and (~m.any(axis=1)).mean() >= 0.10, name
    b, m = sets["walls_turned"]
    counts = m.sum(axis=1)
    assert (counts > 8).mean() >= 0.01
    A = b[:, :12].reshape(-1, 3, 4)[:, :, :3]
    assert ((A == 1.0).sum(axis=(1, 2)) >= 1).all() and ((A == 0.0).sum(axis=(1, 2)) >= 4).all()      # a turn about one world axis, that axis exact
    b, m = sets["flat"]
    h = b[:, 12:15]
    zeros = (h == 0).sum(axis=1)
    assert all((zeros == z).mean() >= 0.2 for z in (0, 1, 2, 3))
    assert m.any(axis=1)[zeros < 3].all()                      # segments, rectangles and thin boxes on the surface all find it; points need not
    b, m = sets["tolerance"]
    inside = ob.tolerance_kinds(b.shape[0]) < 3
    assert np.array_equal(ob.searchable(b), inside) and not m[~inside].any() and m[inside].any(axis=1).mean() >= 0.25
    assert np.isfinite(b).all() and (b[:, 12:15] >= 0).all()   # only the orthonormality rule makes the outside ones misses
    b, m = sets["whole"]
    assert (m.sum(axis=1) == n_tris).all()
    b, m = sets["outside"]
    assert not m.any()
    b, m = sets["far"]
    lo, hi = nr.scene_box(verts, idx)
    diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    assert (np.abs(b[:, 3:12:4] - 0.5 * (lo + hi)).max(axis=1) > 9.0 * diag).all()
    b, m = sets["grid_frame"]
    assert (b[:, :12].reshape(-1, 3, 4)[:, :, :3] == b[0, :12].reshape(3, 4)[:, :3]).all() and not np.array_equal(b[0, :12].reshape(3, 4)[:, :3], EYE)


def test_pose_boxes_statement():
    poses = pr.as_poses(pr._rigid(ob.rotations(np.random.default_rng(1), 5).astype(np.float64), [[1, 2, 3], [0, 0, 0], [-500, 20, 1e6], [0.1, 0.2, 0.3], [7, 7, 7]]))
    lb = np.array([3.5, -20.25, 7.125, 30.0, 0.0, 12.5], np.float32)
    got = ob.pose_boxes(poses, lb)
    assert got.shape == (5, 16) and got.dtype == np.float32
    m, g = poses.reshape(5, 3, 4), got[:, :12].reshape(5, 3, 4)
    assert np.array_equal(g[:, :, :3], m[:, :, :3]) and np.array_equal(got[:, 12:15], np.broadcast_to(lb[3:], (5, 3))) and not got[:, 15].any()
    # the centre is the pose statement applied to the local centre: the posed vertex of pt_pose_triangles
    rec = np.zeros((1, 12), np.float32)
    rec[0, 0:3] = lb[:3]
    assert np.array_equal(g[:, :, 3], pr.transform(poses, rec)[:, 0, 0:3])
    # with the local centre at the origin the record is the pose
    assert np.array_equal(ob.pose_boxes(poses, [0, 0, 0, 1, 2, 3])[:, :12], poses)


@pytest.mark.parametrize("mesh", ["box", "sphere", "strip65", "single", "probe_last"])
def test_posed_mesh_boxes_hold_every_posed_vertex(mesh):
    """By the fp32 statement: the local coordinates of every posed vertex of pt_pose_triangles (poses_ref.transform) lie within the half
    extent, for every pose of poses_ref's sets whose record is searchable; the poses that are not rigid make records that are misses."""
    v, idx = pr.mesh(mesh)
    records = pr.records_of(v, idx)
    state = pt.PathTracerState()
    seen = 0
    for set_name in pr.POSE_SETS:
        poses = pr.pose_set(set_name, v)
        t = float(np.nan_to_num(np.abs(poses[:, 3::4]), nan=0.0, posinf=0.0, neginf=0.0).max())
        pad = pt.posedMeshBoxPad(v, t)
        lo, hi = v.astype(np.float64).min(axis=0) - pad, v.astype(np.float64).max(axis=0) + pad
        lb = pt.pathtracer._local_box("test", lo, hi)
        assert (lb[:3].astype(np.float64) - lb[3:].astype(np.float64) <= lo).all() and (lb[:3].astype(np.float64) + lb[3:].astype(np.float64) >= hi).all()
        boxes = ob.pose_boxes(poses, lb)
        ok = ob.searchable(boxes)
        if set_name in ("identity", "free", "touching", "deep", "mixed", "symmetric"):
            assert ok.all(), set_name
        if set_name == "nonrigid":
            assert ok.tolist() == [False, False, True, False, False, False]      # the mirror is a box
        posed = pr.transform(poses, records).reshape(poses.shape[0], -1, 3, 4)[:, :, :, :3].reshape(poses.shape[0], -1, 3)
        A, c, h = ob.parts(boxes)
        with np.errstate(all="ignore"):
            loc = ob.local(A[:, None], posed - c[:, None])
        inside = (np.abs(loc) <= h[:, None]).all(axis=(1, 2))
        assert inside[ok & np.isfinite(posed).all(axis=(1, 2))].all(), (mesh, set_name, np.flatnonzero(ok & ~inside))
        seen += int(ok.sum())
    assert seen >= 20
    with pytest.raises(pt.PathTracerError, match="vertices"):
        pt.posedMeshBoxes(state, np.zeros((0, 3)), np.zeros((1, 12)))
    with pytest.raises(pt.PathTracerError, match="pad"):
        pt.posedMeshBoxes(state, v, np.zeros((1, 12)), pad=-1.0)


def test_build_lists_and_abi():
    assert "oriented.hip" in _build.HIP_SOURCES and "oriented.h" in _build.HIP_HEADERS and "oriented_device.h" in _build.HIP_HEADERS
    for name in ("oriented.hip", "oriented.h", "oriented_device.h", "lists.hip", "capi_query.hip"):
        assert name not in _build.KERNEL_SOURCES            # pt_kernel_source_hash() does not move
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b"
    for sym in ("pt_query_overlap_oriented", "pt_query_overlap_oriented_any", "pt_query_overlap_oriented_lists", "pt_pose_boxes"):
        assert sym in _native.ABI_SYMBOLS
    assert "pt_debug_overlap_oriented_visits" in _native.TEST_SYMBOLS and "pt_debug_overlap_oriented_visits_cross" in _native.TEST_SYMBOLS
    assert _native.ABI_VERSION == 4 and float(pt.OBOX_ORTHO_TOL) == float(ob.ORTHO_TOL) == 2.0 ** -10
    hdr = open(os.path.join(ROOT, "include", "acgpt.h")).read()
    for proto in ("int pt_query_overlap_oriented(pt_ctx* ctx, const float* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts);",
                  "int pt_query_overlap_oriented_any(pt_ctx* ctx, const float* boxes, size_t n, uint8_t* hit);",
                  "int pt_query_overlap_oriented_lists(pt_ctx* ctx, const float* boxes, size_t n, const uint32_t* offsets,\n"
                  "                                    uint32_t* prims, size_t capacity, uint32_t* found);",
                  "int pt_pose_boxes(pt_ctx* ctx, const float* poses, size_t P, const float local_box[6], float* boxes_out);"):
        assert proto in hdr, proto
    test_hdr = open(os.path.join(ROOT, "include", "acgpt_test.h")).read()
    assert "int pt_debug_overlap_oriented_visits(pt_ctx* ctx, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits);" in test_hdr
    src = open(os.path.join(_build.CSRC, "oriented.h")).read()
    assert "kOBoxOrthoTol = 0x1p-10f" in src


def test_kernels_have_no_scratch_and_no_spills(built):
    """tools/kernel_meta.py on the built library: the oriented kernels and the oriented fill"""
    lib = _native.hip_library_path()
    if not os.path.exists(lib):
        _build.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    rows = [k for k in kernel_meta.kernel_table(lib) if "k_query_oriented" in k["name"] or "k_posed_boxes" in k["name"] or "k_fill_oriented" in k["name"]]
    assert len(rows) == 12 + 2 + 1 + 4, [k["name"] for k in rows]          # the product's twelve, the two counting walks of the cross-axis arm, the poser, the fill
    for k in rows:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] <= 96, k                     # five waves per SIMD at the least


def test_wrapper_argument_checks_need_no_device():
    state = pt.PathTracerState()              # no context: every refusal below comes before the library is touched
    c3, h3 = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    b = pt.orientedBoxes(c3, h3, EIGHTH_Z)
    assert b.shape == (4, 16) and b.dtype == np.float32 and np.array_equal(b, ob.as_oboxes(c3, h3, EIGHTH_Z))
    assert np.array_equal(pt.orientedBoxes(c3, 2.0, np.broadcast_to(QUARTER_Z, (4, 3, 3))), ob.as_oboxes(c3, 2.0, QUARTER_Z))
    for bad_c in (np.zeros((4, 2)), np.zeros(3), [[1, 2]]):
        with pytest.raises(pt.PathTracerError, match="centres"):
            pt.orientedBoxes(bad_c, 1.0, EYE)
    with pytest.raises(pt.PathTracerError, match="broadcast"):
        pt.orientedBoxes(c3, np.ones((3, 3)), EYE)
    for bad_h in (-1.0, float("nan"), [1.0, -0.5, 1.0]):
        with pytest.raises(pt.PathTracerError, match="non-negative"):
            pt.orientedBoxes(c3, bad_h, EYE)
    for bad_r in (np.eye(4), np.zeros((3, 3, 3)), np.zeros((4, 3))):
        with pytest.raises(pt.PathTracerError, match="rotations"):
            pt.orientedBoxes(c3, 1.0, bad_r)
    with pytest.raises(pt.PathTracerError, match="numbers"):
        pt.orientedBoxes(c3, 1.0, np.eye(3).astype(np.complex64))
    for fn in (pt.queryOverlapOriented, pt.queryOverlapOrientedAny, pt.queryOverlapOrientedLists):
        for bad in (np.zeros((4, 8), np.float32), np.zeros(16, np.float32), np.zeros((2, 16, 1), np.float32), [[1, 2]]):
            with pytest.raises(pt.PathTracerError, match="expected"):
                fn(state, bad)
        with pytest.raises(pt.PathTracerError, match="numbers"):
            fn(state, np.zeros((2, 16), np.complex64))
        # NumPy records that fail the orthonormality rule: ValueError, naming the first
        for rot in (1.5 * np.eye(3), np.array([[1, 0.5, 0], [0, 1, 0], [0, 0, 1]]), np.zeros((3, 3)), EIGHTH_Z.astype(np.float64) * (1.0 + 2.0 ** -10.8)):
            mixed = np.concatenate([b, pt.orientedBoxes(c3[:1], 1.0, rot)])
            with pytest.raises(ValueError, match="box 4 are not orthonormal"):
                fn(state, mixed)
    for bad in (9, -1, 2.5, "x", None):
        with pytest.raises(pt.PathTracerError, match="max_prims"):
            pt.queryOverlapOriented(state, b, max_prims=bad)
    with pytest.raises(pt.PathTracerError, match="counts=True"):
        pt.queryOverlapOriented(state, b, max_prims=0, counts=False)
    # no boxes: nothing to do
    none = np.zeros((0, 16), np.float32)
    got = pt.queryOverlapOriented(state, none, max_prims=3)
    assert sorted(got) == ["count", "prim"] and got["prim"].shape == (0, 3) and got["prim"].dtype == np.uint32 and got["count"].shape == (0,)
    assert sorted(pt.queryOverlapOriented(state, none, counts=False)) == ["prim"]
    assert pt.queryOverlapOrientedAny(state, none).shape == (0,) and pt.queryOverlapOrientedAny(state, none).dtype == np.bool_
    lists = pt.queryOverlapOrientedLists(state, none)
    assert lists["offsets"].tolist() == [0] and lists["prim"].shape == (0,) and lists["count"].shape == (0,)
    torch = pytest.importorskip("torch")
    with pytest.raises(pt.PathTracerError, match="the context is on"):
        pt.queryOverlapOriented(state, torch.zeros((4, 16), dtype=torch.float32))
    # the grid in a frame, and bakeOccupancy's refusals
    frame = np.hstack([QUARTER_Z.astype(np.float64), [[10.0], [20.0], [30.0]]])
    cells = pt.occupancyBoxes((2, 3, 4), (0.0, 10.0, 100.0), (4.0, 13.0, 102.0), frame=frame)
    plain = pt.occupancyBoxes((2, 3, 4), (0.0, 10.0, 100.0), (4.0, 13.0, 102.0))
    assert cells.shape == (24, 16) and np.array_equal(cells[:, 12:15], plain[:, 3:6]) and ob.searchable(cells).all()
    want = plain[:, 0:3].astype(np.float64) @ QUARTER_Z.astype(np.float64).T + np.array([10.0, 20.0, 30.0])
    assert np.array_equal(cells[:, 3:12:4], want.astype(np.float32)) and (cells[:, :12].reshape(-1, 3, 4)[:, :, :3] == QUARTER_Z).all()
    for bad in (np.eye(3), "x", np.full((3, 4), np.nan), np.zeros((2, 4))):
        with pytest.raises(pt.PathTracerError, match="bakeOccupancy: frame"):
            pt.bakeOccupancy(state, (2, 2, 2), bounds=((0, 0, 0), (1, 1, 1)), frame=bad)
    with pytest.raises(pt.PathTracerError, match="bounds must be given"):
        pt.bakeOccupancy(state, (2, 2, 2), frame=frame)
    with pytest.raises(ValueError, match="orthonormal"):
        pt.bakeOccupancy(state, (2, 2, 2), bounds=((0, 0, 0), (1, 1, 1)), frame=np.hstack([2.0 * np.eye(3), np.zeros((3, 1))]))
    for lo, hi in (((0, 0, 0), (1, 1, -1)), ((0, 0), (1, 1)), ((0, 0, np.nan), (1, 1, 1))):
        with pytest.raises(pt.PathTracerError, match="poseBoxes: lo and hi"):
            pt.poseBoxes(state, np.zeros((1, 12)), lo, hi)
