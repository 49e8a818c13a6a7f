"""Generalised winding numbers on the GPU: pt_query_winding against tests/winding_ref.py.

The moments (pt_debug_read_winding) equal winding_ref.moments on the tree the device holds (pt_debug_read_tree), every word, as bits;
the two counts of the counting twin equal winding_ref.walk's on those moments, integer for integer; the values are held to the
float64 sum over the same accepted set within 8 x max(E32, 2^-23), E32 the largest difference on that set of points between the
float32 and the float64 reference (both the GPU and the float32 reference are fp32 evaluations of one formula; the device's atan2f is
allowed a few ulps where NumPy's is correctly rounded, x 4; the walk's order of summation differs from the sequential one, x 2).
Points closer to the surface than 1e-3 of the scene's diagonal are left out of the value comparison only
(tests/test_winding_host.py holds their share under 5 %).  Then what the number means on a closed and on a holed icosphere, the edge
scenes, the outputs' bounds, the lifetime of the moments, the render state, the refusals, torch tensors and the wrappers."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import multihit_ref as mr
import nearest_ref as nr
import query_scenes as qs
from test_gpu_refit_edges import _table
import tree_ref as tr
import winding_ref as wr

F = np.float32
pytestmark = pytest.mark.gpu

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
BOX_DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)       # around a wave and a workgroup, and several workgroups
BETAS = (1.0, 2.0, 3.0, 8.0, np.inf)
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
GUARD = 64                                         # bytes of 0xCD kept in front of and behind every output
NEAR_REL = 1e-3
VALUE_SETS = ("inside", "shell")                   # `features` sits on the surface: decisions and finiteness only
ICO_CENTRE, ICO_RADIUS = (0.25, -0.5, 1.0), 1.5


def _L():
    return _native.hip()


def _obj_arrays(path):
    obj = pt.TinyObjWrapper(path)
    v = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    return v, np.ascontiguousarray(obj.getIndexBuffer(), np.uint32).reshape(-1, 3), np.ascontiguousarray(obj.getMaterialIndices(), np.uint32), _table(obj.getMaterials())


def _ico_arrays(subdiv, drop=0):
    v, idx = mr.icosphere(subdiv, ICO_CENTRE, ICO_RADIUS)
    idx = idx[drop:]
    return v, idx, np.zeros(len(idx), np.uint32), qs.box()[3]


@pytest.fixture
def ctxs():
    made = []

    def make(v, idx, ids, mats, **kw):
        c = qs._Ctx.from_arrays(v, idx, ids, mats, **kw)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


@pytest.fixture(scope="module")
def scenes():
    """name -> (context, verts, idx): the Cornell fixtures under the default variant (fp16 centre / half-extent nodes), the box under
    an fp32-node variant, the icosphere at subdivision 2 and 3; each set up once"""
    made = {}

    def get(name):
        if name not in made:
            if name in ("ico2", "ico3"):
                v, idx, ids, mats = _ico_arrays(int(name[3]))
                kw = {}
            else:
                v, idx, ids, mats = _obj_arrays(BOX_DIFFUSE if name == "diffuse" else BOX)
                kw = {"variant": 1} if name == "fp32" else {}
            made[name] = (qs._Ctx.from_arrays(v, idx, ids, mats, **kw), v, idx)
        return made[name]

    yield get
    for c, _, _ in made.values():
        c.close()


class Device:
    """points in a device buffer, an output with 64 bytes of 0xCD in front of and behind it at an address that is 4- but not 16-byte
    aligned, and the visit counts; the C ABI called as a C caller would.  Calls take the first n points."""

    def __init__(self, c, points):
        self.c, self.n_max = c, len(points)
        p = np.zeros((max(self.n_max, 1), 4), np.float32)
        p[:self.n_max, :3] = np.asarray(points, np.float32)[:, :3]
        p[:, 3] = np.float32("nan")                                  # the fourth float is ignored
        self.bufs = c._alloc((p.nbytes, 4 * len(p) + 2 * GUARD + 16, 8 * len(p) + 2 * GUARD + 16))
        self.p, self.out, self.visits = self.bufs[0], self.bufs[1] + GUARD + 4, self.bufs[2] + GUARD + 8
        assert self.out % 4 == 0 and self.out % 16 != 0 and self.visits % 8 == 0
        assert c.L.pt_copy_to_device(c.ctx, self.p, p.ctypes.data, p.nbytes) == 0

    def _arm(self, ptr, nbytes):
        assert self.c.L.pt_device_memset(self.c.ctx, ptr - GUARD, 0xCD, nbytes + 2 * GUARD) == 0

    def _read(self, ptr, nbytes, what):
        raw = np.zeros(nbytes + 2 * GUARD, np.uint8)
        assert self.c.L.pt_copy_to_host(self.c.ctx, raw.ctypes.data, ptr - GUARD, raw.nbytes) == 0
        assert (raw[:GUARD] == 0xCD).all(), "written in front of " + what
        assert (raw[GUARD + nbytes:] == 0xCD).all(), "written past the end of " + what
        return raw[GUARD:GUARD + nbytes].copy()

    def winding(self, beta, n=None, visits=False):
        """w float32 [n][, visits uint32 [n, 2]]"""
        c = self.c
        n = self.n_max if n is None else n
        self._arm(self.out, 4 * n)
        if visits:
            self._arm(self.visits, 8 * n)
            assert c.L.pt_debug_winding_visits(c.ctx, self.p, n, beta, self.out, self.visits) == 0, c.err()
        else:
            assert c.L.pt_query_winding(c.ctx, self.p, n, beta, self.out) == 0, c.err()
        w = self._read(self.out, 4 * n, "out").view(np.float32)
        return (w, self._read(self.visits, 8 * n, "visits").view(np.uint32).reshape(n, 2)) if visits else w

    def free(self):
        for p in self.bufs:
            self.c.L.pt_device_free(self.c.ctx, p)


def winding_info(c):
    w = _native.WindingInfo()
    assert c.L.pt_get_winding_info(c.ctx, C.byref(w)) == 0, c.err()
    return int(w.built), int(w.n_nodes), int(w.bytes)


def build_moments(c):
    """one call of pt_query_winding: the moments are built by it"""
    d = Device(c, np.zeros((1, 3), np.float32))
    try:
        d.winding(2.0)
    finally:
        d.free()


def device_tree(c):
    """(children int32 [n, 2], empty bool [n, 2], records uint32 [n_tris, 12]) of the tree as the device holds it"""
    ti = _native.TreeInfo()
    assert c.L.pt_debug_read_tree(c.ctx, 0, None, 0, C.byref(ti)) == 0, c.err()
    what = next(w for w in (1, 3, 2) if ti.held >> (w - 1) & 1)
    words = np.zeros(ti.n_nodes * (16 if what == 1 else 8), np.uint32)
    assert c.L.pt_debug_read_tree(c.ctx, what, words.ctypes.data, words.nbytes, None) == 0, c.err()
    rec = np.zeros(ti.n_tris * 12, np.uint32)
    assert c.L.pt_debug_read_tree(c.ctx, 5, rec.ctypes.data, rec.nbytes, None) == 0, c.err()
    children = tr.children_of(what, words)[0]
    if what == 1:
        lo, hi = tr.fp32_boxes(words)
        empty = ~(lo <= hi).all(axis=2)
    elif what == 2:
        g_lo, g_hi = tr.half_planes(words)
        empty = ~(g_lo <= g_hi).all(axis=2)
    else:
        empty = (tr.half_planes(words)[1] < 0).any(axis=2)
    assert empty.sum() == (1 if ti.n_tris == 1 else 0)
    return children, empty, rec.reshape(-1, 12)


def read_moments(c):
    built, n_nodes, nbytes = winding_info(c)
    assert built == 1 and nbytes == 96 * n_nodes and n_nodes == c.info().n_nodes
    out = np.zeros((n_nodes, 8), np.float32)
    assert c.L.pt_debug_read_winding(c.ctx, out.ctypes.data, out.nbytes) == 0, c.err()
    return out


def check_moments(c, what=()):
    """the moments the device holds equal the reference on the device's tree, every word; returns (tree, moments)"""
    build_moments(c)
    tree = device_tree(c)
    got, want = read_moments(c), wr.moments(*tree)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, what + (len(bad), bad[:4].tolist(), got[bad[:2, 0]], want[bad[:2, 0]])
    return tree, got


# ---- moments ----------------------------------------------------------------------------------------------------------------------

def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("scene", ["box", "ico3"])
def test_moments_equal_the_reference_in_every_build_mode(ctxs, scene, mode):
    v, idx, ids, mats = _obj_arrays(BOX) if scene == "box" else _ico_arrays(3)
    for kw in ({}, {"variant": 1}):
        c = ctxs(v, idx, ids, mats, build_mode=mode, **kw)
        assert winding_info(c) == (0, 0, 0)
        (children, empty, rec), m = check_moments(c, (scene, mode, kw))
        assert len(rec) == len(idx) and np.isfinite(m).all() and (m[:, 7] > 0).all() and (m[:, 3] > 0).all()
        # the root's sums are the mesh's: the area, and for the closed icosphere a normal sum of nothing
        area = 0.5 * np.linalg.norm(np.cross(*(lambda t: (t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]))(v[:, :3].astype(np.float64)[idx.astype(np.int64)])), axis=1).sum()
        assert abs(m[0, 7] / area - 1) < 1e-5
        if scene == "ico3":
            assert np.abs(m[0, 4:7]).max() < 1e-5 * area


@pytest.mark.parametrize("n_tris", [255, 256, 257])
def test_moments_around_one_workgroup_of_leaves(ctxs, n_tris):
    v, idx, ids, mats = _ico_arrays(2)
    rng = np.random.default_rng(n_tris)
    keep = np.sort(rng.permutation(len(idx))[:n_tris])
    c = ctxs(v, idx[keep], ids[keep], mats)
    assert c.info().n_nodes == n_tris - 1
    check_moments(c, (n_tris,))


def test_moments_after_a_refit_and_after_a_material_edit(ctxs):
    v, idx, ids, mats = _obj_arrays(BOX)
    c = ctxs(v, idx, ids, mats)
    check_moments(c)
    before = read_moments(c)
    info = winding_info(c)
    # a material edit: kept, unchanged
    n_mats = len(mats)
    c.update_materials(mats, ((ids + 1) % n_mats).astype(np.uint32))
    assert winding_info(c) == info and np.array_equal(read_moments(c).view(np.uint32), before.view(np.uint32))
    # a refit: released, rebuilt lazily, equal to the reference on the refitted tree and to a fresh scene's
    moved = v.copy()
    lo, hi = nr.scene_box(v, idx)
    inner = ((v[:, :3] > lo + 1.0) & (v[:, :3] < hi - 1.0)).all(axis=1)
    assert 8 <= inner.sum() < len(v)
    moved[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
    rc, ui = c.update(moved)
    assert rc == 0 and not ui.rebuilt, c.err()
    assert winding_info(c) == (0, 0, 0)
    out = np.zeros((info[1], 8), np.float32)
    assert c.L.pt_debug_read_winding(c.ctx, out.ctypes.data, out.nbytes) != 0 and b"not built" in c.err()      # never builds them
    assert winding_info(c) == (0, 0, 0)
    tree, after = check_moments(c)
    assert winding_info(c) == info and not np.array_equal(after.view(np.uint32), before.view(np.uint32))
    pts = nr.point_set("inside", moved.reshape(-1), idx.reshape(-1), qs.camera(qs.SCENES["box"]))[:257]
    fresh = ctxs(moved, idx, c.mid, c.mats)
    d0, d1 = Device(c, pts), Device(fresh, pts)
    try:
        # a fresh build of the moved scene is another tree: the exact sums agree as two orders of the same terms do, both held to
        # the brute force on the moved vertices; at beta = 2 each is held to the reference walk on its own tree
        want, want32 = wr.exact(pts, moved, idx.reshape(-1)), wr.exact(pts, moved, idx.reshape(-1), np.float32)
        far = _far("box", pts, moved, idx)
        bar = 8 * max(float(np.abs(want32 - want)[far].max()), 2.0 ** -23)
        for ctx, dev in ((c, d0), (fresh, d1)):
            assert np.abs(dev.winding(np.inf) - want)[far].max() <= bar
            t = device_tree(ctx)
            w, vis = dev.winding(2.0, visits=True)
            assert np.array_equal(vis, wr.walk(*t[:2], read_moments(ctx), t[2], pts, 2.0)[0])
    finally:
        d0.free(); d1.free()
    # a new scene: released with the old one
    c.set_scene(v)
    assert winding_info(c) == (0, 0, 0)
    check_moments(c)
    assert np.array_equal(read_moments(c).view(np.uint32), before.view(np.uint32))


# ---- decisions and values ---------------------------------------------------------------------------------------------------------

def _points(name, set_name, v, idx):
    """(points [1000, 3], far bool: at least 1e-3 of the diagonal from the surface)"""
    if name.startswith("ico"):
        pts = mr.shell_points(1000, ICO_CENTRE, ICO_RADIUS)[0]
        return pts, np.ones(len(pts), bool)                  # 2 % of the radius from the sphere at least, the faces sag 1 % at most
    pts = nr.point_set(set_name, v.reshape(-1), idx.reshape(-1), qs.camera(qs.SCENES["box"]))
    return pts, _far(name, pts, v, idx)


def _far(name, pts, v, idx):
    """which points keep at least 1e-3 of the scene's diagonal from the surface (nearest_ref's brute force)"""
    lo, hi = nr.scene_box(v, idx)
    dist = nr.nearest_records(nr.with_radius(pts, np.inf), v.reshape(-1), idx.reshape(-1), np.zeros(len(idx), np.uint32)).view(np.float32)[:, 0]
    return dist >= NEAR_REL * float(np.linalg.norm(hi.astype(np.float64) - lo))


CASES = [(s, k) for s in ("box", "diffuse", "fp32") for k in ("inside", "shell", "features")] + [("ico2", "shell"), ("ico3", "shell")]


@pytest.mark.parametrize("scene,set_name", CASES)
def test_decisions_and_values_against_the_reference_walk(scenes, scene, set_name):
    c, v, idx = scenes(scene)
    n_tris = len(idx)
    tree, m = check_moments(c, (scene,))
    pts, far = _points(scene, set_name, v, idx)
    compare = far if (set_name in VALUE_SETS or scene.startswith("ico")) else np.zeros(len(pts), bool)
    if compare.any():
        assert far.mean() > 0.95
    before = c.info().device_bytes
    d = Device(c, pts)
    worst = {}
    try:
        for beta in BETAS:
            vis_ref, w64 = wr.walk(*tree[:2], m, tree[2], pts, beta, np.float64)
            _, w32 = wr.walk(*tree[:2], m, tree[2], pts, beta, np.float32)
            if np.isinf(beta):
                assert (vis_ref[:, 0] == 0).all() and (vis_ref[:, 1] == n_tris).all()
                w64, w32 = wr.exact(pts, v, idx.reshape(-1), np.float64), wr.exact(pts, v, idx.reshape(-1), np.float32)
            e32 = float(np.abs(w32.astype(np.float64) - w64)[compare].max()) if compare.any() else 0.0
            bar = 8.0 * max(e32, 2.0 ** -23)
            for n in SIZES:
                w, vis = d.winding(beta, n, visits=True)
                assert np.array_equal(vis, vis_ref[:n]), (scene, set_name, beta, n, np.flatnonzero((vis != vis_ref[:n]).any(axis=1))[:4])
                assert np.array_equal(w.view(np.uint32), d.winding(beta, n).view(np.uint32)), (scene, set_name, beta, n)      # the product kernel's bits
                assert np.isfinite(w).all()
                err = np.abs(w.astype(np.float64) - w64[:n])[compare[:n]]
                if err.size:
                    worst[beta] = max(worst.get(beta, (0.0, 0.0, 0.0))[0], float(err.max())), e32, bar
                    assert err.max() <= bar, (scene, set_name, beta, n, float(err.max()), e32, bar)
        print(scene, set_name, "largest |w - w64|, E32, bar per beta:", {b: "%.3g %.3g %.3g" % t for b, t in worst.items()})
    finally:
        d.free()
    assert c.info().device_bytes == before


# ---- meaning ----------------------------------------------------------------------------------------------------------------------

def test_inside_and_outside_of_a_closed_and_of_a_holed_icosphere(ctxs):
    pts, inside = mr.shell_points(1000, ICO_CENTRE, ICO_RADIUS)
    for drop in (0, 8):
        v, idx, ids, mats = _ico_arrays(2, drop)
        c = ctxs(v, idx, ids, mats)
        tree, m = check_moments(c, (drop,))
        ref = wr.walk(*tree[:2], m, tree[2], pts, 2.0)[1]
        assert ((ref > 0.5) == inside).all(), ("the reference walk on the device's tree", drop, np.flatnonzero((ref > 0.5) != inside)[:4])
        d = Device(c, pts)
        try:
            w = d.winding(2.0)
        finally:
            d.free()
        print("drop %d: smallest w inside %.4f, largest outside %.4f" % (drop, w[inside].min(), w[~inside].max()))
        assert ((w > 0.5) == inside).all(), (drop, np.flatnonzero((w > 0.5) != inside)[:4])
        state = qs.state_of(c)
        got, ww = pt.pointsInside(state, pts, method="winding", return_counts=True)
        assert np.array_equal(got, inside) and np.array_equal(ww.view(np.uint32), w.view(np.uint32))
        # crossing parity along one direction aimed through the hole: right on the closed mesh, wrong on the holed one
        whole = mr.icosphere(2, ICO_CENTRE, ICO_RADIUS)
        hole = whole[0][:, :3].astype(np.float64)[whole[1][:8].astype(np.int64)].mean(axis=(0, 1)) - np.array(ICO_CENTRE)
        aimed = (hole / np.linalg.norm(hole)).astype(np.float32)[None, :]
        parity = pt.pointsInside(state, pts, directions=aimed)
        if drop == 0:
            assert np.array_equal(parity, inside)
        else:
            # an inside point whose ray leaves through the hole counts no crossing, an outside point behind the sphere whose ray
            # enters through a face and leaves through the hole counts one
            wrong = parity != inside
            assert (wrong & inside).any() and (wrong & ~inside).any(), wrong.sum()
            print("parity through the hole: %d inside points called outside, %d outside points called inside, of %d" % ((wrong & inside).sum(), (wrong & ~inside).sum(), len(pts)))


def test_bake_distance_field_signed_by_winding(ctxs):
    v, idx, ids, mats = _ico_arrays(2, 8)
    c = ctxs(v, idx, ids, mats)
    state = qs.state_of(c)
    lo, hi = np.array(ICO_CENTRE) - 1.25 * ICO_RADIUS, np.array(ICO_CENTRE) + 1.25 * ICO_RADIUS
    unsigned = pt.bakeDistanceField(state, (9, 10, 11), bounds=(lo, hi))
    signed = pt.bakeDistanceField(state, (9, 10, 11), bounds=(lo, hi), signed="winding")
    cells = pt.distanceFieldPoints((9, 10, 11), lo, hi)
    r = np.linalg.norm(cells.astype(np.float64) - np.array(ICO_CENTRE), axis=1).reshape(9, 10, 11) / ICO_RADIUS
    assert signed.shape == (9, 10, 11) and np.array_equal(np.abs(signed), unsigned)
    clear = (r < 0.95) | (r > 1.02)
    assert np.array_equal((signed < 0)[clear], (r < 0.95)[clear]) and (r < 0.95).sum() > 50


# ---- edges ------------------------------------------------------------------------------------------------------------------------

def test_one_triangle_two_triangles_and_none(ctxs):
    pts = qs.point_sets("box")["around"][0][:257]
    for name, n_tris in (("one_triangle", 1), ("two_triangles", 2)):
        v, idx, ids, mats = qs.SCENES[name].arrays()
        for kw in ({}, {"variant": 1}):
            c = ctxs(v, idx, ids, mats, **kw)
            tree, m = check_moments(c, (name,))
            assert c.info().n_nodes == 1 and tree[1].tolist() == [[False, n_tris == 1]]
            near = np.concatenate([pts, v[:3, :3] + np.float32(7.0)])
            d = Device(c, near)
            try:
                w, vis = d.winding(np.inf, visits=True)
                assert (vis == [0, n_tris]).all()                      # once, not twice
                want = wr.exact(near, v, idx.reshape(-1))
                assert np.abs(w - want).max() < 8 * max(np.abs(wr.exact(near, v, idx.reshape(-1), np.float32) - want).max(), 2.0 ** -23)
                assert np.abs(w).max() > 0.05
                w, vis = d.winding(2.0, visits=True)
                assert np.array_equal(vis, wr.walk(*tree[:2], m, tree[2], near, 2.0)[0]) and np.isfinite(w).all()
                assert (vis[:, 0] == 1).any() and (vis[:, 1] == n_tris).any()
            finally:
                d.free()
    v, idx, ids, mats = qs.SCENES["empty"].arrays()
    c = ctxs(v, idx, ids, mats)
    d = Device(c, pts)
    try:
        w, vis = d.winding(2.0, visits=True)
        assert not w.view(np.uint32).any() and not vis.any() and winding_info(c) == (0, 0, 0)
    finally:
        d.free()


def test_twenty_thousand_coincident_triangles(ctxs):
    """copies: 20 000 times one triangle, a tree of ~96 levels (more than 64 KiB of LDS lane stack); w is 20 000 times one triangle's"""
    v, idx, ids, mats = qs.SCENES["copies"].arrays()
    c = ctxs(v, idx, ids, mats)
    n = len(idx)
    assert c.info().stack_entries >= 64
    tree, m = check_moments(c)
    pts = qs.point_sets("copies")["around"][0][:257]
    one = wr.records_of_scene(v, idx.reshape(-1)[:3])
    v0, v1, v2 = wr.record_vertices(one)
    t64 = wr.solid_angle(pts.astype(np.float64), v0, v1, v2)
    t32 = wr.solid_angle(pts.astype(np.float32), v0, v1, v2)
    seq = np.zeros(len(pts), np.float32)
    for _ in range(n):
        seq = (seq + t32).astype(np.float32)
    want = n * t64 * (0.25 / np.pi)
    lo, hi = nr.scene_box(v, idx)
    far = np.abs(pts[:, 2].astype(np.float64) - 300.0) >= NEAR_REL * float(np.linalg.norm(hi.astype(np.float64) - lo))      # the plane z = 300
    far &= np.isfinite(want)
    e32 = np.abs(seq.astype(np.float64) * (0.25 / np.pi) - want)[far].max()
    d = Device(c, pts)
    try:
        w, vis = d.winding(np.inf, visits=True)
        assert (vis == [0, n]).all() and np.isfinite(w).all()
        err = np.abs(w.astype(np.float64) - want)[far].max()
        print("copies: largest |w - 20000 w1| %.3g, E32 %.3g, largest |w| %.1f" % (err, e32, np.abs(want[far]).max()))
        assert far.mean() > 0.5 and err <= 8 * max(e32, 2.0 ** -23)
        w, vis = d.winding(2.0, visits=True)
        assert np.array_equal(vis, wr.walk(*tree[:2], m, tree[2], pts, 2.0)[0]) and np.isfinite(w).all()
    finally:
        d.free()


@pytest.mark.parametrize("name", ["flat", "point", "zero_area"] + list(qs.MAGNITUDES))
def test_degenerate_scenes_and_magnitudes_stay_finite_and_decide_as_the_reference(ctxs, name):
    v, idx, ids, mats = qs.SCENES[name].arrays()
    c = ctxs(v, idx, ids, mats)
    tree, m = check_moments(c, (name,))
    sets = qs.point_sets(name)
    pts = np.concatenate([sets[k][0][:200] for k in ("inside", "shell", "features", "around")])
    d = Device(c, pts)
    try:
        for beta in (2.0, np.inf):
            w, vis = d.winding(beta, visits=True)
            assert np.isfinite(w).all(), (name, beta, np.flatnonzero(~np.isfinite(w))[:4])
            assert np.array_equal(vis, wr.walk(*tree[:2], m, tree[2], pts, beta)[0]), (name, beta)
    finally:
        d.free()


def test_bad_points_between_good_ones(scenes):
    c, v, idx = scenes("box")
    pts = nr.point_set("inside", v.reshape(-1), idx.reshape(-1), qs.camera(qs.SCENES["box"]))[:64].copy()
    good = Device(c, pts)
    bad = np.array([[np.nan, 1, 2], [1, np.inf, 2], [1, 2, -np.inf], [np.nan, np.nan, np.nan], [np.inf, 0, np.nan]], np.float32)
    where = 2 * np.arange(len(bad)) + 1                                 # every other lane of the first wave
    mixed = pts.copy()
    mixed[where] = bad
    d = Device(c, mixed)
    try:
        for beta in (2.0, np.inf):
            ref, ref_vis = good.winding(beta, visits=True)
            w, vis = d.winding(beta, visits=True)
            ok = np.ones(64, bool); ok[where] = False
            assert np.isnan(w[where]).all() and not vis[where].any()
            assert np.array_equal(w[ok].view(np.uint32), ref[ok].view(np.uint32)) and np.array_equal(vis[ok], ref_vis[ok])
    finally:
        d.free(); good.free()


# ---- housekeeping -----------------------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits_and_the_render_state_stays(ctxs):
    v, idx, ids, mats = _obj_arrays(BOX)
    c, twin = ctxs(v, idx, ids, mats), ctxs(v, idx, ids, mats)
    pts = nr.point_set("shell", v.reshape(-1), idx.reshape(-1), qs.camera(qs.SCENES["box"]))
    before = c.info().device_bytes
    stats = lambda x: bytes((lambda s: (x.L.pt_get_stats(x.ctx, C.byref(s)), s)[1])(_native.Stats()))
    first = c.render(frames=1)
    st = stats(c)
    d = Device(c, pts)
    try:
        a, b = d.winding(2.0), d.winding(2.0)                            # winding() checks the 0xCD guards
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(d.winding(np.inf).view(np.uint32), d.winding(np.inf).view(np.uint32))
    finally:
        d.free()
    assert stats(c) == st
    assert c.info().device_bytes == before and winding_info(c)[0] == 1
    assert _L().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH
    again, other = c.render(frames=1), twin.render(frames=1)
    for x, y, z in zip(first, again, other):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_refusals_leave_the_context_usable(scenes):
    c, v, idx = scenes("box")
    L, ctx = c.L, c.ctx
    pts = nr.point_set("inside", v.reshape(-1), idx.reshape(-1), qs.camera(qs.SCENES["box"]))[:256]
    d = Device(c, pts)
    err = lambda: (L.pt_last_error(ctx) or b"").decode()
    try:
        want = d.winding(2.0)
        p, o, vv = d.p, d.out, d.visits
        W, T = L.pt_query_winding, L.pt_debug_winding_visits
        refused = {
            "beta below 1": W(ctx, p, 256, 0.999, o), "beta 0": W(ctx, p, 256, 0.0, o), "beta negative": W(ctx, p, 256, -2.0, o),
            "beta NaN": W(ctx, p, 256, float("nan"), o),
            "null points": W(ctx, None, 256, 2.0, o), "null out": W(ctx, p, 256, 2.0, None), "too many": W(ctx, p, 0x80000000, 2.0, o),
            "points not aligned": W(ctx, p + 4, 16, 2.0, o), "out not aligned": W(ctx, p, 16, 2.0, o + 2),
            "out is the points": W(ctx, p, 256, 2.0, p), "out inside the points": W(ctx, p, 256, 2.0, p + 256 * 16 - 4),
            "the points inside out": W(ctx, o + 12, 8, 2.0, o), "null context": W(None, p, 256, 2.0, o),
            "twin: null visits": T(ctx, p, 256, 2.0, o, None), "twin: visits not aligned": T(ctx, p, 16, 2.0, o, vv + 4),
            "twin: visits overlap out": T(ctx, p, 256, 2.0, o, o + 4), "twin: visits are the points": T(ctx, p, 256, 2.0, o, p),
            "twin: beta": T(ctx, p, 256, 0.5, o, vv),
            "info: null": L.pt_get_winding_info(ctx, None), "read: null": L.pt_debug_read_winding(ctx, None, 1 << 20),
            "read: capacity": L.pt_debug_read_winding(ctx, ctx, 8),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert W(ctx, p, 256, 0.5, o) != 0 and err().startswith("pt_query_winding: ") and "beta" in err()
        assert W(ctx, None, 256, 0.5, o) != 0 and "beta" in err()                      # beta comes before the pointers
        assert W(ctx, None, 256, 2.0, o) != 0 and "null argument" in err()
        assert W(ctx, p, 0x80000000, 2.0, o) != 0 and "too many points" in err()
        assert W(ctx, p + 4, 16, 2.0, o) != 0 and "aligned" in err()
        assert W(ctx, p, 256, 2.0, p) != 0 and "overlaps" in err()
        assert T(ctx, p, 256, 2.0, o, None) != 0 and err().startswith("pt_debug_winding_visits: ")
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert W(bare, p, 256, 2.0, o) != 0 and b"no scene" in L.pt_last_error(bare)
            assert W(bare, None, 0, 0.0, None) == 0                                   # no points: nothing to do, nothing to refuse
            info = _native.WindingInfo()
            assert L.pt_get_winding_info(bare, C.byref(info)) == 0 and (info.built, info.n_nodes, info.bytes) == (0, 0, 0)
            assert L.pt_debug_read_winding(bare, p, 1 << 20) != 0
        finally:
            L.pt_destroy(bare)
        assert W(ctx, None, 0, 2.0, None) == 0 and T(ctx, None, 0, 2.0, None, None) == 0
        assert np.array_equal(d.winding(2.0).view(np.uint32), want.view(np.uint32))      # the next valid call
        assert W(ctx, p, 256, float("inf"), o) == 0 and W(ctx, p, 256, 1.0, o) == 0
    finally:
        d.free()


def test_querywinding_numpy_and_torch(scenes, monkeypatch):
    c, v, idx = scenes("diffuse")
    state = qs.state_of(c)
    state._device = 0
    pts = nr.point_set("shell", v.reshape(-1), idx.reshape(-1), qs.camera(qs.SCENES["box"]))
    d = Device(c, pts)
    try:
        want = {beta: d.winding(beta) for beta in (2.0, np.inf)}
    finally:
        d.free()
    got = pt.queryWinding(state, pts)
    assert got.dtype == np.float32 and got.shape == (len(pts),) and np.array_equal(got.view(np.uint32), want[2.0].view(np.uint32))
    four = np.concatenate([pts, np.full((len(pts), 1), 123.0, np.float32)], axis=1)
    assert np.array_equal(pt.queryWinding(state, four.tolist(), beta=float("inf")).view(np.uint32), want[np.inf].view(np.uint32))
    info = pt.getWindingInfo(state)
    assert info == {"built": True, "bytes": 96 * c.info().n_nodes, "n_nodes": c.info().n_nodes}
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    L = _L()
    seen = {}
    real = L.pt_query_winding
    monkeypatch.setattr(L, "pt_query_winding", lambda ctx, p, n, beta, out: seen.update(call=(p, n, beta, out)) or real(ctx, p, n, beta, out))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(four.copy()).to(dev)
    w = pt.queryWinding(state, x, beta=3.0)
    assert seen["call"] == (x.data_ptr(), len(pts), 3.0, w.data_ptr()) and w.device == dev and w.dtype == torch.float32 and w.shape == (len(pts),)
    y = (x * 1.0).contiguous()                       # still in flight on torch's stream when the wrapper is entered
    assert np.array_equal(pt.queryWinding(state, y).cpu().numpy().view(np.uint32), want[2.0].view(np.uint32))
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :3].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.queryWinding(state, bad)
    assert pt.queryWinding(state, x[:0]).shape == (0,)


def test_cli_winding_prints_what_the_wrapper_says(built, scenes, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    c, v, idx = scenes("box")
    state = qs.state_of(c)
    # fp32 values, printed as the doubles they are: the app reads back the same fp32
    queries = [(278.0, 273.0, 280.0, None), (278.0, 273.0, 280.0, float("inf")), (278.0, 273.0, -500.0, 3.0), (float(F(100.1)), 50.0, float(F(300.7)), 1.0), (5000.0, 0.0, 0.0, None)]
    # a finite beta's answer depends on the tree: the app builds with the library's default mode, as the context beside it was
    cmd = [exe, "--obj", BOX, "--build-mode", "2", "--width", "64", "--height", "48", "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for x, y, z, beta in queries:
        cmd += ["--winding", "%r,%r,%r" % (x, y, z) + ("" if beta is None else ",%r" % beta)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"winding"')]
    assert len(lines) == len(queries)
    for (x, y, z, beta), line in zip(queries, lines):
        b = 2.0 if beta is None else beta
        want = pt.queryWinding(state, np.array([[x, y, z]], np.float32), beta=b)[0]
        assert np.array_equal(np.array(line["winding"], np.float32), np.array([x, y, z], np.float32))
        assert line["beta"] == ("inf" if np.isinf(b) else b) and np.float32(line["w"]) == want and line["inside"] == bool(want > 0.5)
    # the room's walls face inwards: inside it the number is near -1 (the front is open), outside near 0; w > 0.5 nowhere
    assert [l["w"] < -0.5 for l in lines] == [True, True, False, True, False] and not any(l["inside"] for l in lines)
    for arg in ("1,2", "1,2,nan", "1,inf,3", "1,2,3,0.5", "1,2,3,nan", "1,2,3,-2"):
        bad = subprocess.run([exe, "--obj", BOX, "--winding", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--winding" in bad.stderr, arg
