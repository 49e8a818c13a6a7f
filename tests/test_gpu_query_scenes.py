"""pt_query_closest / pt_query_any, pt_ao_points / pt_ao_image and pt_query_nearest on the scenes of tests/query_scenes.py: every builder,
a tree of ~96 levels (more than 64 KiB of LDS lane stack), one-node trees, no triangles, flat, collapsed and zero-area geometry, four
magnitudes, a variant forced onto a node format the queries do not walk, and refits into and out of those states.

Every output is held to a reference that is independent of the library, as bits: the hit records to the oracle's brute force through
query_ref.hit_records, any-hit to the oracle's, the AO counts to ao_ref's rays under the oracle's any-hit, the closest-point records to
nearest_ref's brute force at max_radius = +inf and at each set's finite radius; pt_trace_closest / pt_trace_any on the same rays agree
too, and pt_debug_nearest_visits gives the same records with counts that make sense.  64 bytes of 0xCD behind every output stay.  Each
case asserts what makes it the case — the node format held, depth, n_nodes == 1, the LDS size, zero-area winners — and the shares of
tests/test_query_scenes_host.py on what it compares."""
import ctypes as C

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import ao_ref as ar
import nearest_ref as nr
import query_scenes as qs
import test_gpu_ao as gpu_ao

pytestmark = pytest.mark.gpu

F = np.float32
MISS = qs.MISS
PARENT_KERNEL_HASH = "0ae80f7fe3d9b38b"            # pt_kernel_source_hash() of the parent build
FP16, FP32 = 11, 0                                 # the node formats the queries walk: fp16 centre / half extent, fp32


@pytest.fixture
def ctxs():
    made = []

    def make(name, build_mode=None, tuning=None):
        v, idx, ids, mats = qs.SCENES[name].arrays()
        c = qs._Ctx.from_arrays(v, idx, ids, mats, build_mode=build_mode, variant=tuning)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def _held(c):
    """The node format the scene holds, read off pt_get_bvh_info: device_bytes is the triangle records (48 B), the shade records (16 B)
    and ONE node array, 32 B a node (fp16) or 64 B (fp32).  Only before the first host query, which brings the fp32 nodes."""
    i = c.info()
    nodes = int(i.device_bytes) - 64 * int(i.n_tris)
    assert nodes in (i.half_node_bytes, i.node_bytes), (nodes, i.half_node_bytes, i.node_bytes)
    return FP16 if nodes == i.half_node_bytes else FP32


def _features(c, q):
    """pt_render_features' normal_depth for the view q, float32 [h, w, 4]"""
    w, h = int(q.width), int(q.height)
    bufs = c._alloc((w * h * 16, w * h * 16))
    try:
        assert c.L.pt_render_features(c.ctx, C.byref(q), bufs[0], bufs[1]) == 0, c.err()
        return c._get(bufs[1], w * h * 16).view(np.float32).reshape(h, w, 4)
    finally:
        for p in bufs:
            c.L.pt_device_free(c.ctx, p)


def _diff(got, ref):
    bad = np.flatnonzero((got != ref).any(axis=1))
    return (bad.size, bad[:4], got[bad][:2], got[bad][:2].view(np.float32), ref[bad][:2], ref[bad][:2].view(np.float32))


def _stages(c, name, oracle, bytes_stay=True):
    """The three stages on context c, which holds scene `name`, against the references; returns every output, for comparisons between
    contexts.  bytes_stay: the context holds the array the queries walk, so device_bytes must not move."""
    s = qs.SCENES[name]
    st = qs.state_of(c)
    info = c.info()
    before = info.device_bytes
    out = {}
    ray_ref, near_ref, ao_ref = qs.ray_reference(oracle, name), qs.nearest_reference(name), qs.ao_reference(oracle, name)
    qs.check_shares(name, ray_ref, near_ref, ao_ref)

    for k, (rays, want, occluded) in ray_ref.items():
        d = qs.DeviceRays(st, rays)
        try:
            rec, occ = d.closest(), d.any()
        finally:
            d.free()
        assert np.array_equal(rec, want), (name, k) + _diff(rec, want)
        assert np.isin(occ, (0, 1)).all() and np.array_equal(occ.astype(bool), occluded), (name, k, np.flatnonzero(occ.astype(bool) != occluded)[:4])
        out["rays", k] = (rec, occ)

    P, N, p, vis_want, ao_want = ao_ref
    d = qs.DeviceAO(st, gpu_ao._records(P, N))
    try:
        vis, ao = d.points(len(P), pt.aoSamples(qs.K_AO), qs.ao_args(p))
    finally:
        d.free()
    assert np.array_equal(vis, vis_want), (name, np.flatnonzero(vis != vis_want)[:4], vis[vis != vis_want][:4], vis_want[vis != vis_want][:4])
    assert np.array_equal(ao, ao_want), name
    out["ao"] = (vis, ao)

    for k, (pts, r, want_inf, want_r) in near_ref.items():
        for rad, want in ((np.inf, want_inf), (r, want_r)):
            d = qs.DevicePoints(st, nr.with_radius(pts, rad))
            try:
                rec = d.nearest()
            finally:
                d.free()
            assert np.array_equal(rec, want), (name, k, float(rad)) + _diff(rec, want)
            out["nearest", k, float(rad)] = rec

    # the counting twin, once per scene: the same records, and counts the tree bounds
    pts, r, want_inf, _ = near_ref["around"]
    n = min(len(pts), 257)
    d = qs.DevicePoints(st, nr.with_radius(pts[:n], np.inf))
    vis_buf = pt.pathtracer._device_buffers(st, 1, n * 8)
    try:
        assert c.L.pt_debug_nearest_visits(c.ctx, d.bufs[0], n, d.bufs[1], vis_buf[0]) == 0, c.err()
        rec = np.zeros((n, 8), np.uint32); counts = np.zeros((n, 2), np.uint32)
        assert c.L.pt_copy_to_host(c.ctx, rec.ctypes.data, d.bufs[1], rec.nbytes) == 0
        assert c.L.pt_copy_to_host(c.ctx, counts.ctypes.data, vis_buf[0], counts.nbytes) == 0
    finally:
        pt.pathtracer._free_device_buffers(st, vis_buf)
        d.free()
    assert np.array_equal(rec, want_inf[:n]), (name,) + _diff(rec, want_inf[:n])
    assert (counts[:, 0] <= info.n_nodes).all() and (counts[:, 1] <= info.n_tris).all(), (counts.max(axis=0), info.n_nodes, info.n_tris)
    assert info.n_tris == 0 or (counts[nr.searchable(nr.with_radius(pts[:n], np.inf)), 1] >= 1).all()

    if bytes_stay:
        assert c.info().device_bytes == before
    # the host queries on the same rays (they bring the fp32 nodes: last)
    for k, (rays, want, occluded) in ray_ref.items():
        t, prim, hit = c.trace(np.ascontiguousarray(rays))
        rec = out["rays", k][0]
        assert np.array_equal(t, rec[:, 0]) and np.array_equal(prim, rec[:, 1]) and np.array_equal(hit != 0, occluded), (name, k)
    return out


def _ao_images(c, name, oracle):
    """pt_ao_image at 9 x 7 and 24 x 16 against the same construction from pt_render_features, the camera mapped with the scene"""
    s = qs.SCENES[name]
    p = qs.ao_parameters(name)
    out = {}
    for w, h in ((9, 7), (24, 16)):
        st = qs.state_of(c, s, w, h)
        nd = _features(c, st.params)
        miss = nd[..., 3].reshape(-1) < 0
        assert (~miss).any() and (miss.any() or (w, h) == (9, 7))
        d = qs.DeviceAO(st, nd)
        try:
            vis, ao = d.image(pt.aoSamples(qs.K_AO), qs.ao_args(p, seed=9))
        finally:
            d.free()
        Pi, Ni = ar.image_points(nd, qs.camera(s, w, h), w, h)
        want, want_ao = qs.ao_expected(oracle, name, Pi, Ni, p, seed=9)
        assert np.array_equal(vis, want), (name, w, h, np.flatnonzero(vis != want)[:4])
        assert np.array_equal(ao, want_ao) and (vis[miss] == qs.K_AO).all()
        if (w, h) == (24, 16):
            assert (want[~miss] < qs.K_AO).any() and (want[~miss] > 0).any()
        out[w, h] = (vis, ao)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        for u, v in zip(x, y) if isinstance(x, tuple) else ((x, y),):
            assert np.array_equal(u, v), k


def test_kernel_source_hash_is_the_parents():
    assert _native.hip().pt_kernel_source_hash().decode() == PARENT_KERNEL_HASH


# the node format each case holds: the default variant takes the fp16 nodes unless the scene's geometry is finer than their planes
# (pt_bvh_info.half_area_ratio / half_box_inflation), pt_set_tuning(1) the fp32 nodes.  Asserted, so that the matrix provably walks both.
def _expected_format(name, tuning):
    if tuning is not None:
        return {1: FP32, 7: FP16}[tuning]
    return qs.DEFAULT_FORMAT.get(name, FP16)


@pytest.mark.parametrize("name,build_mode,tuning", qs.CASES, ids=["%s-mode%s-%s" % (n, m, "default" if t is None else "tuning%d" % t) for n, m, t in qs.CASES])
def test_scene(ctxs, oracle, name, build_mode, tuning):
    s = qs.SCENES[name]
    c = ctxs(name, build_mode, tuning)
    info = c.info()
    v, idx = s.arrays()[:2]
    assert info.n_tris == len(idx)
    assert _held(c) == _expected_format(name, tuning), (name, tuning, info.half_area_ratio, info.half_box_inflation)
    # what makes the case the case
    if name == "sphere":
        assert info.n_tris == 20492 and info.max_depth > ctxs("box", build_mode).info().max_depth
    if name in ("copies", "copies_lifted"):
        assert info.n_tris == 20000
    if name == "copies":
        assert info.stack_entries * 1024 > 65536, info.stack_entries           # more LDS than the 64 KiB a kernel gets unasked
        assert info.max_depth < info.stack_entries <= 128
    if name in ("one_triangle", "two_triangles"):
        assert info.n_nodes == 1
    if name == "flat":
        assert info.scene_hi[1] - info.scene_lo[1] < 1e-2 * (info.scene_hi[0] - info.scene_lo[0])      # the per-axis fallback of the fp16 space
    if s.xform is not None:
        S = max(abs(x) for x in list(info.scene_lo) + list(info.scene_hi))
        assert S == pytest.approx(qs.scene_magnitude(name), rel=1e-3, abs=2e-5)           # (the leaf boxes' pad is 1e-5 at least)

    out = _stages(c, name, oracle)
    if s.box_shaped:
        _ao_images(c, name, oracle)

    hits = np.concatenate([out["rays", k][0][:, 1] for k in qs.ray_set_names(name)])
    near = np.concatenate([rec[:, 1] for k, rec in out.items() if k[0] == "nearest"])
    if name == "copies":                                         # 20 000 exact ties: the lowest index
        assert (hits[hits != MISS] == 0).all() and (near[near != MISS] == 0).all() and (near != MISS).sum() > 1000
    if name == "copies_lifted":
        assert np.unique(hits[hits != MISS]).size > 8 and np.unique(near[near != MISS]).size > 8
    if name == "point":
        assert (hits == MISS).all() and (out["ao"][0] == qs.K_AO).all()
        for k, rec in out.items():
            if k[0] == "nearest":
                f = rec[:, 1] != MISS
                assert (rec[f, 1] == 0).all() and (rec[f, 2:4] == 0).all() and (rec[f, 4:7].view(np.float32) == np.float32(qs.POINT)).all()
    if name == "zero_area":
        zero = qs.zero_area_mask(v, idx)
        assert zero[near[near != MISS]].sum() >= 20 and not zero[hits[hits != MISS]].any()


@pytest.mark.parametrize("tuning", [None, 1])
def test_a_scene_without_triangles(ctxs, oracle, tuning):
    c = ctxs("empty", None, tuning)
    info = c.info()
    assert info.n_tris == 0
    before = info.device_bytes
    out = _stages(c, "empty", oracle)
    assert c.info().device_bytes == before
    for k, x in out.items():
        if k[0] == "rays":
            assert np.array_equal(x[0], qs.qr.miss_records(len(x[0]))) and not x[1].any()
        elif k[0] == "nearest":
            assert np.array_equal(x, nr.miss_records(len(x)))
    assert (out["ao"][0] == qs.K_AO).all() and (out["ao"][1] == np.float32(1.0).view(np.uint32)).all()


def test_a_variant_forced_onto_nodes_the_queries_do_not_walk(ctxs, oracle):
    """pt_set_tuning(ctx, 0, 5): the fp16 {lo, hi} nodes, which neither the fp16 nor the fp32 walk of the queries reads — the third
    branch of query_node_format: the fp32 nodes come on the first query, stay, and are released again by a refit."""
    L = _native.hip()
    assert b"fp16 nodes (32 B)" in L.pt_variant_name(5)
    c, twin = ctxs("box", None, 5), ctxs("box", None, 5)
    i0 = c.info()
    assert int(i0.device_bytes) - 64 * int(i0.n_tris) == i0.half_node_bytes               # one 32-byte node array: the {lo, hi} nodes
    first = _stages(c, "box", oracle, bytes_stay=False)
    b1 = c.info().device_bytes
    assert b1 == i0.device_bytes + i0.node_bytes                                          # the fp32 nodes came with the first query
    _same(first, _stages(c, "box", oracle))                                               # ... and the second leaves the bytes alone
    assert c.info().device_bytes == b1
    _ao_images(c, "box", oracle)
    # a render after the queries equals a render of a context that never ran one
    for x, y in zip(c.render(), twin.render()):
        assert np.array_equal(x, y)
    # the refit releases the fp32 nodes (and keeps its index buffer, 12 B a triangle); the next query brings them back for the new vertices
    qs._refit(c, qs.scaled()[0])
    assert c.info().device_bytes == i0.device_bytes + 12 * i0.n_tris
    _stages(c, "scaled", oracle, bytes_stay=False)
    assert c.info().device_bytes == b1 + 12 * i0.n_tris
    _ao_images(c, "scaled", oracle)
    fresh = ctxs("scaled", None, 5)
    for x, y in zip(c.render(xform=qs.SCALED), fresh.render(xform=qs.SCALED)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("target", qs.REFIT_TARGETS)
def test_refit_into_and_out_of(ctxs, oracle, target):
    """The box refitted to the target equals the target built fresh (and the references), in every output of the three stages; refitted
    back it equals itself.  At x1e6 / x1e-6 the scene box the refit records is what nearest_abs_term must follow."""
    c = ctxs("box")
    before = _stages(c, "box", oracle)
    qs._refit(c, qs.SCENES[target].arrays()[0])
    fresh = ctxs(target)
    for a, b in zip((c.info().scene_lo, c.info().scene_hi), (fresh.info().scene_lo, fresh.info().scene_hi)):
        assert list(a) == list(b)
    got = _stages(c, target, oracle)
    _same(got, _stages(fresh, target, oracle))
    if qs.SCENES[target].box_shaped:
        a, b = _ao_images(c, target, oracle), _ao_images(fresh, target, oracle)
        _same(a, b)
    qs._refit(c, qs.box()[0])
    _same(before, _stages(c, "box", oracle))
