"""pt_query_multi on the GPU: every record and count against tests/multihit_ref.py (the oracle's brute-force triangle test, one triangle
at a time) as bits — on the Cornell fixtures and the fp32-node scene at the sizes around a wave and a workgroup, and over the scene
matrix of tests/query_scenes.py —, record 0 against pt_query_closest, the counts against pt_query_any, prefixes, the pruned walk
against the unpruned one, bad rays, guard bytes, scene edits, the render state, the refusals, torch tensors, acgpt_main --pick-all,
and pointsInside / bakeDistanceField(signed=True) on a closed icosphere."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import denoise_ref as dr
import multihit_ref as mr
import query_ref as qr
import query_scenes as qs
import test_gpu_query as gq
import test_gpu_query_scenes as gqs

pytestmark = pytest.mark.gpu

MISS = mr.MISS
GUARD = qs.GUARD
KS = (1, 2, 3, 4, 8)                     # 1, 2, 4, 8: a list of exactly that size; 3: a list of 4 cut at 3
scenes = gq.scenes                       # the two Cornell fixtures and the fp32-node scene, each set up once
ctxs = gqs.ctxs


def _L():
    return _native.hip()


class _Device:
    """rays in a device buffer with room for 8 records a ray and the counts, 64 guard bytes behind each; the C ABI called as a C
    caller would"""

    def __init__(self, state, rays):
        self.state = state
        self.rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        self.n = n = self.rays.shape[0]
        self.bufs = []
        for nbytes in (max(n * 32, 32), n * mr.KEEP * 32 + GUARD, n * 4 + GUARD):
            self.bufs += pt.pathtracer._device_buffers(state, 1, nbytes)
        if n:
            assert _L().pt_copy_to_device(state.context, self.bufs[0], self.rays.ctypes.data, self.rays.nbytes) == 0

    def run(self, k, counts):
        """(records [n, k, 8] u32 or None, counts [n] u32 or None)"""
        L, s, n = _L(), self.state, self.n
        r, h, c = self.bufs
        assert L.pt_device_memset(s.context, h, 0xCD, n * k * 32 + GUARD) == 0 and L.pt_device_memset(s.context, c, 0xCD, n * 4 + GUARD) == 0
        assert L.pt_query_multi(s.context, r, n, k, h if k else None, c if counts else None) == 0, gq._err(s)
        rec = np.zeros((n, k, 8), np.uint32)
        cnt = np.zeros(n + GUARD // 4, np.uint32)
        tail = np.zeros(GUARD // 4, np.uint32)
        if rec.nbytes:
            assert L.pt_copy_to_host(s.context, rec.ctypes.data, h, rec.nbytes) == 0
        assert L.pt_copy_to_host(s.context, tail.ctypes.data, h + n * k * 32, GUARD) == 0
        assert L.pt_copy_to_host(s.context, cnt.ctypes.data, c, cnt.nbytes) == 0
        assert (tail == 0xCDCDCDCD).all(), "written past the end of the hit records"
        assert (cnt[n if counts else 0:] == 0xCDCDCDCD).all(), "written past the end of the counts" if counts else "counts written unasked"
        return (rec if k else None), (cnt[:n].copy() if counts else None)

    def closest_and_any(self):
        L, s, n = _L(), self.state, self.n
        r, h, c = self.bufs
        rec = np.zeros((n, 8), np.uint32); occ = np.zeros(n, np.uint8)
        assert L.pt_query_closest(s.context, r, n, h) == 0 and L.pt_query_any(s.context, r, n, c) == 0, gq._err(s)
        assert L.pt_copy_to_host(s.context, rec.ctypes.data, h, rec.nbytes) == 0 and L.pt_copy_to_host(s.context, occ.ctypes.data, c, occ.nbytes) == 0
        return rec, occ

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _diff(got, ref):
    bad = np.flatnonzero((got != ref).reshape(len(got), -1).any(axis=1))
    return (bad.size, bad[:4], got[bad][:1], got[bad][:1].view(np.float32), ref[bad][:1], ref[bad][:1].view(np.float32))


def _check(state, ref, ks_counted=KS, ks_pruned=KS, rows=slice(None), closest=True):
    """Everything one ray array can be asked, against its Reference: every max_hits with and without counts, count-only, record 0
    against pt_query_closest, the counts against pt_query_any, the prefixes, the pruned walk against the unpruned.  Returns the
    records at 8 and the counts."""
    rays = ref.rays[rows]
    d = _Device(state, rays)
    try:
        _, only = d.run(0, True)
        assert np.array_equal(only, ref.count[rows]), ("count-only", np.flatnonzero(only != ref.count[rows])[:4])
        full = None
        for k in sorted(set(ks_counted) | set(ks_pruned) | {mr.KEEP}, reverse=True):
            want = ref.records(k, rows)
            if k in ks_counted or k == mr.KEEP:
                rec, cnt = d.run(k, True)                                        # the unpruned walk
                assert np.array_equal(rec, want), (k, "with counts") + _diff(rec, want)
                assert np.array_equal(cnt, ref.count[rows]), (k, np.flatnonzero(cnt != ref.count[rows])[:4])
            if k in ks_pruned:
                pruned, none = d.run(k, False)                                   # the walk cut behind the last kept hit
                assert none is None and np.array_equal(pruned, want), (k, "without counts") + _diff(pruned, want)
            if k == mr.KEEP:
                full = rec
            assert np.array_equal(want, full[:, :k])                             # the prefix of the output at 8
        if closest:
            rec, occ = d.closest_and_any()
            assert np.array_equal(full[:, 0], rec), _diff(full[:, 0], rec)
            assert np.array_equal(only > 0, occ != 0)
        return full, only
    finally:
        d.free()


_fixture_refs = {}


def _fixture_reference(oracle, scene, state, obj, name):
    """Reference of ray set `name` of test_gpu_query.py on a Cornell fixture: computed once, shared, never written"""
    key = ("diffuse" if scene == "diffuse" else "box", name)
    if key not in _fixture_refs:
        v = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
        rays = qr.ray_set(name, v, obj.getIndexBuffer(), gq._camera(state))
        _fixture_refs[key] = mr.Reference(oracle, v, obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials(), rays)
    return _fixture_refs[key]


def test_kernel_source_hash_is_the_parents():
    assert _L().pt_kernel_source_hash().decode() == gq.PARENT_KERNEL_HASH
    assert _L().pt_abi_version() == 4


@pytest.mark.parametrize("name", qr.RAY_SETS)
@pytest.mark.parametrize("scene", ["box", "diffuse", "fp32"])
def test_records_and_counts_equal_the_reference(scenes, oracle, scene, name):
    state, obj = scenes(scene)
    ref = _fixture_reference(oracle, scene, state, obj, name)
    if name == "outside":
        assert not ref.count.any()
    else:
        assert (ref.count > 0).mean() >= 0.25 and (ref.count == 0).mean() >= 0.10
    before = pt.getBvhInfo(state).device_bytes
    for n in gq.SIZES:
        _check(state, ref, rows=slice(0, n))
    assert pt.getBvhInfo(state).device_bytes == before


def test_bad_rays_between_good_ones(scenes, oracle):
    state, obj = scenes("box")
    ref = _fixture_reference(oracle, "box", state, obj, "inside")
    good = ref.rays[(ref.count >= 2) & np.isfinite(ref.rays[:, 7])][:64]
    bad, why = qr.bad_rays(good[0])
    assert bad.shape[0] < 32 and good.shape[0] == 64
    mixed = good.copy()
    where = 2 * np.arange(bad.shape[0]) + 1                 # every other lane of the first wave
    mixed[where] = bad
    still_good = np.ones(64, bool); still_good[where] = False
    v = np.asarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    for counts in (True, False):
        d, m = _Device(state, good), _Device(state, mixed)
        try:
            alone, alone_cnt = d.run(4, counts)
            rec, cnt = m.run(4, counts)
            only = m.run(0, True)[1]
        finally:
            d.free(); m.free()
        assert (alone[:, 1, 1] != MISS).all()
        wrong = (rec[where].reshape(-1, 8) != qr.miss_records(4 * where.size)).any(axis=1).reshape(-1, 4).any(axis=1)
        assert not wrong.any(), [why[i] for i in np.flatnonzero(wrong)]
        assert not only[where].any(), [why[i] for i in np.flatnonzero(only[where])]
        assert np.array_equal(rec[still_good], alone[still_good])
        if counts:
            assert not cnt[where].any() and np.array_equal(cnt[still_good], alone_cnt[still_good]) and (alone_cnt >= 2).all()
    whole = mr.Reference(oracle, v, obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials(), mixed)
    _check(state, whole)


def test_two_calls_give_the_same_bytes(scenes, oracle):
    state, obj = scenes("box")
    ref = _fixture_reference(oracle, "box", state, obj, "inside")
    a, b = _check(state, ref, closest=False), _check(state, ref, closest=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the scene matrix ----------------------------------------------------------------------------------------------------------------

def _matrix(c, oracle, name):
    """max_hits 1, 4 and 8 with counts and 8 without, on every set of the scene; set name -> (records at 8, counts)"""
    st = qs.state_of(c)
    before = c.info().device_bytes
    out = {k: _check(st, ref, ks_counted=(1, 4, 8), ks_pruned=(8,)) for k, ref in mr.scene_reference(oracle, name).items()}
    assert c.info().device_bytes == before
    return out


@pytest.mark.parametrize("name,build_mode,tuning", qs.CASES, ids=["%s-mode%s-%s" % (n, m, "default" if t is None else "tuning%d" % t) for n, m, t in qs.CASES])
def test_scene(ctxs, oracle, name, build_mode, tuning):
    c = ctxs(name, build_mode, tuning)
    assert gqs._held(c) == gqs._expected_format(name, tuning)
    assert len(next(iter(qs.ray_sets(name).values()))) == (257 if name in ("sphere", "copies", "copies_lifted") else 1000)
    out = _matrix(c, oracle, name)
    rec = np.concatenate([r for r, _ in out.values()])
    cnt = np.concatenate([n for _, n in out.values()])
    if name == "copies":                                     # 20 000 exact ties: the first 8 by index, and every one counted
        hit = cnt > 0
        assert hit.sum() >= 100 and (cnt[hit] == 20000).all()
        assert (rec[hit][:, :, 1] == np.arange(mr.KEEP)).all() and (rec[hit][:, :, 0] == rec[hit][:, :1, 0]).all()
    if name == "copies_lifted":
        assert (cnt > mr.KEEP).mean() >= 0.25 and np.unique(rec[:, :, 1]).size > 64
    if name in ("one_triangle", "two_triangles"):
        assert cnt.max() == int(name == "two_triangles") + 1 and c.info().n_nodes == 1
    if name == "point":
        assert not cnt.any() and (rec[:, :, 1] == MISS).all()
    if name == "zero_area":
        zero = qs.zero_area_mask(*qs.SCENES[name].arrays()[:2])
        assert not zero[rec[:, :, 1][rec[:, :, 1] != MISS]].any()
    if name in ("box", "sphere", "flat") + tuple(qs.MAGNITUDES):
        assert (cnt > 2).mean() >= 0.05


@pytest.mark.parametrize("tuning", [None, 1])
def test_a_scene_without_triangles(ctxs, oracle, tuning):
    c = ctxs("empty", None, tuning)
    assert c.info().n_tris == 0
    for rec, cnt in _matrix(c, oracle, "empty").values():
        assert np.array_equal(rec.reshape(-1, 8), qr.miss_records(rec.shape[0] * mr.KEEP)) and not cnt.any()


# ---- state and isolation ---------------------------------------------------------------------------------------------------------------

def test_after_scene_edits_equals_a_fresh_scene(gpu_state_factory, oracle):
    state, obj = gpu_state_factory(gq.BOX, width=97, height=61, max_depth=4, spp=8)
    v0 = np.array(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    rays = np.concatenate([qr.ray_set(name, v0, obj.getIndexBuffer(), gq._camera(state))[:500] for name in ("camera", "inside")])
    idx, mats = obj.getIndexBuffer(), obj.getMaterials()
    first = _check(state, mr.Reference(oracle, v0, idx, obj.getMaterialIndices(), mats, rays))
    fresh = []
    try:
        # 1. a refit: everything strictly inside the room moves
        verts = v0.copy()
        lo, hi = qr.scene_box(verts, idx)
        inner = ((verts[:, :3] > lo + 1.0) & (verts[:, :3] < hi - 1.0)).all(axis=1)
        verts[inner, :3] += np.array([13.0, 7.5, -21.0], np.float32)
        assert not pt.updateVertices(state, verts, "refit")["rebuilt"]
        moved = pt.TinyObjWrapper(gq.BOX)
        moved._vertices = verts.reshape(-1).copy()
        fresh.append(gq._fresh_state(state, moved))
        ref = mr.Reference(oracle, verts, idx, obj.getMaterialIndices(), mats, rays)
        held = pt.getBvhInfo(state).device_bytes
        a, b = _check(state, ref), _check(fresh[-1], ref)
        assert pt.getBvhInfo(state).device_bytes == held
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], first[0])
        # 2. new material assignments on top: the ids rotate by one
        ids = ((np.asarray(obj.getMaterialIndices(), np.uint32) + 1) % obj.getNumMaterials()).astype(np.uint32)
        pt.updateMaterials(state, material_ids=ids)
        moved._materialIndices = ids
        fresh.append(gq._fresh_state(state, moved))
        ref = mr.Reference(oracle, verts, idx, ids, mats, rays)
        c, e = _check(state, ref), _check(fresh[-1], ref)
        assert np.array_equal(c[0], e[0]) and np.array_equal(c[1], a[1])
        assert np.array_equal(c[0][:, :, :7], a[0][:, :, :7]) and (c[0][:, :, 7] != a[0][:, :, 7])[a[0][:, :, 1] != MISS].all()
    finally:
        for s in fresh:
            pt.CleanAllTheThings(s)


def test_calls_leave_the_render_state_alone(gpu_state_factory, oracle):
    kw = dict(width=96, height=64, max_depth=6, direct_lighting=True, importance_sampling=True, spp=8)
    state, obj = gpu_state_factory(gq.BOX, **kw)
    twin, _ = gpu_state_factory(gq.BOX, **kw)
    rays = qr.ray_set("inside", obj.getVerticesFloat(), obj.getIndexBuffer(), gq._camera(state))
    ob = pt.OutputBuffer(pt.OutputBufferType.DEVICE, 96, 64, state)
    try:
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 0
            pt.LaunchCurrentFrame(o, s, 1)
        acc, fb, st = pt.readAccumulation(state), ob.getHostPointer().copy(), bytes(pt.getStats(state))
        got = pt.queryRaysMulti(state, rays, max_hits=8, counts=True)
        pt.queryRaysMulti(state, rays, max_hits=2)
        pt.queryRaysMulti(state, rays, max_hits=0, counts=True)
        assert (got["count"] >= 2).mean() >= 0.10
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(ob.getHostPointer(), fb)
        assert bytes(pt.getStats(state)) == st
        for s, o in ((state, ob), (twin, None)):
            s.params.currentFrameIdx = 1
            pt.LaunchCurrentFrame(o, s, 1)
        assert np.array_equal(pt.readAccumulation(state).view(np.uint32), pt.readAccumulation(twin).view(np.uint32))
    finally:
        ob.free()


def test_refusals_leave_the_context_usable(scenes, oracle):
    state, obj = scenes("box")
    ref = _fixture_reference(oracle, "box", state, obj, "camera").part(0, 256)
    L, ctx = _L(), state.context
    d = _Device(state, ref.rays)
    try:
        r, h, c = d.bufs
        refused = {
            "too many": L.pt_query_multi(ctx, r, 0x80000000, 4, h, c),
            "both outputs null": L.pt_query_multi(ctx, r, 256, 0, None, None),
            "hits null with max_hits": L.pt_query_multi(ctx, r, 256, 4, None, c),
            "hits with max_hits 0": L.pt_query_multi(ctx, r, 256, 0, h, c),
            "max_hits 9": L.pt_query_multi(ctx, r, 256, 9, h, c),
            "null rays": L.pt_query_multi(ctx, None, 256, 4, h, c),
            "rays not aligned": L.pt_query_multi(ctx, r + 4, 16, 4, h, c),
            "hits not aligned": L.pt_query_multi(ctx, r, 16, 4, h + 8, c),
            "counts not aligned": L.pt_query_multi(ctx, r, 16, 4, h, c + 2),
            "hits are the rays": L.pt_query_multi(ctx, r, 256, 1, r, c),
            "hits overlap the rays' end": L.pt_query_multi(ctx, r, 32, 8, r + 31 * 32, c),
            "counts inside the rays": L.pt_query_multi(ctx, r, 256, 4, h, r + 100 * 4),
            "counts inside the hits": L.pt_query_multi(ctx, r, 256, 4, h, h + 256 * 4 * 32 - 4),
            "count-only into the rays": L.pt_query_multi(ctx, r, 256, 0, None, r),
            "null context": L.pt_query_multi(None, r, 256, 4, h, c),
        }
        assert all(rc != 0 for rc in refused.values()), refused
        assert L.pt_query_multi(ctx, r, 256, 9, h, c) != 0 and gq._err(state).startswith("pt_query_multi: ") and "max_hits" in gq._err(state)
        assert L.pt_query_multi(ctx, r, 0x80000000, 4, h, c) != 0 and "too many rays" in gq._err(state)
        assert L.pt_query_multi(ctx, r, 256, 4, h, h) != 0 and "overlaps" in gq._err(state)
        bare = C.c_void_p()
        assert L.pt_create(C.byref(bare), 0) == 0
        try:
            assert L.pt_query_multi(bare, r, 256, 4, h, c) != 0 and b"no scene" in L.pt_last_error(bare)
            assert L.pt_query_multi(bare, None, 0, 4, h, None) == 0             # no rays: nothing to do
        finally:
            L.pt_destroy(bare)
        assert L.pt_query_multi(ctx, None, 0, 4, h, None) == 0 and L.pt_query_multi(ctx, None, 0, 0, None, c) == 0
        assert L.pt_query_multi(ctx, r, 16, 8, h, h + 16 * 8 * 32) == 0, gq._err(state)          # the counts right behind the hits (inside the buffer): no overlap
    finally:
        d.free()
    _check(state, ref)                                                          # the next valid calls


# ---- wrappers and CLI ----------------------------------------------------------------------------------------------------------------

def _packed(got, k):
    return np.concatenate([got["t"].view(np.uint32)[..., None], got["prim"][..., None], got["u"].view(np.uint32)[..., None], got["v"].view(np.uint32)[..., None],
                           got["normal"].view(np.uint32), got["material"][..., None]], axis=2)


def test_queryraysmulti_numpy_path(scenes, oracle):
    state, obj = scenes("diffuse")
    ref = _fixture_reference(oracle, "diffuse", state, obj, "inside")
    n = len(ref.rays)
    got = pt.queryRaysMulti(state, ref.rays)                                    # max_hits 4, no counts
    assert set(got) == {"t", "prim", "u", "v", "normal", "material"}
    assert got["t"].shape == (n, 4) and got["normal"].shape == (n, 4, 3) and got["prim"].dtype == np.uint32 and got["t"].dtype == np.float32
    assert np.array_equal(_packed(got, 4), ref.records(4))
    got = pt.queryRaysMulti(state, ref.rays.tolist(), max_hits=8, counts=True)
    assert np.array_equal(_packed(got, 8), ref.records(8)) and got["count"].dtype == np.uint32 and np.array_equal(got["count"], ref.count)
    only = pt.queryRaysMulti(state, ref.rays, max_hits=0, counts=True)
    assert only["t"].shape == (n, 0) and np.array_equal(only["count"], ref.count)
    none = pt.queryRaysMulti(state, np.zeros((0, 8), np.float32), max_hits=3, counts=True)
    assert none["t"].shape == (0, 3) and none["count"].shape == (0,)


def test_torch_tensors_go_in_and_come_out_without_a_copy(scenes, oracle, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    state, obj = scenes("box")
    ref = _fixture_reference(oracle, "box", state, obj, "inside")
    L = _L()
    seen = []
    real = L.pt_query_multi
    monkeypatch.setattr(L, "pt_query_multi", lambda ctx, r, n, k, h, c: seen.append((r, n, k, h, c)) or real(ctx, r, n, k, h, c))
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(ref.rays.copy()).to(dev)
    got = pt.queryRaysMulti(state, x, max_hits=8, counts=True)
    assert seen[-1][0] == x.data_ptr() and seen[-1][1:3] == (len(ref.rays), 8)
    assert seen[-1][3] == got["t"].data_ptr() and seen[-1][4] == got["count"].data_ptr()      # views of what the library wrote
    assert all(v.device == dev for v in got.values())
    assert got["prim"].dtype == torch.int32 and got["count"].dtype == torch.int32 and got["normal"].shape == (len(ref.rays), 8, 3)
    back = {k: v.cpu().numpy() for k, v in got.items()}
    back = {k: (v.view(np.uint32) if v.dtype != np.float32 else v) for k, v in back.items()}
    assert np.array_equal(_packed(back, 8), ref.records(8)) and np.array_equal(back["count"], ref.count)
    y = (x * 1.0).contiguous()                                                  # still in flight on torch's stream when the wrapper is entered
    again = pt.queryRaysMulti(state, y, max_hits=2)
    assert seen[-1][0] == y.data_ptr() and seen[-1][4] is None and "count" not in again
    assert torch.equal(again["t"], got["t"][:, :2]) and torch.equal(again["prim"], got["prim"][:, :2])
    only = pt.queryRaysMulti(state, x, max_hits=0, counts=True)
    assert seen[-1][3] is None and torch.equal(only["count"], got["count"])
    for bad, what in ((x.double(), "float32"), (x.t().contiguous().t(), "contiguous"), (x.cpu(), "the context is on"), (x[:, :6].contiguous(), "expected an")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.queryRaysMulti(state, bad)
    assert pt.queryRaysMulti(state, x[:0], counts=True)["count"].shape == (0,)


def test_cli_pick_all_prints_what_queryraysmulti_says(built, gpu_state_factory, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    w, h = 128, 96
    picks = [(w // 2, h // 2, 4), (0, 0, 4), (40, 30, 8), (90, 30, 1), (64, 20, 2)]
    cmd = [exe, "--obj", gq.BOX, "--width", str(w), "--height", str(h), "--spp-per-launch", "1", "--frames", "1", "--out", str(tmp_path / "f.png")]
    for x, y, k in picks:
        cmd += ["--pick-all", "%d,%d" % (x, y) if k == 4 else "%d,%d,%d" % (x, y, k)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"pick_all"')]
    assert [tuple(l["pick_all"]) for l in lines] == [p[:2] for p in picks]
    state, obj = gpu_state_factory(gq.BOX, width=w, height=h, max_depth=4, spp=1)
    rays = dr.pixel_rays(w, h, *gq._camera(state))[[y * w + x for x, y, _ in picks]]
    got = pt.queryRaysMulti(state, rays, max_hits=8, counts=True)
    names = [l.split()[1] for l in open(os.path.splitext(gq.BOX)[0] + ".mtl") if l.startswith("newmtl")]
    assert got["count"][0] >= 2 and got["count"][1] == 0                         # the centre goes through a block and the back wall, the corner misses
    for i, line in enumerate(lines):
        k = picks[i][2]
        assert line["count"] == int(got["count"][i]) and len(line["hits"]) == min(k, line["count"])
        for j, hit in enumerate(line["hits"]):
            assert hit["prim"] == int(got["prim"][i, j]) and np.float32(hit["t"]) == got["t"][i, j]
            assert hit["material"] == names[int(got["material"][i, j])]
            assert np.array_equal(np.array(hit["normal"], np.float32), got["normal"][i, j])
            assert np.array_equal(np.array(hit["position"], np.float32), rays[i, 0:3] + got["t"][i, j] * rays[i, 3:6])
    for arg, what in (("%d,0" % w, "outside"), ("1,1,9", "k = 1..8"), ("1,1,0", "k = 1..8")):
        bad = subprocess.run([exe, "--obj", gq.BOX, "--width", str(w), "--height", str(h), "--pick-all", arg], capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and what in bad.stderr, (arg, bad.stderr)


# ---- inside and signed distance ------------------------------------------------------------------------------------------------------
CENTRE, RADIUS = (278.0, 274.0, 280.0), 150.0


def test_points_inside_and_the_signed_field(oracle):
    """One closed icosphere alone (subdivision 3, 1 280 triangles)"""
    v, idx = mr.icosphere(3, CENTRE, RADIUS)
    ids, mats = np.zeros(len(idx), np.uint32), qs.box()[3]
    c = qs._Ctx.from_arrays(v, idx, ids, mats)
    try:
        st = qs.state_of(c)
        pts, inside = mr.shell_points(1000, CENTRE, RADIUS)
        got, cnt = pt.pointsInside(st, pts, return_counts=True)
        assert got.dtype == np.bool_ and np.array_equal(got, inside)             # right on every point
        rays, n, m = pt.pathtracer._inside_rays("pointsInside", pts, None)
        want = mr.first_hits(oracle, v, idx, ids, mats, rays)[2].reshape(n, m)
        assert cnt.shape == (1000, 3) and cnt.dtype == np.uint32 and np.array_equal(cnt, want)
        assert np.array_equal(pt.pointsInside(st, pts, directions=[(0, 0, 1)]), (mr.first_hits(oracle, v, idx, ids, mats, pt.pathtracer._inside_rays(
            "pointsInside", pts, [(0, 0, 1)])[0])[2] & 1) != 0)
        # the signed field: negative exactly at the cells closer to the centre than 0.95 R (the grid has none in the shell between)
        res = (5, 7, 9)
        cells = pt.distanceFieldPoints(res, *[[float(x) for x in b] for b in (c.info().scene_lo, c.info().scene_hi)])
        rad = np.linalg.norm(cells.astype(np.float64) - np.array(CENTRE), axis=1)
        named = pt.pointsInside(st, cells)
        assert np.array_equal(named & (rad < 0.95 * RADIUS), rad < 0.95 * RADIUS) and 10 <= (rad < 0.95 * RADIUS).sum() < len(cells)
        assert not named[rad > 1.02 * RADIUS].any()
        plain = pt.bakeDistanceField(st, res)
        signed, prims = pt.bakeDistanceField(st, res, signed=True, return_prims=True)
        assert signed.shape == res and np.array_equal((signed < 0).reshape(-1), named)
        assert np.array_equal((signed < 0).reshape(-1)[rad < 0.95 * RADIUS], np.ones((rad < 0.95 * RADIUS).sum(), bool))
        assert np.array_equal(np.abs(signed).view(np.uint32), plain.view(np.uint32)) and (plain > 0).all()
        assert np.array_equal(pt.bakeDistanceField(st, res, signed=False).view(np.uint32), plain.view(np.uint32)) and (prims != MISS).all()
    finally:
        c.close()
