"""A pt_create_multi group held to a plain context, call by call.

include/acgpt.h promises of a group that every setter and update "updates every rank" and that every query and image stage "acts on
rank 0".  Each test here makes one plain context and one group with identical settings (a rehearsal group: every rank on device 0,
ACGPT_REHEARSE_SAME_GPU=1 while it is created), applies the same calls to both and asserts equal bits: the accumulation as uint32, the
resolved 8-bit frame buffer, and radiance_rays, shadow_rays, paths and pixels of pt_get_stats (a group's are sums over its ranks).  A
group's reduce has exactly one non-zero term per pixel, so equality is the contract, and no comparison in this
file knows a tolerance.  Sample chunks are explicit, 1 or 4, on both sides: the automatic choice depends on pixels per rank.

What a plain context computes is held to the CPU oracle by the parity suite; tests/test_group_host.py holds the owner formula of
k_keep_owned to the oracle's partition."""
import ctypes as C
import os

import numpy as np
import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import group_ref as gr
from scene_utils import random_rays

pytestmark = pytest.mark.gpu

BOX = gr.BOX
MIB = 1 << 20
CHUNKS = {2: 4, 3: 1, 5: 4, 16: 1}          # explicit sample chunks per world: both legal values get every kind of test


def _L():
    return _native.hip()


@pytest.fixture
def twins(gpu_state_factory, monkeypatch):
    """make(path, world, **kw) -> (plain, group, obj); everything made is destroyed when the test ends"""
    made = []

    def make(path, world, **kw):
        kw.setdefault("sample_chunks", CHUNKS[world])
        plain, group, obj = gr.make_twins(gpu_state_factory, monkeypatch, path, world, **kw)
        made.extend([plain, group])
        return plain, group, obj

    yield make
    gr.release(*made)
    assert gr.REHEARSE not in os.environ


def _both(plain, group, call, *args):
    """the same setter on both sides; both must accept it"""
    for s in (plain, group):
        assert call(s.context, *args) == 0, gr.error_of(s)


# ---- 1. shapes against worlds --------------------------------------------------------------------------------------------------------

SHAPES = {2: [(100, 52), (17, 13), (9, 5), (1, 1)], 3: [(100, 52), (17, 13), (9, 5), (1, 1)], 5: [(100, 52), (17, 13), (9, 5), (1, 1)],
          16: [(17, 13), (1, 1)]}


@pytest.mark.parametrize("world", [2, 3, 5, 16])
def test_shapes_against_worlds(twins, world):
    """Tiles are 8 x 4 pixels: at 1 x 1 and 9 x 5 most ranks own no pixel (launch_frames_single's per_frame == 0, an empty private buffer,
    a reduce over buffers that are all zero but one), 17 x 13 and 100 x 52 end in partial tiles.  Frames 0 to 2 as three launches, then
    as one batch of three.  Largest shape first: the ranks' private buffers are not regrown for the smaller ones, so pixels a rank owned
    in the larger layout would show in the smaller image if a new sequence did not start from zero."""
    plain, group, _ = twins(BOX, world)
    for w, h in SHAPES[world]:
        what = "world %d, %d x %d" % (world, w, h)
        singles = gr.same_render(plain, group, w, h, 3, 1, what + ", three launches")
        batch = gr.same_render(plain, group, w, h, 3, 3, what + ", one batch")
        assert np.array_equal(batch[0], singles[0]) and np.array_equal(batch[1], singles[1]), what
        assert gr.total(batch[2])[:3] == gr.total(singles[2])[:3], what
        assert all(s[3] == w * h and s[2] == w * h * 8 for s in singles[2]), what
        owners = np.unique(gr.owner_image(w, h, world)).size      # ranks that own a pixel at all
        if (w, h) == (1, 1):
            assert owners == 1
        elif (w, h) == (9, 5):
            assert owners == min(world, 3)          # two tiles in each of two strip rows, dealt from rank 0 and from rank world - 1
        else:
            assert owners == (world if world <= 5 else 6)          # 17 x 13 on 16 ranks: 3 x 4 tiles, ranks 0 to 2 and 13 to 15


# ---- 2. every render row on a group --------------------------------------------------------------------------------------------------

def _sky():
    """31 x 63 texels (rows x columns): the seams of tests/test_gpu_shapes.py's odd map"""
    return np.random.default_rng(5).uniform(0.05, 1.0, size=(31, 63, 3)).astype(np.float32)


@pytest.mark.parametrize("world", [2, 3])
def test_every_render_row(twins, world):
    """Light mode 1, the microfacet model, an environment map, both math modes, every kernel variant pt_set_tuning names and the three
    builders, one after the other on the SAME two contexts: a setting changed twice must reach every rank twice.  96 x 64, two frames in
    one batch per row.  With the map cleared and the modes back, the bits of the first row return."""
    plain, group, obj = twins(BOX, world, width=96, height=64)
    L = _L()
    w, h = 96, 64
    seen = {}

    def row(name):
        seen[name] = gr.same_render(plain, group, w, h, 2, 2, "world %d, row %s" % (world, name))
        return seen[name]

    def env(img):
        for s in (plain, group):
            pt.setEnvironment(s, img)

    first = row("default")
    _both(plain, group, L.pt_set_light_mode, 1)
    row("lights")
    _both(plain, group, L.pt_set_material_model, _native.MATERIALS_MICROFACET)
    row("lights ggx")
    _both(plain, group, L.pt_set_material_model, _native.MATERIALS_REFERENCE)
    _both(plain, group, L.pt_set_light_mode, 0)
    env(_sky())
    row("env")
    _both(plain, group, L.pt_set_light_mode, 1)
    _both(plain, group, L.pt_set_material_model, _native.MATERIALS_MICROFACET)
    row("lights ggx env")
    _both(plain, group, L.pt_set_material_model, _native.MATERIALS_REFERENCE)
    _both(plain, group, L.pt_set_light_mode, 0)
    env(None)
    again = row("default again")
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]) and again[2] == first[2], "the cleared map left something behind"
    # the rows are different estimators: a setter that reached no rank at all would leave them equal
    for a, b in (("default", "lights"), ("lights", "lights ggx"), ("default", "env"), ("lights ggx", "lights ggx env")):
        assert not np.array_equal(seen[a][0], seen[b][0]), (a, b)

    _both(plain, group, L.pt_set_math_mode, _native.MATH_FAST)
    fast = row("fast")
    _both(plain, group, L.pt_set_math_mode, _native.MATH_IEEE)
    ieee = row("ieee")
    assert np.array_equal(ieee[0], first[0]) and not np.array_equal(fast[0], first[0])

    tried = 0
    for v in range(64):
        name = L.pt_variant_name(v)
        if name is None:
            break
        if name.startswith(b"DIAG"):          # timing experiments of the experiments build, never the product's
            continue
        rc = L.pt_set_tuning(plain.context, 0, v)
        rcg = L.pt_set_tuning(group.context, 0, v)
        assert (rc == 0) == (rcg == 0), (v, gr.error_of(plain), gr.error_of(group))
        if rc != 0:                           # does not fit the scene: refused on both sides
            continue
        row("variant %d" % v)
        tried += 1
    assert tried >= 8
    _both(plain, group, L.pt_set_tuning, 0, -1)
    back = row("variant chosen per scene")
    assert np.array_equal(back[0], first[0]) and back[2] == first[2]

    for mode in (1, 2, 0):
        _both(plain, group, L.pt_set_build_mode, mode)
        for s in (plain, group):
            pt.buildTheAccelarationStructure(s, obj)
        row("build mode %d" % mode)


# ---- 3. vertex updates ---------------------------------------------------------------------------------------------------------------

def _update(plain, group, verts, mode, what):
    infos = [pt.updateVertices(s, verts, mode) for s in (plain, group)]
    assert infos[0]["rebuilt"] == infos[1]["rebuilt"], what
    assert np.float32(infos[0]["area_ratio"]).view(np.uint32) == np.float32(infos[1]["area_ratio"]).view(np.uint32), what
    return infos[0]


def _same_queries(plain, group, lo, hi, what):
    """a few hundred fixed rays, points and boxes: the answers of both sides, byte for byte"""
    rng = np.random.default_rng(41)
    rays = random_rays(300, 43, lo=tuple(lo), hi=tuple(hi))
    pts = rng.uniform(lo, hi, size=(300, 3)).astype(np.float32)
    half = rng.uniform(0.0, 40.0, size=(300, 3)).astype(np.float32)
    answers = []
    for s in (plain, group):
        answers.append([pt.queryRays(s, rays), pt.queryNearest(s, pts), pt.queryOverlap(s, pts, half), pt.queryWinding(s, pts)])
    for name, a, b in zip(("pt_query_closest", "pt_query_nearest", "pt_query_overlap", "pt_query_winding"), *answers):
        assert gr.blob(a) == gr.blob(b), "%s: %s" % (what, name)
    hits = answers[0][0]["prim"] != 0xFFFFFFFF          # the inputs are no trivial ones: hits and misses, found points, full and empty boxes
    assert hits.any() and not hits.all() and (answers[0][1]["distance"] >= 0).all()
    assert (answers[0][2]["count"] > 0).any() and (answers[0][2]["count"] == 0).any()
    return answers[0]


@pytest.mark.parametrize("world", [3])
def test_vertex_updates(twins, tmp_path, world):
    """PT_UPDATE_REFIT, PT_UPDATE_REBUILD and PT_UPDATE_AUTO on both sides of PT_UPDATE_AUTO_AREA_RATIO on a 332-triangle mesh (an
    icosphere in the Cornell shell), under light mode 1: the same rebuilt flag and area ratio on both sides, a render after each, and
    after the refit the four queries.  The refit moves a vertex of the lamp, so a rank that kept its old light list shows in its tiles;
    "acts on rank 0" must mean rank 0's updated scene."""
    path = gr.sphere_scene(str(tmp_path / "mesh.obj"))
    plain, group, obj = twins(path, world, width=100, height=52)
    L = _L()
    w, h = 100, 52
    v0 = np.ascontiguousarray(obj.getVerticesFloat(), np.float32).reshape(-1, 4)
    assert obj.getIndexBuffer().size // 3 == 332
    sphere, lamp = gr.object_vertices(path, "s000"), gr.object_vertices(path, "lamp")
    _both(plain, group, L.pt_set_light_mode, 1)
    before = gr.same_render(plain, group, w, h, 2, 1, "before any update")
    lo, hi = v0[:, :3].min(axis=0) - 20.0, v0[:, :3].max(axis=0) + 20.0
    q_before = _same_queries(plain, group, lo, hi, "before any update")

    rng = np.random.default_rng(9)
    v1 = v0.copy()                              # the sphere moved and jittered, one corner of the lamp pulled down and sideways
    v1[sphere, :3] += np.float32([35.0, -20.0, 25.0]) + rng.normal(scale=0.3, size=(len(sphere), 3)).astype(np.float32)
    v1[lamp[0], :3] += np.float32([-60.0, -45.0, 30.0])
    info = _update(plain, group, v1, "refit", "refit")
    assert not info["rebuilt"]
    refit = gr.same_render(plain, group, w, h, 2, 1, "after the refit")
    assert not np.array_equal(refit[0], before[0])
    q_refit = _same_queries(plain, group, lo, hi, "after the refit")
    assert gr.blob(q_refit[0]) != gr.blob(q_before[0]) and gr.blob(q_refit[1]) != gr.blob(q_before[1])

    v2 = v1.copy()
    v2[sphere, :3] = (v2[sphere, :3] - v2[sphere, :3].mean(axis=0)) * np.float32(1.7) + v2[sphere, :3].mean(axis=0)
    info = _update(plain, group, v2, "rebuild", "rebuild")
    assert info["rebuilt"]
    rebuilt = gr.same_render(plain, group, w, h, 2, 2, "after the rebuild")
    assert not np.array_equal(rebuilt[0], refit[0])

    v3 = v2.copy()                              # under the ratio: half a unit of jitter
    v3[:, :3] += rng.uniform(-0.5, 0.5, size=(len(v3), 3)).astype(np.float32)
    info = _update(plain, group, v3, "auto", "auto, small move")
    assert not info["rebuilt"] and info["area_ratio"] <= _native.UPDATE_AUTO_AREA_RATIO
    gr.same_render(plain, group, w, h, 2, 1, "after auto, small move")

    v4 = v3[rng.permutation(len(v3))]           # over it: the vertices scrambled (test_gpu_update.py's construction)
    info = _update(plain, group, v4, "auto", "auto, scrambled")
    assert info["rebuilt"]
    gr.same_render(plain, group, w, h, 2, 1, "after auto, scrambled")
    _same_queries(plain, group, lo, hi, "after auto, scrambled")


# ---- 4. material edits ---------------------------------------------------------------------------------------------------------------

def _copy_mats(mats):
    return [_native.Material.from_buffer_copy(m) for m in mats]


def _emits(m):
    return m.emission.x + m.emission.y + m.emission.z > 0


@pytest.mark.parametrize("world", [3])
def test_material_edits(twins, world):
    """pt_update_materials under light mode 1: a diffuse wall made emissive, the lamp switched off, the ids of half the triangles
    reassigned: each edit changes the light list of every rank.  A render after each; then pt_render_features on both."""
    plain, group, obj = twins(BOX, world, width=100, height=52)
    L = _L()
    w, h = 100, 52
    _both(plain, group, L.pt_set_light_mode, 1)
    mats = _copy_mats(obj.getMaterials())
    ids = np.ascontiguousarray(obj.getMaterialIndices(), np.uint32)
    used = np.bincount(ids, minlength=len(mats))
    lamp = next(i for i, m in enumerate(mats) if _emits(m))
    wall = max((i for i, m in enumerate(mats) if m.bsdfType == pt.BSDF_DIFFUSE and not _emits(m)), key=lambda i: used[i])
    assert used[wall] > 0 and used[lamp] > 0
    images = [gr.same_render(plain, group, w, h, 2, 1, "before any edit")]

    def edit(what, materials=None, material_ids=None):
        for s in (plain, group):
            pt.updateMaterials(s, materials=materials, material_ids=material_ids)
        images.append(gr.same_render(plain, group, w, h, 2, 1, what))
        assert not np.array_equal(images[-1][0], images[-2][0]), what

    m1 = _copy_mats(mats)
    m1[wall].emission = _native.Float3(2.0, 1.5, 1.0)
    edit("a wall made emissive", materials=m1)
    m2 = _copy_mats(m1)
    m2[lamp].emission = _native.Float3(0.0, 0.0, 0.0)
    edit("the lamp switched off", materials=m2)
    ids3 = ids.copy()
    ids3[::2] = (ids3[::2] + 1) % len(mats)
    edit("half the ids reassigned", material_ids=ids3)

    feats = [pt.renderFeatures(s) for s in (plain, group)]
    for s in (plain, group):          # renderFeatures reads the state's own params: the setup's 100 x 52 camera
        assert (int(s.params.width), int(s.params.height)) == (w, h)
    for a, b in zip(*feats):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    prims = feats[0][0][..., 3].view(np.uint32)
    assert np.unique(prims[prims != 0xFFFFFFFF]).size > 8          # the box is in view


# ---- 5. scratch limit and batches ----------------------------------------------------------------------------------------------------

def _frames_per_launch(world, w, h, limit):
    """launch_frames_single's arithmetic: a rank holds num_samples = rows * cols * 32 pixel slots, rows = ceil(h / 4) strips of
    cols = ceil(w / (8 world)) tiles each; one float4 (16 bytes) per slot and sub-frame has to fit the limit"""
    per_frame = -(-h // 4) * -(-w // (8 * world)) * 32 * 16
    return max(1, limit // per_frame)


@pytest.mark.parametrize("world", [2, 3])
def test_scratch_limit_cuts_a_batch(twins, world):
    """pt_set_scratch_limit at its 1 MiB minimum and a batch of 7 frames at 328 x 204 (51 strip rows).  A rank's slots times 16 bytes:
      plain      41 tiles per strip: 41 * 51 * 32 * 16 = 1 070 592 B > 1 048 576: one frame per launch, 7 launches
      2 ranks    21 tiles per strip: 21 * 51 * 32 * 16 =   548 352 B: one frame per launch, 7 launches per rank
      3 ranks    14 tiles per strip: 14 * 51 * 32 * 16 =   365 568 B: two frames per launch, launches of 2, 2, 2 and 1 per rank
    The result equals 7 single launches, and what the limit's default gives."""
    w, h = 328, 204
    assert _frames_per_launch(1, w, h, MIB) == 1 and _frames_per_launch(2, w, h, MIB) == 1 and _frames_per_launch(3, w, h, MIB) == 2
    assert _frames_per_launch(world, w, h, MIB) < 7 and _frames_per_launch(world, w, h, 1 << 30) >= 7
    plain, group, _ = twins(BOX, world, width=w, height=h, spp=4)
    uncut = gr.same_render(plain, group, w, h, 7, 7, "world %d, the default limit" % world)
    _both(plain, group, _L().pt_set_scratch_limit, MIB)
    cut = gr.same_render(plain, group, w, h, 7, 7, "world %d, a batch of 7 under 1 MiB" % world)
    singles = gr.same_render(plain, group, w, h, 7, 1, "world %d, 7 single launches" % world)
    for other in (uncut, singles):
        assert np.array_equal(cut[0], other[0]) and np.array_equal(cut[1], other[1])
        assert gr.total(cut[2])[:3] == gr.total(other[2])[:3]
    assert gr.total(cut[2])[2] == w * h * 4 * 7


# ---- 6. restored accumulation: k_keep_owned ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3, 5, 16])
def test_restored_accumulation(twins, world):
    """A caller's buffer with a distinct, finite, strictly positive value per pixel and channel, one frame at currentFrameIdx = 3, on
    fresh contexts: every rank copies the buffer and keeps the pixels k_keep_owned calls its own.  A pixel kept by two ranks comes out
    with its prior doubled, a pixel kept by none loses it."""
    for w, h in ((9, 5), (17, 13), (100, 52)):
        plain, group, _ = twins(BOX, world, width=w, height=h)
        prior = gr.prior_image(w, h)
        want = gr.render(plain, w, h, 1, frame0=3, prior=prior)
        got = gr.render(group, w, h, 1, frame0=3, prior=prior)
        gr.assert_same(got, want, "world %d, %d x %d restored at frame 3" % (world, w, h))
        # the prior carries weight 3/4 at frame 3 and is positive everywhere: a pixel that lost it shows, whichever pixel it is
        empty = gr.render(plain, w, h, 1, frame0=3)
        assert np.all(np.any(want[0][..., :3] != empty[0][..., :3], axis=-1))
        gr.release(plain, group)


# ---- 7. continuation logic -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [3])
def test_continuation_and_reseeding(twins, world):
    """launch_frames_multi continues the ranks' private buffers only on the straight continuation of its last launch (the same buffer,
    the expected frame index, the same shape); anything else starts from the caller's buffer (frame > 0) or from zero (frame 0).
    (The header does not promise that a buffer rewritten in place and resubmitted with the expected frame index is picked up; the
    code continues from its private buffers there, and this test stays away from it.)"""
    plain, group, _ = twins(BOX, world, width=96, height=64)
    w, h = 96, 64
    a = gr.TwinImage(plain, group, w, h)
    b = gr.TwinImage(plain, group, w, h)
    t = gr.TwinImage(plain, group, h, w)
    try:
        # frames 0, 1 and 2
        for f in range(3):
            a.launch(f)
        three = a.check("frames 0 to 2")
        # restart at frame 0 into the same buffer
        a.launch(0)
        s0 = a.check("restart, frame 0")
        a.launch(1)
        s1 = a.check("restart, frame 1")
        assert not np.array_equal(s1[0], three[0])
        # frame 1 again, from a second buffer that holds the state after frame 0
        b.put(s0[0])
        b.launch(1)
        again = b.check("frame 1 from a copy of the state after frame 0")
        assert np.array_equal(again[0], s1[0])
        # the expected frame index (2, after frame 1 into b) in ANOTHER buffer, which holds something else: re-seeded from that buffer
        prior = gr.prior_image(w, h)
        a.put(prior)
        a.launch(2)
        seeded = a.check("frame 2 from another buffer")
        b.launch(2)
        cont = b.check("frame 2 in the buffer of frame 1")
        assert not np.array_equal(seeded[0], cont[0])
        # back in the first buffer (b's launch came last: seeded from what the reduce left in a, the same values), then that buffer
        # overwritten by the caller and a frame index that is not the continuation (4 would be)
        a.launch(3)
        a.check("frame 3 in the first buffer")
        a.put(prior * np.float32(2.0))
        a.launch(5)
        a.check("frame 5 after the caller overwrote the buffer")
        a.launch(6)
        a.check("frame 6 continues")
        # another shape and back, each from frame 0
        t.launch(0); t.launch(1)
        t.check("64 x 96 after 96 x 64")
        a.launch(0); a.launch(1)
        back = a.check("96 x 64 again")
        assert np.array_equal(back[0], s1[0]) and np.array_equal(back[1], s1[1])
    finally:
        a.free(); b.free(); t.free()


# ---- 8. refusals on a group ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [3])
def test_refusals_leave_every_rank_as_it_was(twins, world):
    """Each call is refused with a message that names the reason, and a render afterwards still equals the plain context's."""
    plain, group, obj = twins(BOX, world, width=96, height=64)
    L = _L()
    w, h = 96, 64
    want = gr.render(plain, w, h, 2, 2)
    verts = np.ascontiguousarray(obj.getVerticesFloat(), np.float32)
    ids = np.ascontiguousarray(obj.getMaterialIndices(), np.uint32)
    mats = obj.getMaterials()
    bad_ids = ids.copy()
    bad_ids[len(ids) // 2] = len(mats)
    info = _native.UpdateInfo()

    def still_equal(what):
        gr.assert_same(gr.render(group, w, h, 2, 2), want, "world %d, after %s" % (world, what))

    assert L.pt_set_partition(group.context, 1, world) != 0 and b"partitions the image itself" in gr.error_of(group)
    still_equal("pt_set_partition")
    refusals = [
        ("pt_set_scratch_limit", lambda s: L.pt_set_scratch_limit(s.context, MIB - 1), b"at least 1 MiB"),
        ("pt_set_tuning", lambda s: L.pt_set_tuning(s.context, 0, 63), b"unknown kernel variant"),
        ("pt_update_vertices", lambda s: L.pt_update_vertices(s.context, verts.ctypes.data, verts.size // 4 - 1, _native.UPDATE_REFIT, C.byref(info)),
         b"vertices, the scene has"),
        ("pt_update_materials", lambda s: L.pt_update_materials(s.context, C.addressof(mats), len(mats), bad_ids.ctypes.data, bad_ids.size, None),
         b"material index out of range"),
    ]
    assert L.pt_variant_name(63) is None
    for name, call, reason in refusals:
        for s in (plain, group):
            handle = L.pt_scene_handle(s.context)
            assert call(s) != 0, name
            assert reason in gr.error_of(s), (name, gr.error_of(s))
            assert L.pt_scene_handle(s.context) == handle, name
        still_equal(name)
    # the microfacet model without light mode 1: accepted by the setter, refused by the launch, the buffers left as they were
    _both(plain, group, L.pt_set_material_model, _native.MATERIALS_MICROFACET)
    prior = gr.prior_image(w, h)
    for s in (plain, group):
        img = gr.Image(s, w, h, prior)
        try:
            assert img.launch(0, 2, refused=True) != 0 and b"light mode 1" in gr.error_of(s)
            assert np.array_equal(img.read()[0], prior.view(np.uint32))
        finally:
            img.free()
    _both(plain, group, L.pt_set_material_model, _native.MATERIALS_REFERENCE)
    still_equal("the refused launch")
    gr.assert_same(gr.render(plain, w, h, 2, 2), want, "the plain context after its refusals")
