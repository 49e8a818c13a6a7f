"""The cases of tests/golden/cast_walk.npz: what pt_query_sweep, pt_query_capsule_cast, pt_query_box_cast, pt_query_triangle_cast
(each with its _any form and every mode of its pt_debug_*_visits hook) and pt_query_poses_cast answer on four scenes under both node
formats.  A plain module: the scenes, the inputs (regenerated from fixed seeds, never stored), the device run that the recording script
and tests/test_gpu_cast_walk_parity.py share, and the CPU references for tests/test_cast_walk_host.py.

The fixture holds the library to the commit it was recorded from bit for bit, the visit counts included: the four families walk the
BVH through one policy (csrc/cast_walk.h), and a change to what that policy admits shows in the counts before it shows in a record.

Scenes: the two Cornell fixtures; the single-triangle scene, whose one node names its triangle twice with the second under an empty
box; 20 000 copies of one triangle, the deepest tree of tests/query_scenes.py (~96 levels), for the stack depth.
Inputs: N = 321 casts per family and scene, two workgroups with the second holding one full wave and one lane.  Cast 0 starts in contact
with two triangles that share an edge (t = 0 for both: an exact tie that goes to the lower index; the single-triangle scene has no
second triangle to tie with), then come rows drawn from the family's generator sets and every miss before any traversal of its
bad_cases(), shuffled together.
"""
import os
import types

import numpy as np

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import boxcast_ref as br
import capsule_ref as cr
import poses_ref as pr
import query_scenes as qs
import sweep_ref as sw
import tricast_ref as tc

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cast_walk.npz")
N = 321
SEED = 4242
POOL = 160                   # rows generated per set; N are drawn from all of them
GUARD = 64                   # bytes of 0xCD kept behind every output
DIFFUSE = os.path.join(pt.SCENES, "cornell_box_diffuse.obj")
K_POSE_NO_EARLY, K_POSE_POSE_MAJOR = 1, 2          # csrc/poses.h
POSE_FLAGS = (None, 0, K_POSE_NO_EARLY | K_POSE_POSE_MAJOR)      # None: pt_query_poses_cast itself


def _diffuse():
    obj = pt.TinyObjWrapper(DIFFUSE)
    mats = obj.getMaterials()
    table = (_native.Material * len(mats))(*[_native.Material.from_buffer_copy(m) for m in mats])
    return qs._frozen(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), table)


# name -> (arrays(), build mode): test_gpu_query_scenes.CASES builds the copies with mode 2
SCENES = {"box": (qs.box, None), "diffuse": (_diffuse, None), "one_triangle": (lambda: qs.triangles(1), None), "copies": (qs.copies, 2)}
FORMATS = {"fp16": None, "fp32": 1}          # pt_set_tuning's variant: the default takes the fp16 centre / half-extent nodes on these scenes


class Family:
    def __init__(self, name, ref, floats, words, sets, gen, bad, records, modes):
        self.name, self.ref, self.floats, self.words, self.sets, self.gen, self.bad, self.records, self.modes = name, ref, floats, words, sets, gen, bad, records, modes
        self.call, self.any, self.hook = "pt_query_%s" % name, "pt_query_%s_any" % name, "pt_debug_%s_visits" % name


FAMILIES = {f.name: f for f in [
    Family("sweep", sw, 8, 8, ("aimed", "grazing", "inside", "outside"), sw.sweep_set, sw.bad_sweeps, sw.sweep_records, (None,)),
    Family("capsule_cast", cr, 12, 8, ("aimed", "grazing", "links", "inside", "outside"), cr.cast_set, cr.bad_casts, cr.capsule_records, (0, 1)),
    Family("box_cast", br, 20, 12, ("aimed", "grazing", "links", "overlap", "outside"), br.cast_set, br.bad_casts, br.box_records, (0, 1)),
    Family("triangle_cast", tc, 16, 8, ("aimed", "links", "grazing", "overlap", "outside"), tc.cast_set, tc.bad_casts, tc.cast_records, (None,)),
]}


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def tied_pair(v, idx):
    """(i, j, midpoint): the first two triangles that share two vertex positions and the midpoint of what they share, or (0, None,
    the midpoint of triangle 0's first edge) when there is one triangle"""
    p = v[:, :3][idx.astype(np.int64)].astype(np.float64)
    for i in range(min(len(p), 64)):
        for j in range(i + 1, min(len(p), 64)):
            same = [a for a in p[i] if any((a == b).all() for b in p[j])]
            if len(same) >= 2:
                return i, j, 0.5 * (same[0] + same[1])
    return 0, None, 0.5 * (p[0, 0] + p[0, 1])


def tie_cast(family, v, idx):
    """One cast that starts in contact with both triangles of tied_pair"""
    m = tied_pair(v, idx)[2]
    diag = sw._extent(v, idx.reshape(-1))[3]
    d = np.array([0.3, 1.0, 0.2]) * (0.1 * diag)
    s = 0.01 * diag
    if family == "sweep":
        return sw._pack(m[None], d[None], s, np.inf)[0]
    if family == "capsule_cast":
        return cr.pack(m[None], (m + s * np.array([1.0, 1.4, 0.6]))[None], d[None], s, np.inf)[0]
    if family == "box_cast":
        box = np.zeros(16, np.float32)
        box[0:12] = np.concatenate([np.eye(3), m[:, None]], axis=1).reshape(-1)
        box[12:15] = s
        return br.pack(box[None], d[None], np.inf)[0]
    # a triangle with the midpoint as its centroid, across the shared edge and through both triangles' planes
    tri = m + s * np.array([[-1.0, -1.2, -0.8], [1.1, 0.9, 1.3], [-0.1, 0.3, -0.5]])
    return tc.pack(tri[None], d[None], np.inf)[0]


def casts_of(family, scene):
    """The N casts of a family on a scene, float32 [N, floats], read-only"""
    f = FAMILIES[family]
    v, idx, ids = SCENES[scene][0]()[:3]
    flat = idx.reshape(-1)
    pool = np.concatenate([f.gen(name, v, flat, n=POOL) for name in f.sets])
    bad = f.bad(pool[0])[0]
    rng = np.random.default_rng(SEED + 16 * list(FAMILIES).index(family) + list(SCENES).index(scene))
    rows = pool[np.sort(rng.permutation(pool.shape[0])[:N - 1 - bad.shape[0]])]
    rest = np.concatenate([rows, bad])
    casts = np.ascontiguousarray(np.concatenate([tie_cast(family, v, idx)[None], rest[rng.permutation(rest.shape[0])]]), np.float32)
    assert casts.shape == (N, f.floats)
    assert int((~f.ref.castable(casts)).sum()) == bad.shape[0], (family, scene)
    casts.setflags(write=False)
    return casts


def reference(family, scene, casts=None):
    """The CPU reference's records of casts_of(family, scene), uint32 [N, words]"""
    f = FAMILIES[family]
    v, idx, ids = SCENES[scene][0]()[:3]
    return f.records(casts_of(family, scene) if casts is None else casts, v, idx.reshape(-1), ids)


def pose_inputs():
    """(mesh records [12, 12], poses [5, 12], motions [5, 4]): a cube of 60 units in the Cornell box under five rigid poses, each moving
    at a point of the scene; pose 1 rests on the floor (t = 0), pose 3 has a finite tmax"""
    v, idx = qs.box()[:2]
    mesh = pr.records_of(*pr.mesh("box"))
    assert mesh.shape == (12, 12)
    rng = np.random.default_rng(SEED + 999)
    centre = pr.FREE_LO + rng.random((5, 3)) * (pr.FREE_HI - pr.FREE_LO)
    rot = pr._rotations(rng, 5)
    rot[1] = np.eye(3)
    centre[1, 1] = 29.5
    poses = pr.as_poses(pr._rigid(rot, centre))
    target = sw._targets(rng, v, idx.reshape(-1), 5)[0]
    motions = np.zeros((5, 4), np.float32)
    motions[:, 0:3] = (target - centre) * rng.uniform(0.5, 2.0, (5, 1))
    motions[:, 3] = np.inf
    motions[3, 3] = 0.25
    return mesh, poses, motions


def pose_reference():
    v, idx, ids = qs.box()[:3]
    mesh, poses, motions = pose_inputs()
    return tc.poses_cast(poses, motions, mesh, v, idx.reshape(-1), ids)


# ---- the device run ------------------------------------------------------------------------------------------------------------------
def _L():
    return _native.hip()


class _Device:
    """casts in a device buffer, with buffers for the records, the bytes and the visit counts and a guard behind each; the C ABI
    called as a C caller would"""
    def __init__(self, state, family, casts):
        self.state, self.f, self.n = state, FAMILIES[family], casts.shape[0]
        casts = np.ascontiguousarray(casts, np.float32)
        self.bufs = pt.pathtracer._device_buffers(state, 4, self.n * 4 * max(self.f.floats, self.f.words) + GUARD)
        assert _L().pt_copy_to_device(state.context, self.bufs[0], casts.ctypes.data, casts.nbytes) == 0

    def _err(self):
        return (_L().pt_last_error(self.state.context) or b"").decode()

    def _read(self, ptr, nbytes):
        raw = np.zeros(nbytes + GUARD, np.uint8)
        assert _L().pt_copy_to_host(self.state.context, raw.ctypes.data, ptr, raw.nbytes) == 0
        assert (raw[nbytes:] == 0xCD).all(), "written past the end of the output"
        return raw[:nbytes].copy()

    def _arm(self, ptr, nbytes):
        assert _L().pt_device_memset(self.state.context, ptr, 0xCD, nbytes + GUARD) == 0

    def records(self):
        self._arm(self.bufs[1], self.n * 4 * self.f.words)
        assert getattr(_L(), self.f.call)(self.state.context, self.bufs[0], self.n, self.bufs[1]) == 0, self._err()
        return self._read(self.bufs[1], self.n * 4 * self.f.words).view(np.uint32).reshape(self.n, self.f.words)

    def blocked(self):
        self._arm(self.bufs[2], self.n)
        assert getattr(_L(), self.f.any)(self.state.context, self.bufs[0], self.n, self.bufs[2]) == 0, self._err()
        return self._read(self.bufs[2], self.n)

    def visits(self, mode):
        self._arm(self.bufs[1], self.n * 4 * self.f.words)
        self._arm(self.bufs[3], self.n * 8)
        args = (self.state.context, self.bufs[0], self.n, self.bufs[1], self.bufs[3]) + (() if mode is None else (mode,))
        assert getattr(_L(), self.f.hook)(*args) == 0, self._err()
        return (self._read(self.bufs[1], self.n * 4 * self.f.words).view(np.uint32).reshape(self.n, self.f.words),
                self._read(self.bufs[3], self.n * 8).view(np.uint32).reshape(self.n, 2))

    def free(self):
        pt.pathtracer._free_device_buffers(self.state, self.bufs)


def _poses_cast(state, mesh, poses, motions, flags):
    """pt_query_poses_cast's records as uint32 [P, 8], or the debug hook's with flags"""
    L, P = _L(), poses.shape[0]
    mesh, poses, motions = (np.ascontiguousarray(a, np.float32) for a in (mesh, poses, motions))
    assert L.pt_set_query_mesh(state.context, mesh.ctypes.data, mesh.shape[0]) == 0
    bufs = pt.pathtracer._device_buffers(state, 3, max(poses.nbytes, P * 32) + GUARD)
    try:
        for ptr, a in zip(bufs, (poses, motions)):
            assert L.pt_copy_to_device(state.context, ptr, a.ctypes.data, a.nbytes) == 0
        assert L.pt_device_memset(state.context, bufs[2], 0xCD, P * 32 + GUARD) == 0
        if flags is None:
            assert L.pt_query_poses_cast(state.context, bufs[0], bufs[1], P, bufs[2]) == 0
        else:
            assert L.pt_debug_query_poses_cast(state.context, bufs[0], bufs[1], P, bufs[2], flags) == 0
        raw = np.zeros(P * 32 + GUARD, np.uint8)
        assert L.pt_copy_to_host(state.context, raw.ctypes.data, bufs[2], raw.nbytes) == 0
        assert (raw[P * 32:] == 0xCD).all(), "written past the end of the output"
        return raw[:P * 32].view(np.uint32).reshape(P, 8).copy()
    finally:
        pt.pathtracer._free_device_buffers(state, bufs)


def run_all():
    """key -> array of everything the fixture holds, from the library that is loaded: "<family>/<scene>/<format>/records", ".../any",
    ".../visits<mode>/records", ".../visits<mode>/counts", "poses_cast/<format>/flags<flags>"."""
    out = {}
    for scene, (arrays, build_mode) in SCENES.items():
        v, idx, ids, mats = arrays()
        for fmt, variant in FORMATS.items():
            c = qs._Ctx.from_arrays(v, idx, ids, mats, build_mode=build_mode, variant=variant)
            try:
                state = types.SimpleNamespace(context=c.ctx)
                for family, f in FAMILIES.items():
                    d = _Device(state, family, casts_of(family, scene))
                    try:
                        key = "%s/%s/%s/" % (family, scene, fmt)
                        out[key + "records"] = d.records()
                        out[key + "any"] = d.blocked()
                        for mode in f.modes:
                            rec, counts = d.visits(mode)
                            out[key + "visits%s/records" % ("" if mode is None else mode)] = rec
                            out[key + "visits%s/counts" % ("" if mode is None else mode)] = counts
                    finally:
                        d.free()
                if scene == "box":
                    mesh, poses, motions = pose_inputs()
                    for flags in POSE_FLAGS:
                        out["poses_cast/%s/flags%s" % (fmt, "" if flags is None else flags)] = _poses_cast(state, mesh, poses, motions, flags)
            finally:
                c.close()
    return out


# ---- the file ------------------------------------------------------------------------------------------------------------------------
# The records of one (family, scene) are the same array under every format, call and mode (the recording script refuses to write
# anything else), so the file holds them once: "<family>/<scene>/records".  The bytes and the counts are kept per format and mode.
def pack(got):
    packed = {}
    for key, a in got.items():
        part = key.split("/")
        if part[0] == "poses_cast":
            if "poses_cast/records" in packed:
                assert np.array_equal(packed["poses_cast/records"], a), key
            packed["poses_cast/records"] = a
        elif part[-1] == "records":
            short = "%s/%s/records" % (part[0], part[1])
            if short in packed:
                assert np.array_equal(packed[short], a), key
            packed[short] = a
        else:
            packed[key] = a
    return packed


def expected(golden, key):
    """What the fixture says run_all()'s entry `key` is"""
    part = key.split("/")
    if part[0] == "poses_cast":
        return golden["poses_cast/records"]
    if part[-1] == "records":
        return golden["%s/%s/records" % (part[0], part[1])]
    return golden[key]


def all_keys():
    keys = []
    for scene in SCENES:
        for fmt in FORMATS:
            for family, f in FAMILIES.items():
                key = "%s/%s/%s/" % (family, scene, fmt)
                keys += [key + "records", key + "any"]
                for mode in f.modes:
                    keys += [key + "visits%s/records" % ("" if mode is None else mode), key + "visits%s/counts" % ("" if mode is None else mode)]
            if scene == "box":
                keys += ["poses_cast/%s/flags%s" % (fmt, "" if flags is None else flags) for flags in POSE_FLAGS]
    return keys
