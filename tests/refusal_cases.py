"""The refusal matrix of the query entry points: every way a call can be refused before any device work, as plain data.

Shared by tests/test_gpu_refusals.py and tests/golden/make_refusals_golden.py.  A case is a label and the call's arguments; what
it expects is not written here but recorded from a build of the library (tests/golden/query_refusals.json).

Every case runs on a context WITHOUT a scene.  All argument refusals precede "no scene (pt_set_scene first)", so a call whose
arguments pass ends there and nothing is ever launched: device pointers are plain aligned integers that nothing dereferences.
The only real memory is what the host side of a call reads: pt_ao_*'s parameter block and disk pattern, pt_ao_image's pt_params.
"""
import ctypes as C

import numpy as np

N = 64                                     # records per call: every array is at least 64 bytes
SENTINEL = 0                               # pt_debug_list_phases(ctx, 0) is refused: a known last error ahead of every case


class A:
    """A device array of a call: bytes = n * per + plus at the nominal n, its alignment, whether the call needs it."""
    def __init__(self, name, per, align=16, required=True, plus=0):
        self.name, self.per, self.align, self.required, self.plus = name, per, align, required, plus

    def size(self):
        return N * self.per + self.plus


class V:
    """A scalar argument (or a host pointer) and its good value."""
    def __init__(self, name, good):
        self.name, self.good = name, good


class Entry:
    """An entry point: its arguments after the context in ABI order (A, V, or the string "n"), the cases only it has (label ->
    overrides of the good call), and whether it is a posed call (run again on a context that holds a query mesh)."""
    def __init__(self, name, args, own=(), posed=False, key=None):
        self.name, self.args, self.own, self.posed, self.key = name, args, list(own), posed, key or name
        self.arrays = [a for a in args if isinstance(a, A)]

    def good(self):
        g = {"ctx": True, "n": N}
        for k, a in enumerate(self.arrays):
            g[a.name] = 0x100000 * (k + 1)
        for a in self.args:
            if isinstance(a, V):
                g[a.name] = a.good
        return g

    def cases(self):
        """[(label, arguments)] in a fixed order."""
        g, arrs = self.good(), self.arrays
        out = [("all arguments fine", dict(g)), ("null context", dict(g, ctx=None))]
        out.append(("n == 0, null pointers", dict(g, n=0, **{a.name: None for a in arrs})))
        for a in arrs:
            out.append(("null %s" % a.name, dict(g, **{a.name: None})))
        out.append(("n = 0x80000000", dict(g, n=0x80000000)))
        for a in arrs:
            out.append(("%s misaligned" % a.name, dict(g, **{a.name: g[a.name] + (4 if a.align > 1 else 1)})))
        for i, a in enumerate(arrs):
            for b in arrs[i + 1:]:
                small, large = (a, b) if a.size() <= b.size() else (b, a)
                out.append(("%s and %s: the same pointer" % (a.name, b.name), dict(g, **{b.name: g[a.name]})))
                out.append(("%s and %s: a tail overlap" % (a.name, b.name), dict(g, **{b.name: g[a.name] + a.size() - 16})))
                out.append(("%s and %s: one inside the other" % (a.name, b.name), dict(g, **{small.name: g[large.name] + 16})))
        for label, over in self.own:
            out.append((label, dict(g, **over)))
        # one probe per adjacent pair of steps: two faults at once, the earlier step's message is expected
        first = arrs[0]
        out.append(("probe: null context and n == 0", dict(g, ctx=None, n=0)))
        for label, over in [o for o in self.own if "n" not in o[1]][:1]:
            out.append(("probe: n == 0 and %s" % label, dict(g, **dict(over, n=0))))
            out.append(("probe: %s and null %s" % (label, first.name), dict(g, **dict(over, **{first.name: None}))))
        out.append(("probe: null %s and n = 0x80000000" % arrs[-1].name, dict(g, n=0x80000000, **{arrs[-1].name: None})))
        out.append(("probe: n = 0x80000000 and %s misaligned" % first.name, dict(g, n=0x80000000, **{first.name: g[first.name] + 4})))
        if len(arrs) > 1:
            other = arrs[1]
            out.append(("probe: %s misaligned and %s the same pointer" % (first.name, other.name),
                        dict(g, **{first.name: g[first.name] + 4, other.name: g[first.name] + 4})))
        assert len({label for label, _ in out}) == len(out), self.key
        return out


def _records(name, noun, in_bytes, out_bytes, own=()):
    """A product call, its any-hit twin where out_bytes is 1."""
    return Entry(name, [A(noun, in_bytes), "n", A("out", out_bytes, align=16 if out_bytes > 1 else 1)], own)


def _visits(name, noun, in_bytes, out_bytes, extra=(), own=(), out_align=16):
    return Entry(name, [A(noun, in_bytes), "n", A("out", out_bytes, align=out_align), A("visits", 8, align=8)] + list(extra), own)


def _list(name, noun, in_bytes):
    own = [("max_prims above the limit", {"max_prims": 9}), ("prims without max_prims", {"max_prims": 0}), ("max_prims without prims", {"prims": None}),
           ("nothing to write", {"max_prims": 0, "prims": None, "counts": None})]
    return Entry(name, [A(noun, in_bytes), "n", V("max_prims", 2), A("prims", 8, required=False), A("counts", 4, align=4, required=False)], own)


def _hit(name, noun, in_bytes):
    return Entry(name, [A(noun, in_bytes), "n", A("hit", 1, align=1)])


def _twin(name, noun, in_bytes):
    return Entry(name, [A(noun, in_bytes), "n", A("counts", 4, align=4), A("visits", 8, align=8)])


def _lists(name, noun, in_bytes):
    own = [("capacity above memory", {"capacity": 1 << 62}), ("capacity 0 and no prims", {"capacity": 0, "prims": None}),
           ("capacity 0 and prims misaligned", {"capacity": 0, "prims": 0x300004}), ("prims null with a capacity", {"prims": None}),
           ("capacity above memory and offsets misaligned", {"capacity": 1 << 62, "offsets": 0x200004}),
           ("capacity above memory and found on offsets", {"capacity": 1 << 62, "found": 0x200000})]
    return Entry(name, [A(noun, in_bytes), "n", A("offsets", 4, align=4, plus=4), A("prims", 8, align=4), V("capacity", 2 * N), A("found", 4, align=4, required=False)], own)


_FLAGS01 = [("flags above 1", {"flags": 2})]
_MODE01 = [("mode above 1", {"mode": 2})]
_POSE_FLAGS = [("flags above 3", {"flags": 4})]
_MULTI_OWN = [("max_hits above the limit", {"max_hits": 9}), ("hits without max_hits", {"max_hits": 0}), ("max_hits without hits", {"hits": None}),
              ("nothing to write", {"max_hits": 0, "hits": None, "counts": None})]
_K_OWN = [("max_k above the limit", {"max_k": 9}), ("out without max_k", {"max_k": 0}), ("max_k without out", {"out": None}),
          ("nothing to write", {"max_k": 0, "out": None, "counts": None})]
_BETA = [("beta below 1", {"beta": 0.5}), ("beta a NaN", {"beta": float("nan")}), ("beta +inf", {"beta": float("inf")})]

ENTRIES = [
    _records("pt_query_closest", "rays", 32, 32), _records("pt_query_any", "rays", 32, 1),
    Entry("pt_query_multi", [A("rays", 32), "n", V("max_hits", 2), A("hits", 64, required=False), A("counts", 4, align=4, required=False)], _MULTI_OWN),
    _records("pt_query_nearest", "points", 16, 32), _visits("pt_debug_nearest_visits", "points", 16, 32),
    Entry("pt_query_nearest_k", [A("points", 16), "n", V("max_k", 2), A("out", 64, required=False), A("counts", 4, align=4, required=False)], _K_OWN),
    _hit("pt_query_within_any", "points", 16),
    Entry("pt_debug_nearest_k_visits", [A("points", 16), "n", V("max_k", 2), A("out", 64, required=False), A("counts", 4, align=4, required=False), V("hit", None),
                                        A("visits", 8, align=8)], _K_OWN + [("hit with a list", {"hit": 0x500000}), ("hit with a list and n == 0", {"hit": 0x500000, "n": 0}),
                                                                            ("hit with max_k 0 and counts", {"hit": 0x500000, "max_k": 0, "out": None})]),
    Entry("pt_debug_nearest_k_visits", [A("points", 16), "n", V("max_k", 0), V("out", None), V("counts", None), A("hit", 1, align=1), A("visits", 8, align=8)],
          key="pt_debug_nearest_k_visits (hit)"),
    Entry("pt_query_winding", [A("points", 16), "n", V("beta", 2.0), A("out", 4, align=4)], _BETA),
    Entry("pt_debug_winding_visits", [A("points", 16), "n", V("beta", 2.0), A("out", 4, align=4), A("visits", 8, align=8)], _BETA),
    _list("pt_query_overlap", "boxes", 32), _hit("pt_query_overlap_any", "boxes", 32), _twin("pt_debug_overlap_visits", "boxes", 32),
    _list("pt_query_triangles", "tris", 48), _hit("pt_query_triangles_any", "tris", 48), _twin("pt_debug_triangles_visits", "tris", 48),
    _list("pt_query_overlap_oriented", "boxes", 64), _hit("pt_query_overlap_oriented_any", "boxes", 64),
    _twin("pt_debug_overlap_oriented_visits", "boxes", 64), _twin("pt_debug_overlap_oriented_visits_cross", "boxes", 64),
    _lists("pt_query_overlap_lists", "boxes", 32), _lists("pt_query_triangles_lists", "tris", 48), _lists("pt_query_overlap_oriented_lists", "boxes", 64),
    _records("pt_query_segments", "segments", 32, 32), _visits("pt_debug_segments_visits", "segments", 32, 32, [V("flags", 0)], _FLAGS01),
    _records("pt_query_triangle_distance", "tris", 48, 48), _visits("pt_debug_triangle_distance_visits", "tris", 48, 48, [V("flags", 0)], _FLAGS01),
    _records("pt_query_sweep", "sweeps", 32, 32), _records("pt_query_sweep_any", "sweeps", 32, 1), _visits("pt_debug_sweep_visits", "sweeps", 32, 32),
    _records("pt_query_capsule_cast", "casts", 48, 32), _records("pt_query_capsule_cast_any", "casts", 48, 1),
    _visits("pt_debug_capsule_cast_visits", "casts", 48, 32, [V("mode", 0)], _MODE01),
    _records("pt_query_box_cast", "casts", 80, 48), _records("pt_query_box_cast_any", "casts", 80, 1),
    _visits("pt_debug_box_cast_visits", "casts", 80, 48, [V("mode", 0)], _MODE01),
    _records("pt_query_triangle_cast", "casts", 64, 32), _records("pt_query_triangle_cast_any", "casts", 64, 1),
    _visits("pt_debug_triangle_cast_visits", "casts", 64, 32),
    # the posed calls: P * T is judged with the two-triangle mesh of the second context (with one triangle no P passes "too many poses"
    # and fails "too many posed triangles")
    Entry("pt_pose_triangles", [A("poses", 48), "n", A("tris_out", 96)], [("too many posed triangles", {"n": 0x40000000})], posed=True),
    Entry("pt_query_poses_any", [A("poses", 48), "n", A("hit", 1, align=1), A("first", 4, align=4, required=False)],
          [("too many posed triangles", {"n": 0x40000000})], posed=True),
    Entry("pt_query_poses_distance", [A("poses", 48), "n", V("max_radius", 1.0), A("out", 48)], [("too many posed triangles", {"n": 0x40000000})], posed=True),
    Entry("pt_debug_query_poses", [A("poses", 48), "n", V("max_radius", 1.0), A("hit", 1, align=1), A("first", 4, align=4, required=False), V("out", None), V("flags", 0)],
          _POSE_FLAGS + [("too many posed triangles", {"n": 0x40000000}), ("out with hit", {"out": 0x400000}), ("out with first", {"out": 0x400000, "hit": None}),
                         ("out with hit and n == 0", {"out": 0x400000, "n": 0}), ("nothing", {"hit": None, "first": None})], posed=True),
    Entry("pt_debug_query_poses", [A("poses", 48), "n", V("max_radius", 1.0), V("hit", None), V("first", None), A("out", 48), V("flags", 0)],
          _POSE_FLAGS + [("too many posed triangles", {"n": 0x40000000})], posed=True, key="pt_debug_query_poses (distance)"),
    Entry("pt_query_poses_cast", [A("poses", 48), A("motions", 16), "n", A("out", 32)], [("too many posed triangles", {"n": 0x40000000})], posed=True),
    Entry("pt_debug_query_poses_cast", [A("poses", 48), A("motions", 16), "n", A("out", 32), V("flags", 0)],
          _POSE_FLAGS + [("too many posed triangles", {"n": 0x40000000})], posed=True),
]


# ---- ambient occlusion: the parameter block and the disk pattern are host memory the call reads ------------------------------------
def _ao_own():
    return [("null disk", {"disk": None}), ("null ap", {"ap": None}),
            ("samples 0", {"ap": {"samples": 0}}), ("samples 257", {"ap": {"samples": 257, "total_samples": 257}}),
            ("radius 0", {"ap": {"radius": 0.0}}), ("radius +inf", {"ap": {"radius": float("inf")}}), ("radius a NaN", {"ap": {"radius": float("nan")}}),
            ("bias negative", {"ap": {"bias": -1.0}}), ("bias +inf", {"ap": {"bias": float("inf")}}),
            ("total_samples below samples", {"ap": {"total_samples": 1}}), ("reserved set", {"ap": {"reserved1": 1}}),
            ("disk point 1 outside", {"disk": [0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]}), ("disk point 0 a NaN", {"disk": [float("nan"), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]}),
            ("disk point 3 outside, past samples", {"disk": [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0], "ap": {"samples": 3}}),
            ("samples 0 and visible misaligned", {"ap": {"samples": 0}, "visible": 0x200004}),
            ("samples 0 and ao on visible", {"ap": {"samples": 0}, "ao": 0x200000}),
            ("disk point 1 outside and ao on visible", {"disk": [0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0], "ao": 0x200000})]


_AO_GOOD = {"samples": 4, "radius": 1.0, "bias": 0.001, "seed": 7, "accumulate": 0, "total_samples": 4}
_DISK_GOOD = [0.0, 0.0, 0.5, 0.0, 0.0, 0.5, -0.5, -0.5]

ENTRIES += [
    Entry("pt_ao_points", [A("points", 32), "n", V("disk", _DISK_GOOD), V("ap", {}), A("visible", 4, align=4), A("ao", 4, align=4, required=False)], _ao_own()),
    # n is width * height: N = 8 x 8; "n = 0x80000000" is 65536 x 32768
    Entry("pt_ao_image", [V("p", True), A("normal_depth", 16), V("disk", _DISK_GOOD), V("ap", {}), A("visible", 4, align=4), A("ao", 4, align=4, required=False)],
          _ao_own() + [("null p", {"p": None}), ("null p and null disk", {"p": None, "disk": None})]),
]

BY_KEY = {e.key: e for e in ENTRIES}
assert len(BY_KEY) == len(ENTRIES)


def _marshal(entry, args, ctx, keep):
    """The ctypes argument list of a case.  keep: collects the host objects the call reads, alive until it returns."""
    from acgpathtracing_amd import _native
    out = [ctx if args["ctx"] else None]
    for a in entry.args:
        if a == "n":
            out.append(args["n"])
            continue
        v = args[a.name]
        if a.name == "ap" and v is not None:
            fields = dict(_AO_GOOD, **v)
            ap = _native.AoParams(fields["samples"], fields["radius"], fields["bias"], fields["seed"], fields["accumulate"], fields["total_samples"])
            ap.reserved[1] = fields.get("reserved1", 0)
            keep.append(ap)
            v = C.byref(ap)
        elif a.name == "disk" and v is not None:
            disk = np.zeros(2 * _native.AO_MAX_SAMPLES, np.float32)      # as long as the longest pattern the call may read
            disk[:len(v)] = v
            keep.append(disk)
            v = disk.ctypes.data
        elif a.name == "p" and v is not None:
            p = _native.PathTraceParams()
            n = args["n"]
            p.width, p.height = (8, n // 8) if n < 0x80000000 else (65536, 32768)
            keep.append(p)
            v = C.byref(p)
        out.append(v)
    return out


def run_entry(L, entry, ctx, prefix=""):
    """{label: [return code, pt_last_error's text]} of every case of the entry point on the context.  Before each case a call that
    is known to be refused sets the last error, so that a case that must leave it alone shows that text."""
    got = {}
    for label, args in entry.cases():
        assert L.pt_debug_list_phases(ctx, SENTINEL) == 1
        keep = []
        rc = getattr(L, entry.name)(*_marshal(entry, args, ctx, keep))
        got[prefix + label] = [int(rc), L.pt_last_error(ctx if args["ctx"] else None).decode()]
    return got


MESH = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1, 1, 0, 1, 0, 1, 1]], np.float32)      # two triangles: 0x40000000 poses are 2^31 posed triangles


def run_all(L):
    """{entry point: {label: [rc, text]}} on two fresh contexts without a scene; the second holds the two-triangle query mesh."""
    vp = C.c_void_p
    plain, meshed = vp(), vp()
    assert L.pt_create(C.byref(plain), 0) == 0 and L.pt_create(C.byref(meshed), 0) == 0
    try:
        assert L.pt_set_query_mesh(meshed, MESH.ctypes.data, len(MESH)) == 0, L.pt_last_error(meshed)
        got = {}
        for e in ENTRIES:
            got[e.key] = run_entry(L, e, plain)
            if e.posed:
                got[e.key].update(run_entry(L, e, meshed, "with a query mesh: "))
        return got
    finally:
        L.pt_destroy(plain)
        L.pt_destroy(meshed)


# ---- the wrappers' refusals of a tensor, before the library is called ---------------------------------------------------------------
def tensor_messages(pt, torch, state):
    """{label: the PathTracerError's text} of every query function of pt (acgpathtracing_amd.pathtracer) on a tensor it must refuse:
    on the CPU, float64, one column too many, not contiguous — and what a tensor may not come with.  The state's context has no scene:
    a tensor that a lost check let through would be refused there.  Each bad tensor is at least as large as a good one."""
    dev = torch.device("cuda", state._device)
    n = 3

    def bad(width):
        return [("on the CPU", torch.zeros((n, width), dtype=torch.float32)), ("float64", torch.zeros((n, width), dtype=torch.float64, device=dev)),
                ("too wide", torch.zeros((n, width + 1), dtype=torch.float32, device=dev)), ("not contiguous", torch.zeros((n, 2 * width), dtype=torch.float32, device=dev)[:, ::2])]
    poses = torch.zeros((n, 12), dtype=torch.float32, device=dev)
    one = np.ones(3, np.float32)
    calls = [("queryRays", 8, lambda t: pt.queryRays(state, t)), ("queryRays any_hit", 8, lambda t: pt.queryRays(state, t, any_hit=True)),
             ("queryRaysMulti", 8, lambda t: pt.queryRaysMulti(state, t)), ("queryNearest", 4, lambda t: pt.queryNearest(state, t)),
             ("queryWinding", 4, lambda t: pt.queryWinding(state, t)), ("queryNearestK", 4, lambda t: pt.queryNearestK(state, t)),
             ("queryWithinAny", 4, lambda t: pt.queryWithinAny(state, t)), ("queryWithinAny radius", 4, lambda t: pt.queryWithinAny(state, t, radius=1.0)),
             ("querySegments", 8, lambda t: pt.querySegments(state, t)),
             ("queryOverlap", 8, lambda t: pt.queryOverlap(state, t)), ("queryOverlap half_extents", 8, lambda t: pt.queryOverlap(state, t, 1.0)),
             ("queryOverlapAny", 8, lambda t: pt.queryOverlapAny(state, t)), ("queryOverlapLists", 8, lambda t: pt.queryOverlapLists(state, t)),
             ("queryTriangles", 12, lambda t: pt.queryTriangles(state, t)), ("queryTrianglesAny", 12, lambda t: pt.queryTrianglesAny(state, t)),
             ("queryTrianglesLists", 12, lambda t: pt.queryTrianglesLists(state, t)), ("queryTriangleDistance", 12, lambda t: pt.queryTriangleDistance(state, t)),
             ("queryOverlapOriented", 16, lambda t: pt.queryOverlapOriented(state, t)), ("queryOverlapOrientedAny", 16, lambda t: pt.queryOverlapOrientedAny(state, t)),
             ("queryOverlapOrientedLists", 16, lambda t: pt.queryOverlapOrientedLists(state, t)),
             ("querySweep", 8, lambda t: pt.querySweep(state, t)), ("querySweep any_hit", 8, lambda t: pt.querySweep(state, t, any_hit=True)),
             ("querySweep directions", 8, lambda t: pt.querySweep(state, t, directions=one)), ("querySweep radius", 8, lambda t: pt.querySweep(state, t, radius=1.0)),
             ("queryCapsuleCast", 12, lambda t: pt.queryCapsuleCast(state, t)), ("queryCapsuleCast p1", 12, lambda t: pt.queryCapsuleCast(state, t, p1=one)),
             ("queryBoxCast", 20, lambda t: pt.queryBoxCast(state, t)), ("queryBoxCast directions", 20, lambda t: pt.queryBoxCast(state, t, directions=one)),
             ("queryTriangleCast", 16, lambda t: pt.queryTriangleCast(state, t)), ("queryTriangleCast directions", 16, lambda t: pt.queryTriangleCast(state, t, directions=one)),
             ("queryPosesCast motions", 4, lambda t: pt.queryPosesCast(state, poses, t)), ("poseBoxCasts motions", 4, lambda t: pt.poseBoxCasts(state, poses, ((0, 0, 0), (1, 1, 1)), t))]
    got = {}
    for label, width, call in calls:
        for kind, t in bad(width):
            try:
                call(t)
                got["%s, %s" % (label, kind)] = "accepted"
            except pt.PathTracerError as e:
                got["%s, %s" % (label, kind)] = str(e)
    return got


def run_tensor_messages():
    """tensor_messages on a fresh context without a scene"""
    import torch
    from acgpathtracing_amd import pathtracer as pt
    state = pt.PathTracerState()
    pt.createDeviceContext(state, 0)
    try:
        return tensor_messages(pt, torch, state)
    finally:
        pt.CleanAllTheThings(state)


# ---- the fixture's form ------------------------------------------------------------------------------------------------------------
def pack(got):
    """run_all's answers as the fixture holds them: the distinct [return code, text] pairs once, the entry point's own name written
    "{fn}", and per entry point one index per case in cases()' order (the posed calls' second pass behind the first)."""
    answers, packed = [], {}
    for key, per_label in got.items():
        e = BY_KEY[key]
        labels = [label for label, _ in e.cases()]
        labels += ["with a query mesh: " + label for label in labels] if e.posed else []
        assert sorted(labels) == sorted(per_label), key
        row = []
        for label in labels:
            rc, text = per_label[label]
            a = [rc, "{fn}" + text[len(e.name):] if text.startswith(e.name + ":") else text]
            if a not in answers:
                answers.append(a)
            row.append(answers.index(a))
        packed[key] = row
    return {"answers": answers, "cases": packed}


def unpack(fixture):
    """{entry point: {label: [return code, text]}} of a packed fixture"""
    got = {}
    for key, row in fixture["cases"].items():
        e = BY_KEY[key]
        labels = [label for label, _ in e.cases()]
        labels += ["with a query mesh: " + label for label in labels] if e.posed else []
        assert len(labels) == len(row), key
        got[key] = {label: [fixture["answers"][k][0], fixture["answers"][k][1].replace("{fn}", e.name, 1)] for label, k in zip(labels, row)}
    return got


def dump(fixture, fh):
    """a fixture of lists and dicts of rows as JSON, one row per line"""
    import json
    fh.write("{\n")
    for i, (name, table) in enumerate(sorted(fixture.items())):
        if isinstance(table, str):
            body = json.dumps(table)
        else:
            rows = ["%s: %s" % (json.dumps(k), json.dumps(table[k])) for k in sorted(table)] if isinstance(table, dict) else [json.dumps(r) for r in table]
            body = ("{%s}" if isinstance(table, dict) else "[%s]") % ("\n" + ",\n".join(rows) + "\n")
        fh.write("%s: %s%s\n" % (json.dumps(name), body, "," if i + 1 < len(fixture) else ""))
    fh.write("}\n")
