"""What the query wrappers of pathtracer.py send to the library, traced with a stub in the library's place (no GPU, no build).

Shared by tests/test_query_transport_host.py and tests/golden/make_transport_golden.py.  Stub stands in for _native.hip():
pt_device_malloc hands out numbered fake pointers and remembers their sizes, the copies and the query symbols record themselves and
return 0, downloads leave the host array as it is (zeros).  CASES is every public query function with NumPy input at n = 0, 1 and 5
and every option that changes the call.
"""
import ctypes as C

import numpy as np

BASE, STRIDE = 0x700000000000, 1 << 32      # fake device pointers: allocation k starts at BASE + k * STRIDE
MESH_TRIS = 3                               # what the stub's pt_get_query_mesh reports

# per query symbol: its arguments after the context (p: device pointer, n: the count, s: scalar, h: host pointer) and the bytes the call
# may touch behind each device pointer, from n and the scalars
_REC = {"pt_query_closest": (32, 32), "pt_query_any": (32, 1), "pt_query_nearest": (16, 32), "pt_query_within_any": (16, 1), "pt_query_segments": (32, 32),
        "pt_query_triangle_distance": (48, 48), "pt_query_sweep": (32, 32), "pt_query_sweep_any": (32, 1), "pt_query_capsule_cast": (48, 32),
        "pt_query_capsule_cast_any": (48, 1), "pt_query_box_cast": (80, 48), "pt_query_box_cast_any": (80, 1), "pt_query_triangle_cast": (64, 32),
        "pt_query_triangle_cast_any": (64, 1), "pt_query_overlap_any": (32, 1), "pt_query_triangles_any": (48, 1), "pt_query_overlap_oriented_any": (64, 1)}
SYMBOLS = {name: ("pnp", lambda n, a=a, b=b: (a * n, b * n)) for name, (a, b) in _REC.items()}
SYMBOLS.update({
    "pt_query_multi": ("pnspp", lambda n, k: (32 * n, 32 * n * k, 4 * n)),
    "pt_query_nearest_k": ("pnspp", lambda n, k: (16 * n, 32 * n * k, 4 * n)),
    "pt_query_winding": ("pnsp", lambda n, beta: (16 * n, 4 * n)),
    "pt_query_overlap": ("pnspp", lambda n, k: (32 * n, 4 * n * k, 4 * n)),
    "pt_query_triangles": ("pnspp", lambda n, k: (48 * n, 4 * n * k, 4 * n)),
    "pt_query_overlap_oriented": ("pnspp", lambda n, k: (64 * n, 4 * n * k, 4 * n)),
    "pt_list_offsets": ("pnph", lambda n: (4 * n, 4 * (n + 1))),
    "pt_query_overlap_lists": ("pnppsp", lambda n, cap: (32 * n, 4 * (n + 1), 4 * cap, 4 * n)),
    "pt_query_triangles_lists": ("pnppsp", lambda n, cap: (48 * n, 4 * (n + 1), 4 * cap, 4 * n)),
    "pt_query_overlap_oriented_lists": ("pnppsp", lambda n, cap: (64 * n, 4 * (n + 1), 4 * cap, 4 * n)),
    "pt_pose_boxes": ("pnhp", lambda n: (48 * n, 64 * n)),
    "pt_pose_triangles": ("pnp", lambda n: (48 * n, 48 * n * MESH_TRIS)),
    "pt_query_poses_any": ("pnpp", lambda n: (48 * n, n, 4 * n)),
    "pt_query_poses_distance": ("pnsp", lambda n, r: (48 * n, 48 * n)),
    "pt_query_poses_cast": ("ppnp", lambda n: (48 * n, 16 * n, 32 * n)),
})


class Stub:
    """fail_at: the index (among the calls that can fail: everything but pt_device_free and pt_last_error) of the one call that
    returns 1.  total: what pt_list_offsets reports as the lists' total, from n."""
    def __init__(self, fail_at=None, total=lambda n: 2 * n + 1):
        self.fail_at, self.total = fail_at, total
        self.events, self.sizes, self.freed, self.errors, self.calls = [], [], [], [], 0

    def _fails(self):
        self.calls += 1
        return self.calls - 1 == self.fail_at

    def _inside(self, ptr, nbytes, what):
        k, off = divmod(int(ptr) - BASE, STRIDE)
        if not (0 <= k < len(self.sizes)) or k in self.freed:
            self.errors.append("%s: %#x is not a live allocation" % (what, ptr))
        elif off + nbytes > self.sizes[k]:
            self.errors.append("%s: %d bytes at offset %d of an allocation of %d" % (what, nbytes, off, self.sizes[k]))

    def pt_device_malloc(self, ctx, out, nbytes):
        if self._fails():
            return 1
        if nbytes <= 0:
            self.errors.append("an allocation of %d bytes" % nbytes)
        out._obj.value = BASE + len(self.sizes) * STRIDE
        self.sizes.append(int(nbytes))
        return 0

    def pt_device_free(self, ctx, ptr):
        k, off = divmod(int(ptr) - BASE, STRIDE)
        if off or not (0 <= k < len(self.sizes)) or k in self.freed:
            self.errors.append("pt_device_free of %#x: not a live allocation" % ptr)
        self.freed.append(k)
        return 0

    def pt_last_error(self, ctx):
        return b"the stub said no"

    def pt_copy_to_device(self, ctx, dst, src, nbytes):
        if self._fails():
            return 1
        self._inside(dst, nbytes, "pt_copy_to_device")
        self.events.append({"symbol": "pt_copy_to_device", "bytes": int(nbytes)})
        return 0

    def pt_copy_to_host(self, ctx, dst, src, nbytes):
        if self._fails():
            return 1
        self._inside(src, nbytes, "pt_copy_to_host")
        self.events.append({"symbol": "pt_copy_to_host", "bytes": int(nbytes)})
        return 0

    def pt_get_query_mesh(self, ctx, ntris, nbytes):
        if self._fails():
            return 1
        ntris._obj.value, nbytes._obj.value = MESH_TRIS, 48 * MESH_TRIS
        return 0

    def __getattr__(self, name):
        if name not in SYMBOLS:
            raise AttributeError(name)
        sig, touched = SYMBOLS[name]

        def call(ctx, *args):
            assert len(args) == len(sig), (name, args)
            if self._fails():
                return 1
            n = int(args[sig.index("n")])
            scalars = [a for a, kind in zip(args, sig) if kind == "s"]
            pointers = [a for a, kind in zip(args, sig) if kind == "p"]
            for p, nbytes in zip(pointers, touched(n, *scalars)):
                if p is not None:
                    self._inside(p, nbytes, name)
            if name == "pt_list_offsets" and args[3] is not None:
                args[3]._obj.value = self.total(n)
            self.events.append({"symbol": name, "n": n, "scalars": [repr(float(s)) if isinstance(s, float) else int(s) for s in scalars],
                                "null": [p is None for p in pointers]})
            return 0
        return call

    def all_freed(self):
        return sorted(self.freed) == list(range(len(self.sizes))) and not self.errors


def describe(x):
    """keys, dtypes and shapes of what a query function returns"""
    if isinstance(x, dict):
        return {k: describe(v) for k, v in x.items()}
    if isinstance(x, tuple):
        return [describe(v) for v in x]
    return {"dtype": str(x.dtype), "shape": list(x.shape)}


def trace(events):
    """The events as the fixture holds them: consecutive downloads in a canonical order (which of two outputs comes back first is not
    observable), everything else in the order of the calls."""
    out, run = [], []
    for e in events + [None]:
        if e is not None and e["symbol"] == "pt_copy_to_host":
            run.append(e)
            continue
        out += sorted(run, key=lambda d: d["bytes"])
        run = []
        if e is not None:
            out.append(e)
    return out


class State:
    """what the wrappers read of a PathTracerState"""
    context = C.c_void_p(1)
    _device = 0


def _rng(n, *shape):
    return np.random.default_rng(7 + n).uniform(-1.0, 1.0, (n,) + shape).astype(np.float32)


def _rot(n):
    return np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3)).copy()


def _poses(n):
    p = np.zeros((n, 3, 4), np.float32)
    p[:, :, :3] = np.eye(3)
    p[:, :, 3] = _rng(n, 3)
    return p


_VERTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
_IDX = np.array([[0, 1, 2], [0, 1, 3]], np.int32)


def cases(pt):
    """[(label, f(n) -> the function's result)] on the module pt (acgpathtracing_amd.pathtracer) and a State."""
    s = State()
    inf = float("inf")

    def obox(n):
        return pt.orientedBoxes(_rng(n, 3), 0.5, _rot(n))

    def box_casts(n):
        c = np.zeros((n, 20), np.float32)
        c[:, :16], c[:, 16:19], c[:, 19] = obox(n), 1.0, 2.0
        return c
    return [
        ("queryRays", lambda n: pt.queryRays(s, _rng(n, 8))),
        ("queryRays any_hit", lambda n: pt.queryRays(s, _rng(n, 8), any_hit=True)),
        ("queryRaysMulti", lambda n: pt.queryRaysMulti(s, _rng(n, 8))),
        ("queryRaysMulti max_hits=2 counts", lambda n: pt.queryRaysMulti(s, _rng(n, 8), max_hits=2, counts=True)),
        ("queryRaysMulti max_hits=0 counts", lambda n: pt.queryRaysMulti(s, _rng(n, 8), max_hits=0, counts=True)),
        ("pointsInside", lambda n: pt.pointsInside(s, _rng(n, 3))),
        ("pointsInside return_counts", lambda n: pt.pointsInside(s, _rng(n, 3), return_counts=True)),
        ("pointsInside winding", lambda n: pt.pointsInside(s, _rng(n, 3), method="winding", return_counts=True)),
        ("queryNearest (n, 3)", lambda n: pt.queryNearest(s, _rng(n, 3), max_radius=2.0)),
        ("queryNearest (n, 4)", lambda n: pt.queryNearest(s, np.abs(_rng(n, 4)))),
        ("bakeDistanceField", lambda n: pt.bakeDistanceField(s, (1, 1, n), bounds=((0, 0, 0), (1, 1, 1)), return_prims=True) if n else pt.queryNearest(s, _rng(0, 3))),
        ("queryWinding (n, 3)", lambda n: pt.queryWinding(s, _rng(n, 3))),
        ("queryWinding (n, 4) beta=inf", lambda n: pt.queryWinding(s, _rng(n, 4), beta=inf)),
        ("queryNearestK", lambda n: pt.queryNearestK(s, _rng(n, 3))),
        ("queryNearestK k=2 counts", lambda n: pt.queryNearestK(s, np.abs(_rng(n, 4)), k=2, counts=True)),
        ("queryNearestK k=0 counts", lambda n: pt.queryNearestK(s, _rng(n, 3), k=0, max_radius=1.0, counts=True)),
        ("queryWithinAny radius", lambda n: pt.queryWithinAny(s, _rng(n, 3), radius=0.5)),
        ("queryWithinAny (n, 4)", lambda n: pt.queryWithinAny(s, np.abs(_rng(n, 4)))),
        ("sphereContacts", lambda n: pt.sphereContacts(s, _rng(n, 3), 0.5)),
        ("sphereContacts radii max_contacts=3", lambda n: pt.sphereContacts(s, _rng(n, 3), np.abs(_rng(n)), max_contacts=3)),
        ("querySegments (n, 6)", lambda n: pt.querySegments(s, _rng(n, 6), max_radius=3.0)),
        ("querySegments (n, 8)", lambda n: pt.querySegments(s, np.abs(_rng(n, 8)))),
        ("capsuleClearance", lambda n: pt.capsuleClearance(s, _rng(n, 3), _rng(n, 3) + 1, 0.25)),
        ("queryOverlap", lambda n: pt.queryOverlap(s, _rng(n, 3), 0.5)),
        ("queryOverlap records max_prims=3 no counts", lambda n: pt.queryOverlap(s, np.abs(_rng(n, 8)), max_prims=3, counts=False)),
        ("queryOverlap max_prims=0", lambda n: pt.queryOverlap(s, _rng(n, 3), np.abs(_rng(n, 3)), max_prims=0)),
        ("queryOverlapAny", lambda n: pt.queryOverlapAny(s, _rng(n, 3), (0.5, 0.25, 1.0))),
        ("bakeOccupancy", lambda n: pt.bakeOccupancy(s, (1, n, 1), bounds=((0, 0, 0), (1, 1, 1))) if n else pt.queryOverlapAny(s, _rng(0, 8))),
        ("bakeOccupancy counts", lambda n: pt.bakeOccupancy(s, (n, 1, 1), bounds=((0, 0, 0), (1, 1, 1)), counts=True) if n else pt.queryOverlapAny(s, _rng(0, 8))),
        ("bakeOccupancy frame", lambda n: pt.bakeOccupancy(s, (1, 1, n), bounds=((0, 0, 0), (1, 1, 1)), frame=np.eye(4)[:3]) if n else pt.queryOverlapAny(s, _rng(0, 8))),
        ("bakeOccupancy frame counts", lambda n: pt.bakeOccupancy(s, (1, 1, n), bounds=((0, 0, 0), (1, 1, 1)), frame=np.eye(4)[:3], counts=True) if n else pt.queryOverlapAny(s, _rng(0, 8))),
        ("queryTriangles", lambda n: pt.queryTriangles(s, _rng(n, 3, 3))),
        ("queryTriangles (n, 9) max_prims=2 no counts", lambda n: pt.queryTriangles(s, _rng(n, 9), max_prims=2, counts=False)),
        ("queryTriangles (n, 12) max_prims=0", lambda n: pt.queryTriangles(s, _rng(n, 12), max_prims=0)),
        ("queryTrianglesAny", lambda n: pt.queryTrianglesAny(s, _rng(n, 3, 3))),
        ("queryOverlapLists", lambda n: pt.queryOverlapLists(s, _rng(n, 3), 0.5)),
        ("queryTrianglesLists", lambda n: pt.queryTrianglesLists(s, _rng(n, 3, 3))),
        ("queryOverlapOriented", lambda n: pt.queryOverlapOriented(s, obox(n))),
        ("queryOverlapOriented max_prims=0", lambda n: pt.queryOverlapOriented(s, obox(n), max_prims=0)),
        ("queryOverlapOriented max_prims=1 no counts", lambda n: pt.queryOverlapOriented(s, obox(n), max_prims=1, counts=False)),
        ("queryOverlapOrientedAny", lambda n: pt.queryOverlapOrientedAny(s, obox(n))),
        ("queryOverlapOrientedLists", lambda n: pt.queryOverlapOrientedLists(s, obox(n))),
        ("poseBoxes", lambda n: pt.poseBoxes(s, _poses(n), (0, 0, 0), (1, 2, 3))),
        ("posedMeshBoxes", lambda n: pt.posedMeshBoxes(s, _VERTS, _poses(n))),
        ("meshCollisions", lambda n: pt.meshCollisions(s, _VERTS, _IDX, _poses(n))),
        ("meshCollisions pairs", lambda n: pt.meshCollisions(s, _VERTS, _IDX, _poses(n), pairs=True)),
        ("meshCollisions all pairs", lambda n: pt.meshCollisions(s, _VERTS, _IDX, _poses(n), pairs="all")),
        ("queryTriangleDistance", lambda n: pt.queryTriangleDistance(s, _rng(n, 3, 3), max_radius=2.0)),
        ("queryTriangleDistance (n, 12)", lambda n: pt.queryTriangleDistance(s, np.abs(_rng(n, 12)))),
        ("meshClearance", lambda n: pt.meshClearance(s, _VERTS, _IDX, _poses(n), max_radius=4.0)),
        ("posedTriangles", lambda n: pt.posedTriangles(s, _poses(n))),
        ("posedTriangles split", lambda n: pt.posedTriangles(s, _poses(n), _limit=2 * MESH_TRIS)),
        ("queryPosesAny", lambda n: pt.queryPosesAny(s, _poses(n))),
        ("queryPosesAny first", lambda n: pt.queryPosesAny(s, _poses(n), first=True)),
        ("queryPosesAny first split", lambda n: pt.queryPosesAny(s, _poses(n).reshape(n, 12), first=True, _limit=2 * MESH_TRIS)),
        ("queryPosesDistance", lambda n: pt.queryPosesDistance(s, _poses(n), max_radius=1.5)),
        ("queryPosesDistance split", lambda n: pt.queryPosesDistance(s, _poses(n), _limit=MESH_TRIS)),
        ("querySweep records", lambda n: pt.querySweep(s, np.abs(_rng(n, 8)))),
        ("querySweep records any_hit", lambda n: pt.querySweep(s, np.abs(_rng(n, 8)), any_hit=True)),
        ("querySweep origins", lambda n: pt.querySweep(s, _rng(n, 3), _rng(n, 3), radius=0.25, tmax=3.0)),
        ("querySweep origins per item any_hit", lambda n: pt.querySweep(s, _rng(n, 3), _rng(n, 3), radius=np.abs(_rng(n)), tmax=np.abs(_rng(n)), any_hit=True)),
        ("queryCapsuleCast records", lambda n: pt.queryCapsuleCast(s, np.abs(_rng(n, 12)))),
        ("queryCapsuleCast records any_hit", lambda n: pt.queryCapsuleCast(s, np.abs(_rng(n, 12)), any_hit=True)),
        ("queryCapsuleCast ends", lambda n: pt.queryCapsuleCast(s, _rng(n, 3), _rng(n, 3), _rng(n, 3), radius=0.25)),
        ("queryCapsuleCast ends per item any_hit", lambda n: pt.queryCapsuleCast(s, _rng(n, 3), _rng(n, 3), _rng(n, 3), radius=np.abs(_rng(n)), tmax=np.abs(_rng(n)), any_hit=True)),
        ("queryBoxCast records", lambda n: pt.queryBoxCast(s, box_casts(n))),
        ("queryBoxCast records any_hit", lambda n: pt.queryBoxCast(s, box_casts(n), any_hit=True)),
        ("queryBoxCast boxes", lambda n: pt.queryBoxCast(s, obox(n), (0, 0, 1), tmax=2.0)),
        ("queryBoxCast boxes per item any_hit", lambda n: pt.queryBoxCast(s, obox(n), _rng(n, 3), tmax=np.abs(_rng(n)), any_hit=True)),
        ("poseBoxCasts", lambda n: pt.poseBoxCasts(s, _poses(n), ((0, 0, 0), (1, 1, 1)), (0, 0, 1, 2))),
        ("queryTriangleCast records", lambda n: pt.queryTriangleCast(s, np.abs(_rng(n, 16)))),
        ("queryTriangleCast records any_hit", lambda n: pt.queryTriangleCast(s, np.abs(_rng(n, 16)), any_hit=True)),
        ("queryTriangleCast triangles", lambda n: pt.queryTriangleCast(s, _rng(n, 3, 3), (0, 1, 0), tmax=2.0)),
        ("queryTriangleCast triangles per item any_hit", lambda n: pt.queryTriangleCast(s, _rng(n, 9), _rng(n, 3), tmax=np.abs(_rng(n)), any_hit=True)),
        ("queryPosesCast", lambda n: pt.queryPosesCast(s, _poses(n), (0, 0, 1, 5))),
        ("queryPosesCast per pose directions", lambda n: pt.queryPosesCast(s, _poses(n), _rng(n, 3))),
        ("meshCast", lambda n: pt.meshCast(s, _VERTS, _IDX, _poses(n), (1, 0, 0))),
    ]


SIZES = (0, 1, 5)
TOTALS = {"lists hold 2 n + 1": lambda n: 2 * n + 1, "lists are empty": lambda n: 0}


def run_case(pt, f, n, stub):
    """f(n) with the stub in the library's place: (description of the result or None, the PathTracerError or None)"""
    from acgpathtracing_amd import _native
    real = _native.hip
    _native.hip = lambda: stub
    try:
        return describe(f(n)), None
    except pt.PathTracerError as e:
        return None, e
    finally:
        _native.hip = real


def record(pt):
    """{label: {total: {n: {"calls": trace, "result": description}}}}"""
    got = {}
    for label, f in cases(pt):
        got[label] = {}
        for tname, total in TOTALS.items():
            # the stub's counts stay zero: meshCollisions, which expands them, agrees with empty lists only
            if (tname == "lists are empty") != ("all pairs" in label) and "Lists" not in label:
                continue
            per_n = {}
            for n in SIZES:
                stub = Stub(total=total)
                result, err = run_case(pt, f, n, stub)
                assert err is None, (label, n, err)
                per_n[str(n)] = {"calls": trace(stub.events), "result": result}
            got[label][tname] = per_n
    return got


# ---- the fixture's form ------------------------------------------------------------------------------------------------------------
def pack(got):
    """record()'s answer as the fixture holds it: the distinct calls and the distinct results once, and per case, kind of total and n
    the indices of its calls and of its result"""
    calls, results, cases = [], [], {}

    def index(table, x):
        if x not in table:
            table.append(x)
        return table.index(x)
    for label, per_total in got.items():
        cases[label] = {tname: {n: [[index(calls, e) for e in one["calls"]], index(results, one["result"])] for n, one in per_n.items()}
                        for tname, per_n in per_total.items()}
    return {"calls": calls, "results": results, "cases": cases}


def unpack(fixture):
    return {label: {tname: {n: {"calls": [fixture["calls"][k] for k in one[0]], "result": fixture["results"][one[1]]} for n, one in per_n.items()}
                    for tname, per_n in per_total.items()} for label, per_total in fixture["cases"].items()}
