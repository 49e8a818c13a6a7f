"""What tests/test_group_host.py and tests/test_gpu_group.py share: a NumPy mirror of the owner formula of render_megakernel.hip
k_keep_owned, and the helpers that hold a pt_create_multi group to a plain context call by call.

The reference of every comparison is the plain context (held to the CPU oracle by the parity suite): DESIGN.md section 6 shows that a
group's reduce has exactly one non-zero term per pixel, so the accumulation, the resolved frame buffer and the summed counters of a
group equal the plain context's as bits and integers.  Nothing here knows a tolerance.

A plain module: importing it touches no GPU."""
import ctypes as C
import os
import sys

import numpy as np

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
from scene_utils import make_params

BOX = os.path.join(pt.SCENES, "cornell_box.obj")
REHEARSE = "ACGPT_REHEARSE_SAME_GPU"
COUNTERS = ("radiance_rays", "shadow_rays", "paths", "pixels")


def owner(x, y, world):
    """The rank that owns pixel (x, y): k_keep_owned's expression, on integer arrays."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return ((x >> 3) % world - (y >> 2) % world + world) % world


def owner_image(w, h, world):
    """[h, w] of owner(x, y, world)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return owner(xx, yy, world)


# ---- twins ---------------------------------------------------------------------------------------------------------------------------

def make_twins(gpu_state_factory, monkeypatch, path, world, sample_chunks, width=96, height=64, spp=8, **kw):
    """(plain state, group state of `world` ranks on device 0, the scene's TinyObjWrapper): identical settings on both sides.  The
    rehearsal switch is in the environment only while the group is created."""
    assert sample_chunks in (1, 4)          # explicit on both sides: the automatic choice depends on pixels per rank
    args = dict(width=width, height=height, max_depth=4, direct_lighting=True, importance_sampling=True, spp=spp, sample_chunks=sample_chunks)
    args.update(kw)
    plain, obj = gpu_state_factory(path, **args)
    assert REHEARSE not in os.environ
    monkeypatch.setenv(REHEARSE, "1")
    try:
        group, _ = gpu_state_factory(path, device_ids=[0] * world, **args)
    finally:
        monkeypatch.delenv(REHEARSE)
    assert _native.hip().pt_device_count(group.context) == world and _native.hip().pt_device_count(plain.context) == 1
    return plain, group, obj


def release(*states):
    """Destroy the contexts now (the factory's clean-up at the end of the session then finds nothing left to do)."""
    for s in states:
        pt.CleanAllTheThings(s)


def error_of(state):
    return _native.hip().pt_last_error(state.context) or b""


def counters(state):
    s = _native.Stats()
    assert _native.hip().pt_get_stats(state.context, C.byref(s)) == 0
    return tuple(int(getattr(s, k)) for k in COUNTERS)


class Image:
    """An accumulation buffer and a frame buffer of one context on the device, w x h, the accumulation zero or `prior`."""

    def __init__(self, state, w, h, prior=None):
        self.state, self.w, self.h = state, int(w), int(h)
        L = _native.hip()
        self.acc, self.fb = C.c_void_p(), C.c_void_p()
        assert L.pt_device_malloc(state.context, C.byref(self.acc), self.w * self.h * 16) == 0, error_of(state)
        assert L.pt_device_malloc(state.context, C.byref(self.fb), self.w * self.h * 4) == 0, error_of(state)
        assert L.pt_device_memset(state.context, self.fb, 0, self.w * self.h * 4) == 0
        if prior is None:
            assert L.pt_device_memset(state.context, self.acc, 0, self.w * self.h * 16) == 0
        else:
            self.put(prior)

    def put(self, acc):
        a = np.ascontiguousarray(acc).view(np.uint32)
        assert a.size == self.w * self.h * 4
        assert _native.hip().pt_copy_to_device(self.state.context, self.acc, a.ctypes.data, a.nbytes) == 0, error_of(self.state)

    def params(self, frame, spp=None, depth=None):
        p = self.state.params
        q = make_params(self.w, self.h, int(p.samplesPerPixel) if spp is None else spp, int(p.maxDepth) if depth is None else depth,
                        bool(p.useDirectLighting), bool(p.useImportanceSampling), frame=frame)
        q.accumulationBuffer, q.frameBuffer = self.acc.value, self.fb.value
        q.handle = _native.hip().pt_scene_handle(self.state.context)
        return q

    def launch(self, frame, n=1, refused=False):
        """pt_launch_frames of frames frame .. frame + n - 1; the launch's counters, or the return code of a launch that is to be refused"""
        q = self.params(frame)
        rc = _native.hip().pt_launch_frames(self.state.context, C.byref(q), n)
        if refused:
            return rc
        assert rc == 0, error_of(self.state)
        return counters(self.state)

    def read(self):
        """(accumulation [h, w, 4] uint32, frame buffer [h, w, 4] uint8)"""
        L = _native.hip()
        acc, fb = np.zeros((self.h, self.w, 4), np.uint32), np.zeros((self.h, self.w, 4), np.uint8)
        assert L.pt_copy_to_host(self.state.context, acc.ctypes.data, self.acc, acc.nbytes) == 0, error_of(self.state)
        assert L.pt_copy_to_host(self.state.context, fb.ctypes.data, self.fb, fb.nbytes) == 0, error_of(self.state)
        return acc, fb

    def free(self):
        if self.state.context:
            for p in (self.acc, self.fb):
                if p.value:
                    _native.hip().pt_device_free(self.state.context, p)
        self.acc = self.fb = C.c_void_p()


def render(state, w, h, frames, fuse=1, frame0=0, prior=None):
    """Frames frame0 .. frame0 + frames - 1 into fresh buffers, `fuse` per pt_launch_frames: (accumulation bits, frame buffer, the
    counters of every launch)."""
    img = Image(state, w, h, prior)
    try:
        sts, f = [], 0
        while f < frames:
            n = min(fuse, frames - f)
            sts.append(img.launch(frame0 + f, n))
            f += n
        acc, fb = img.read()
    finally:
        img.free()
    return acc, fb, sts


def total(sts):
    """Counters of a sequence of launches: rays and paths summed, the pixel count of each launch"""
    return tuple(sum(s[k] for s in sts) for k in range(3)) + (tuple(s[3] for s in sts),)


def assert_same(got, want, what):
    """(accumulation bits, frame buffer, counters) of the group against the plain context's: equal bits, equal integers."""
    (acc, fb, st), (racc, rfb, rst) = got, want
    assert acc.dtype == np.uint32 and racc.dtype == np.uint32 and acc.shape == racc.shape, what
    diff = np.any(acc != racc, axis=-1)
    if diff.any():
        yx = np.argwhere(diff)
        raise AssertionError("%s: %d of %d pixels differ in the accumulation, first at (y, x) %s" % (what, int(diff.sum()), diff.size, yx[:4].tolist()))
    assert np.array_equal(fb, rfb), "%s: frame buffer" % (what,)
    assert st == rst, "%s: counters %s, the plain context's %s" % (what, st, rst)


def same_render(plain, group, w, h, frames, fuse, what, **kw):
    """Render on both sides and compare; returns the plain context's (accumulation bits, frame buffer, [counters])."""
    want = render(plain, w, h, frames, fuse, **kw)
    got = render(group, w, h, frames, fuse, **kw)
    assert_same(got, want, what)
    return want


class TwinImage:
    """The same buffers on both sides, for sequences that keep them across launches: every call goes to the plain context's Image and to
    the group's."""

    def __init__(self, plain, group, w, h, prior=None):
        self.sides = [Image(plain, w, h, prior), Image(group, w, h, prior)]

    def put(self, acc):
        for i in self.sides:
            i.put(acc)

    def launch(self, frame, n=1):
        want, got = [i.launch(frame, n) for i in self.sides]
        assert got == want, "counters %s, the plain context's %s" % (got, want)

    def check(self, what):
        """both sides' buffers hold the same bits; returns the plain context's (accumulation bits, frame buffer)"""
        (racc, rfb), (acc, fb) = [i.read() for i in self.sides]
        assert_same((acc, fb, None), (racc, rfb, None), what)
        return racc, rfb

    def free(self):
        for i in self.sides:
            i.free()


def blob(x):
    """The bytes of a query result: an array, or a dict / tuple of them, in a fixed order."""
    if isinstance(x, dict):
        return b"".join(k.encode() + b"\0" + blob(x[k]) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return b"".join(blob(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


def prior_image(w, h):
    """[h, w, 4] float32, every value distinct, finite and strictly positive: 1/4 + i / 1024 (exact in fp32 up to 2^14 values per unit)"""
    a = (np.float32(0.25) + np.arange(w * h * 4, dtype=np.float32) * np.float32(2.0 ** -10)).reshape(h, w, 4)
    assert np.unique(a).size == a.size and np.isfinite(a).all() and (a > 0).all()
    return a


# ---- the mesh of the update tests ---------------------------------------------------------------------------------------------------

def sphere_scene(path):
    """One icosphere of 320 triangles in the Cornell shell with its lamp (12 triangles): the generator of the refit tests at its smallest.
    Writes path and a sibling .mtl."""
    if pt.SCENES not in sys.path:
        sys.path.insert(0, pt.SCENES)
    import make_scenes
    make_scenes.stress_scene(path, n_spheres=1, subdiv=2, mtl_name=os.path.basename(path)[:-4] + ".mtl")
    return path


def object_vertices(path, prefix):
    """0-based indices of the vertices that the faces of the OBJ objects whose name starts with `prefix` reference."""
    out, obj, nv = set(), "", 0
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "o":
            obj = t[1]
        elif t[0] == "v":
            nv += 1
        elif t[0] == "f" and obj.startswith(prefix):
            for w in t[1:]:
                k = int(w.split("/")[0])
                out.add(k - 1 if k > 0 else nv + k)
    return np.array(sorted(out))
