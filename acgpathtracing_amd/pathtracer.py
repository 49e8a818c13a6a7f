"""Host-side mirror of the reference's render path, over the C ABI.

Names, argument meaning and error behaviour follow PathTracer_Optix/PathTracerMain.cpp so a
test written against the reference's functions reads the same here:

    reference (PathTracerMain.cpp)                 here
    ------------------------------------------------------------------------------
    TinyObjWrapper obj(path)            :650       TinyObjWrapper(path)
    initCamera()                        :228-233   initCamera()
    createDeviceContext(state)          :240-258   createDeviceContext(state)
    buildTheAccelarationStructure(..)   :260-398   buildTheAccelarationStructure(state, obj)
    createModule/ProgramGroups/Pipeline :400-539   (nothing to do: AOT gfx950 code object)
    createShaderBindingTable(state,obj) :544-627   createShaderBindingTable(state, obj)
    initializeTheLaunch(state)          :143-164   initializeTheLaunch(state)
    updateState(output_buffer, state)   :166-182   updateState(output_buffer, state)
    LaunchCurrentFrame(buffer, state)   :184-210   LaunchCurrentFrame(output_buffer, state)
    keyCallback(...)                    :100-141   keyCallback(state, key)
    CleanAllTheThings(state)            :629-646   CleanAllTheThings(state)
    sutil::CUDAOutputBuffer<uchar4>                OutputBuffer (DEVICE / ZERO_COPY modes)

Everything that computes runs in libacgpt_hip.so; this module only marshals.
"""
import ctypes as C
import os

import numpy as np

from . import _native
from ._native import AreaLight, BvhInfo, Float3, Material, PathTraceParams, Stats

BSDF_DIFFUSE, BSDF_METALLIC, BSDF_REFRACTION = 0, 1, 2

# PathTracerMain.cpp:42-43, 58-59
maxiumumRecursionDepth = 28
samples_per_launch = 128

SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scenes")


class PathTracerError(RuntimeError):
    """Counterpart of sutil::Exception thrown by CUDA_CHECK / OPTIX_CHECK (sutil/Exception.h:82-112)."""


def _check(ctx, rc, what):
    if rc != 0:
        msg = _native.hip().pt_last_error(ctx)
        raise PathTracerError("%s failed: %s" % (what, msg.decode() if msg else "unknown error"))


def _f3(v):
    return Float3(float(v[0]), float(v[1]), float(v[2]))


# ------------------------------------------------------------------ scene ingest ----
class TinyObjWrapper:
    """OBJ/MTL ingest, API of PathTracer_Optix/TinyObjWrapper.h:77-115 (the parsing itself is
    the C++ in acgpathtracing_amd/host/TinyObjWrapper.cpp)."""

    def __init__(self, filename=None):
        self.dataLoaded = False
        self._vertices = np.zeros(0, np.float32)
        self._indexBuffer = np.zeros(0, np.uint32)
        self._materialIndices = np.zeros(0, np.uint32)
        self._materials = (Material * 0)()
        self.warning = ""
        self.error = ""
        if filename is not None:
            self.loadFile(filename)

    def loadFile(self, filename):
        L = _native.host()
        h = L.pth_obj_load(os.fsencode(filename))
        try:
            self.dataLoaded = bool(L.pth_obj_ok(h))
            self.warning = (L.pth_obj_warning(h) or b"").decode()
            self.error = (L.pth_obj_error(h) or b"").decode()
            if not self.dataLoaded:
                return False
            sizes = [C.c_size_t() for _ in range(4)]
            L.pth_obj_sizes(h, *[C.byref(s) for s in sizes])
            nv, ni, nm, nmat = [s.value for s in sizes]
            self._vertices = np.zeros(nv, np.float32)
            self._indexBuffer = np.zeros(ni, np.uint32)
            self._materialIndices = np.zeros(nm, np.uint32)
            self._materials = (Material * nmat)()
            L.pth_obj_fill(h, self._vertices.ctypes.data, self._indexBuffer.ctypes.data,
                           self._materialIndices.ctypes.data, C.addressof(self._materials) if nmat else None)
        finally:
            L.pth_obj_free(h)
        return True

    def getVerticesFloat(self):
        return self._vertices

    def getIndexBuffer(self):
        return self._indexBuffer

    def getMaterialIndices(self):
        return self._materialIndices

    def getMaterials(self):
        return self._materials

    def getNumMaterials(self):
        return len(self._materials)


# ------------------------------------------------------------------------ camera ----
class Camera:
    """sutil::Camera (sutil/Camera.h:38-75); UVWFrame is computed by the C++ host library."""

    def __init__(self, eye=(1.0, 1.0, 1.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovY=35.0, aspectRatio=1.0):
        self.m_eye, self.m_lookat, self.m_up = tuple(eye), tuple(lookat), tuple(up)
        self.m_fovY, self.m_aspectRatio = float(fovY), float(aspectRatio)

    def eye(self): return self.m_eye
    def setEye(self, v): self.m_eye = tuple(v)
    def lookat(self): return self.m_lookat
    def setLookat(self, v): self.m_lookat = tuple(v)
    def up(self): return self.m_up
    def setUp(self, v): self.m_up = tuple(v)
    def fovY(self): return self.m_fovY
    def setFovY(self, v): self.m_fovY = float(v)
    def aspectRatio(self): return self.m_aspectRatio
    def setAspectRatio(self, v): self.m_aspectRatio = float(np.float32(v))

    def UVWFrame(self):
        e = np.asarray(self.m_eye, np.float32); l = np.asarray(self.m_lookat, np.float32); u = np.asarray(self.m_up, np.float32)
        U = np.zeros(3, np.float32); V = np.zeros(3, np.float32); W = np.zeros(3, np.float32)
        _native.host().pth_camera_uvw(e.ctypes.data, l.ctypes.data, u.ctypes.data, C.c_float(self.m_fovY),
                                      C.c_float(self.m_aspectRatio), U.ctypes.data, V.ctypes.data, W.ctypes.data)
        return U, V, W


g_camera = Camera()


def initCamera():
    """PathTracerMain.cpp:228-233."""
    g_camera.setEye((278.0, 273.0, -900.0))
    g_camera.setLookat((278.0, 273.0, 330.0))
    g_camera.setUp((0.0, 1.0, 0.0))
    g_camera.setFovY(35.0)
    return g_camera


# ----------------------------------------------------------------- output buffer ----
class OutputBufferType:
    """sutil::CUDAOutputBufferType (sutil/CUDAOutputBuffer.h:45-51); the GL_INTEROP and CUDA_P2P
    modes have no meaning on a headless single-process-per-GPU node."""
    DEVICE = 0
    ZERO_COPY = 2


class OutputBuffer:
    """uchar4 framebuffer owner with sutil::CUDAOutputBuffer's map/unmap/getHostPointer protocol."""

    def __init__(self, buffer_type, width, height, state=None):
        self.m_type = buffer_type
        self.m_width = self.m_height = 0
        self._state = state
        self._dev = None
        self._host_mapped = None
        self._host = None
        if state is not None:
            self.resize(width, height)
        else:
            self.m_width, self.m_height = int(width), int(height)

    def _ctx(self):
        if self._state is None or not self._state.context:
            raise PathTracerError("OutputBuffer: no device context")
        return self._state.context

    def attach(self, state):
        self._state = state
        self.resize(self.m_width, self.m_height)

    def width(self): return self.m_width
    def height(self): return self.m_height
    def setStream(self, stream): pass     # launches and copies share the context's stream
    def setDevice(self, device_idx): pass

    def _release(self):
        L = _native.hip()
        if self._dev is not None and self.m_type == OutputBufferType.DEVICE:
            L.pt_device_free(self._ctx(), self._dev)
        if self._host_mapped is not None:
            L.pt_host_free_mapped(self._ctx(), self._host_mapped)
        self._dev = self._host_mapped = None

    def resize(self, width, height):
        L = _native.hip()
        self._release()
        self.m_width, self.m_height = max(1, int(width)), max(1, int(height))
        nbytes = self.m_width * self.m_height * 4
        if self.m_type == OutputBufferType.DEVICE:
            p = C.c_void_p()
            _check(self._ctx(), L.pt_device_malloc(self._ctx(), C.byref(p), nbytes), "OutputBuffer.resize")
            self._dev = p.value
        else:
            hp, dp = C.c_void_p(), C.c_void_p()
            _check(self._ctx(), L.pt_host_malloc_mapped(self._ctx(), C.byref(hp), C.byref(dp), nbytes), "OutputBuffer.resize")
            self._host_mapped, self._dev = hp.value, dp.value
        self._host = np.zeros((self.m_height, self.m_width, 4), np.uint8)

    def map(self):
        return self._dev

    def unmap(self):
        pass   # pt_launch returns synchronised (the reference syncs the stream here, CUDAOutputBuffer.h:259-275)

    def getHostPointer(self):
        """uint8 array [height, width, 4]; row 0 is the bottom image row."""
        L = _native.hip()
        nbytes = self.m_width * self.m_height * 4
        if self.m_type == OutputBufferType.DEVICE:
            _check(self._ctx(), L.pt_copy_to_host(self._ctx(), self._host.ctypes.data, self._dev, nbytes), "OutputBuffer.getHostPointer")
        else:
            C.memmove(self._host.ctypes.data, self._host_mapped, nbytes)
        return self._host

    def free(self):
        self._release()


# ------------------------------------------------------------------ render state ----
class PathTracerState:
    """PathTracerState, PathTracerMain.cpp:71-93 (the OptiX handles collapse into one context)."""

    def __init__(self):
        self.context = None
        self.params = PathTraceParams()
        self.refreshAccumulationBuffer = False
        self.frame_counter = 0
        self.sample_summ = 0
        self.total_ms = 0.0
        self._accum_bytes = 0
        self._temporal = []           # TemporalHistory objects holding device buffers of this context (freed by CleanAllTheThings)
        self._scene_verts = None      # host copy of the scene's current vertex positions, (n, 4) float32
        self._scene_idx = None        # host copy of the scene's index buffer, (n_tris, 3) uint32: bakeVertexAO's triangles
        self._scene_serial = 0        # advanced by buildTheAccelarationStructure only (pt_set_scene): TemporalHistory(motion=True)'s key
        self._verts_serial = 0        # advanced by every change of the positions (a build or updateVertices)
        self._mats_serial = 0         # advanced by every change of the materials (a build or updateMaterials)
        self._device = 0              # the context's device (rank 0's of a group): where queryRays expects a tensor of rays


def createDeviceContext(state, device_id=0, device_ids=None):
    """device_ids (a list): ONE context over several GPUs of the node (pt_create_multi) — pixel tiles per device and an
    RCCL reduce of the accumulation per launch behind the same functions; device_id alone: the reference's one device."""
    L = _native.hip()
    ctx = C.c_void_p()
    if device_ids is not None:
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        rc = L.pt_create_multi(C.byref(ctx), ids, len(device_ids))
    else:
        rc = L.pt_create(C.byref(ctx), int(device_id))
    if rc != 0:
        msg = L.pt_last_error(None)
        raise PathTracerError("createDeviceContext failed: %s" % (msg.decode() if msg else "unknown"))
    state.context = ctx
    state._device = int(device_ids[0]) if device_ids is not None else int(device_id)


def buildTheAccelarationStructure(state, objs):
    """Uploads geometry + materials and builds the LBVH on the device."""
    L = _native.hip()
    v = np.ascontiguousarray(objs.getVerticesFloat(), np.float32)
    idx = np.ascontiguousarray(objs.getIndexBuffer(), np.uint32)
    mid = np.ascontiguousarray(objs.getMaterialIndices(), np.uint32)
    mats = objs.getMaterials()
    state._materials = mats
    rc = L.pt_set_scene(state.context, v.ctypes.data, v.size // 4, idx.ctypes.data, idx.size // 3,
                        mid.ctypes.data, C.addressof(mats) if len(mats) else None, len(mats))
    _check(state.context, rc, "buildTheAccelarationStructure")
    state.params.handle = L.pt_scene_handle(state.context)
    state._scene_verts = v.reshape(-1, 4).copy()
    state._scene_idx = idx.reshape(-1, 3).copy()
    state._scene_serial += 1
    state._verts_serial += 1
    state._mats_serial += 1


def createModule(state): pass
def createProgramGroups(state): pass
def createPipeline(state): pass


def createShaderBindingTable(state, obj):
    """The per-material records were uploaded with the scene (pt_set_scene); nothing else to bind."""
    return None


def _alloc_accumulation(state):
    L = _native.hip()
    nbytes = int(state.params.width) * int(state.params.height) * 16
    p = C.c_void_p()
    _check(state.context, L.pt_device_malloc(state.context, C.byref(p), nbytes), "accumulation alloc")
    # zero-filled: under pt_set_partition(rank, world) the pixels of other ranks are never written and the
    # cross-rank reduce(SUM) of distributed.reduce_accumulation relies on them being 0
    _check(state.context, L.pt_device_memset(state.context, p, 0, nbytes), "accumulation clear")
    state.params.accumulationBuffer = p.value
    state._accum_bytes = nbytes


def initializeTheLaunch(state):
    """PathTracerMain.cpp:143-164 — including the hard-coded area light (:154-158)."""
    _alloc_accumulation(state)
    state.params.frameBuffer = None
    state.params.samplesPerPixel = samples_per_launch
    state.params.currentFrameIdx = 0
    al = state.params.areaLight
    al.emission = Float3(10.0, 10.0, 10.0)
    al.corner = Float3(343.0, 547.0, 227.0)
    al.v1 = Float3(0.0, 0.0, 105.0)
    al.v2 = Float3(-130.0, 0.0, 0.0)
    # normalize(cross(v1, v2)) in fp32, vec_math.h:533-549
    v1 = np.array([0.0, 0.0, 105.0], np.float32); v2 = np.array([-130.0, 0.0, 0.0], np.float32)
    c = np.array([v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]], np.float32)
    inv = np.float32(1.0) / np.sqrt(np.float32(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), dtype=np.float32)
    al.normal = _f3(c * inv)


def updateState(output_buffer, state):
    """PathTracerMain.cpp:166-182."""
    if state.refreshAccumulationBuffer:
        state.refreshAccumulationBuffer = False
        state.params.currentFrameIdx = 0
        state.sample_summ = 0
        state.frame_counter = 0
        state.total_ms = 0.0
        L = _native.hip()
        if state.params.accumulationBuffer:
            L.pt_device_free(state.context, state.params.accumulationBuffer)
        _alloc_accumulation(state)


def LaunchCurrentFrame(output_buffer, state, sub_frames=1):
    """PathTracerMain.cpp:184-210: map, launch, unmap, synchronised on return.  sub_frames > 1 renders that many
    consecutive frames (currentFrameIdx, currentFrameIdx + 1, ...) in one kernel launch (pt_launch_frames); the
    buffers end up as after sub_frames separate calls.  The caller advances currentFrameIdx."""
    L = _native.hip()
    state.params.frameBuffer = output_buffer.map() if output_buffer is not None else None
    rc = L.pt_launch_frames(state.context, C.byref(state.params), int(sub_frames))
    if output_buffer is not None:
        output_buffer.unmap()
    _check(state.context, rc, "LaunchCurrentFrame")


def setLightMode(state, mode):
    """0: the reference's estimator (hard-coded rectangle, PathTracerMain.cpp:154-158; the default).  1: the scene's own
    emissive triangles as the area light, light and BSDF sampling combined by the power heuristic (opt-in)."""
    _check(state.context, _native.hip().pt_set_light_mode(state.context, int(mode)), "pt_set_light_mode")
    state._light_mode = int(mode)
    state.refreshAccumulationBuffer = True


def setMaterialModel(state, model):
    """0 / "reference": the reference's materials (the default).  1 / "microfacet": metal and glass honour pt_material.roughness as
    rough GGX BSDFs, light-sampled with MIS (include/acgpt.h pt_set_material_model); part of light mode 1: a launch in light mode 0
    under model 1 is refused."""
    m = {"reference": _native.MATERIALS_REFERENCE, "microfacet": _native.MATERIALS_MICROFACET}.get(model, model)
    _check(state.context, _native.hip().pt_set_material_model(state.context, int(m)), "pt_set_material_model")
    state._material_model = int(m)
    state.refreshAccumulationBuffer = True


def readHDR(path):
    """Radiance .hdr (RGBE, flat or run-length encoded scanlines, "-Y H +X W"): float32 [H, W, 3], row 0 = the top row.
    The same reader as host/ImageIO.cpp loadHDR."""
    d = open(path, "rb").read()
    pos = d.index(b"\n") + 1
    if not d.startswith(b"#?"):
        raise ValueError("%s: not a Radiance HDR file" % path)
    while True:
        end = d.index(b"\n", pos)
        line = d[pos:end]
        pos = end + 1
        if not line:
            break
        if line.startswith(b"FORMAT=") and line != b"FORMAT=32-bit_rle_rgbe":
            raise ValueError("%s: unsupported %s" % (path, line.decode()))
    end = d.index(b"\n", pos)
    f = d[pos:end].split()
    pos = end + 1
    if len(f) != 4 or f[0] != b"-Y" or f[2] != b"+X":
        raise ValueError("%s: unsupported resolution line" % path)
    h, w = int(f[1]), int(f[3])
    px = np.zeros((h, w, 4), np.uint8)
    for y in range(h):
        if 8 <= w < 32768 and d[pos:pos + 2] == b"\x02\x02" and ((d[pos + 2] << 8) | d[pos + 3]) == w and not d[pos + 2] & 0x80:
            pos += 4
            for c in range(4):
                x = 0
                while x < w:
                    n = d[pos]
                    pos += 1
                    if n > 128:
                        n -= 128
                        px[y, x:x + n, c] = d[pos]
                        pos += 1
                    else:
                        if n == 0:
                            raise ValueError("%s: bad run-length data" % path)
                        px[y, x:x + n, c] = np.frombuffer(d, np.uint8, n, pos)
                        pos += n
                    x += n
        else:
            px[y] = np.frombuffer(d, np.uint8, 4 * w, pos).reshape(w, 4)
            pos += 4 * w
    e = px[..., 3:4].astype(np.int32)
    return np.where(e > 0, np.ldexp(px[..., :3].astype(np.float32), e - 136), 0).astype(np.float32)


def readPFM(path):
    """.pfm (PF colour / Pf grey, either byte order): float32 [H, W, 3], row 0 = the top row (the file stores the bottom row first)."""
    d = open(path, "rb").read()
    toks, pos = [], 0
    for _ in range(4):
        while d[pos:pos + 1].isspace():
            pos += 1
        b = pos
        while pos < len(d) and not d[pos:pos + 1].isspace():
            pos += 1
        toks.append(d[b:pos])
    pos += 1
    nc = {b"PF": 3, b"Pf": 1}.get(toks[0])
    w, h, scale = int(toks[1]), int(toks[2]), float(toks[3])
    if nc is None or scale == 0.0:
        raise ValueError("%s: not a PFM file" % path)
    a = np.frombuffer(d, "<f4" if scale < 0 else ">f4", w * h * nc, pos).astype(np.float32).reshape(h, w, nc)[::-1]
    return np.ascontiguousarray(np.repeat(a, 3, axis=2) if nc == 1 else a)


def writePFM(path, rgb):
    """The counterpart of readPFM: float32 [H, W, 3] with row 0 = the top row, as a little-endian colour .pfm (the file stores the
    bottom row first).  readPFM(writePFM(x)) returns x bit for bit."""
    a = np.asarray(rgb, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("writePFM: an image of shape [H, W, 3], got %s" % (a.shape,))
    with open(path, "wb") as fh:
        fh.write(b"PF\n%d %d\n-1.0\n" % (a.shape[1], a.shape[0]))
        fh.write(np.ascontiguousarray(a[::-1]).astype("<f4").tobytes())


def loadEnvironment(path):
    """An environment map file by its suffix (.hdr / .pfm): float32 [H, W, 3], row 0 = the +Y pole."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".hdr":
        return readHDR(path)
    if ext == ".pfm":
        return readPFM(path)
    raise ValueError("%s: unknown environment map format (.hdr or .pfm)" % path)


def setEnvironment(state, image_or_path=None, scale=1.0):
    """Environment lighting (include/acgpt.h pt_set_environment): a latitude-longitude map of linear radiance, [H, W, 3] with row 0 =
    the +Y pole, or a .hdr / .pfm path, seen by rays that leave the scene and, in light mode 1, importance-sampled as a light.
    scale: a number or an (r, g, b) triple.  None clears the map."""
    L = _native.hip()
    s = (float(scale),) * 3 if np.isscalar(scale) else tuple(float(v) for v in scale)
    if image_or_path is None:
        rc = L.pt_set_environment(state.context, None, 0, 0, _f3(s))
    else:
        img = loadEnvironment(image_or_path) if isinstance(image_or_path, (str, os.PathLike)) else image_or_path
        img = np.ascontiguousarray(np.asarray(img, dtype=np.float32))
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("setEnvironment: an image of shape [H, W, 3], got %s" % (img.shape,))
        rc = L.pt_set_environment(state.context, img.ctypes.data, img.shape[1], img.shape[0], _f3(s))
    _check(state.context, rc, "pt_set_environment")
    state.refreshAccumulationBuffer = True


def setMathMode(state, mode):
    """Arithmetic of the shading code (include/acgpt.h pt_set_math_mode).  "fast" / 1 (the default): what the reference's own build
    computes with (nvcc --use_fast_math, CMakeLists.txt:267): approximate reciprocal, square root, sine and cosine.  "ieee" / 0:
    correctly rounded division and square root and the C library's sincosf / acosf, the level the CPU oracle is written at."""
    m = {"ieee": _native.MATH_IEEE, "fast": _native.MATH_FAST}.get(mode, mode)
    _check(state.context, _native.hip().pt_set_math_mode(state.context, int(m)), "pt_set_math_mode")
    state._math_mode = int(m)
    state.refreshAccumulationBuffer = True


def getStats(state):
    s = Stats()
    _check(state.context, _native.hip().pt_get_stats(state.context, C.byref(s)), "pt_get_stats")
    return s


def getBvhInfo(state):
    b = BvhInfo()
    _check(state.context, _native.hip().pt_get_bvh_info(state.context, C.byref(b)), "pt_get_bvh_info")
    return b


UPDATE_MODES = {"refit": _native.UPDATE_REFIT, "rebuild": _native.UPDATE_REBUILD, "auto": _native.UPDATE_AUTO}


def updateVertices(state, verts, mode="refit"):
    """New vertex positions for the scene of the last buildTheAccelarationStructure (pt_update_vertices): index buffer and materials
    stay.  verts: float32 (n, 4) or flat n * 4 array (w ignored), or a CPU tensor of either, n the scene's vertex count.  mode "refit"
    keeps the tree's topology and refits its boxes, "rebuild" builds anew, "auto" refits and rebuilds if the tree got too much worse.
    Every image and query bit equals a fresh build's.  Refreshes state.params.handle; returns pt_update_info as a dict."""
    if mode not in UPDATE_MODES:
        raise ValueError("updateVertices: mode must be one of %s" % sorted(UPDATE_MODES))
    if hasattr(verts, "detach"):            # a torch tensor: host memory only (device-pointer input is not part of the ABI)
        if verts.device.type != "cpu":
            raise ValueError("updateVertices: vertices must be in host memory")
        verts = verts.detach().numpy()
    v = np.asarray(verts)
    if not ((v.ndim == 2 and v.shape[1] == 4) or (v.ndim == 1 and v.size % 4 == 0)) or v.size == 0:
        raise ValueError("updateVertices: expected an (n, 4) or flat n * 4 array, got shape %s" % (v.shape,))
    v = np.ascontiguousarray(v, np.float32)
    L = _native.hip()
    info = _native.UpdateInfo()
    _check(state.context, L.pt_update_vertices(state.context, v.ctypes.data, v.size // 4, UPDATE_MODES[mode], C.byref(info)),
           "updateVertices")
    state.params.handle = L.pt_scene_handle(state.context)
    state._scene_verts = v.reshape(-1, 4).copy()
    state._verts_serial += 1
    return {"ms": info.ms, "area_ratio": info.area_ratio, "rebuilt": bool(info.rebuilt)}


def updateMaterials(state, materials=None, material_ids=None):
    """A new material table and/or assignment for the scene of the last buildTheAccelarationStructure (pt_update_materials): the
    vertices, the index buffer and the tree stay.  materials: the whole new table — TinyObjWrapper.getMaterials()' array or a list of
    Material —, None for the current one.  material_ids: one id per triangle in the scene's order, a uint32-valued integer array
    (NumPy or a CPU tensor), None to keep every triangle's.  Every image and query bit equals a fresh build's with the new materials.
    Refreshes state.params.handle; returns pt_update_info as a dict.  The accumulation is left as it is: restart it
    (state.params.currentFrameIdx = 0), as after updateVertices.  A TemporalHistory starts anew after the call."""
    if materials is None and material_ids is None:
        raise ValueError("updateMaterials: give materials, material_ids or both")
    if materials is None:
        mats = getattr(state, "_materials", None)
        if mats is None:
            raise ValueError("updateMaterials: no scene (buildTheAccelarationStructure first)")
    elif isinstance(materials, C.Array) and materials._type_ is Material:
        mats = materials
    else:
        items = list(materials)
        if not all(isinstance(m, Material) for m in items):
            raise ValueError("updateMaterials: materials must be Material structures (pt_material)")
        mats = (Material * len(items))(*items)
    ids = None
    if material_ids is not None:
        if hasattr(material_ids, "detach"):     # a torch tensor: host memory only
            if material_ids.device.type != "cpu":
                raise ValueError("updateMaterials: material ids must be in host memory")
            material_ids = material_ids.detach().numpy()
        a = np.asarray(material_ids)
        if a.ndim != 1:
            raise ValueError("updateMaterials: expected a flat array of one id per triangle, got shape %s" % (a.shape,))
        if a.dtype.kind not in "iu":
            raise ValueError("updateMaterials: material ids must be integers, got %s" % a.dtype)
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("updateMaterials: material ids must fit uint32")
        ids = np.ascontiguousarray(a, np.uint32)
    L = _native.hip()
    info = _native.UpdateInfo()
    rc = L.pt_update_materials(state.context, C.addressof(mats) if len(mats) else None, len(mats),
                               ids.ctypes.data if ids is not None else None, ids.size if ids is not None else 0, C.byref(info))
    _check(state.context, rc, "updateMaterials")
    state.params.handle = L.pt_scene_handle(state.context)
    state._materials = mats
    state._mats_serial += 1
    return {"ms": info.ms, "area_ratio": info.area_ratio, "rebuilt": bool(info.rebuilt)}


def readAccumulation(state):
    """float32 [height, width, 4] copy of params.accumulationBuffer (row 0 = bottom)."""
    h, w = int(state.params.height), int(state.params.width)
    out = np.zeros((h, w, 4), np.float32)
    _check(state.context, _native.hip().pt_copy_to_host(state.context, out.ctypes.data, state.params.accumulationBuffer, out.nbytes),
           "readAccumulation")
    return out


def _device_buffers(state, count, nbytes):
    L = _native.hip()
    out = []
    try:
        for _ in range(count):
            p = C.c_void_p()
            _check(state.context, L.pt_device_malloc(state.context, C.byref(p), nbytes), "device alloc")
            out.append(p.value)
    except Exception:
        _free_device_buffers(state, out)
        raise
    return out


def _free_device_buffers(state, ptrs):
    for p in ptrs:
        _native.hip().pt_device_free(state.context, p)


def _read_image(state, ptr):
    h, w = int(state.params.height), int(state.params.width)
    out = np.zeros((h, w, 4), np.float32)
    _check(state.context, _native.hip().pt_copy_to_host(state.context, out.ctypes.data, ptr, out.nbytes), "copy to host")
    return out


def _source_image(state, image, bufs, what):
    """The device pointer behind the `image` argument of `what`: None is the state's accumulation buffer, a float32 [height, width, 4]
    array is uploaded into a new buffer appended to bufs (the caller frees those), anything else is a device pointer."""
    if image is None:
        return state.params.accumulationBuffer
    if not isinstance(image, np.ndarray):
        return int(image)
    h, w = int(state.params.height), int(state.params.width)
    if image.shape != (h, w, 4):
        raise ValueError("%s: an image of shape %s, got %s" % (what, (h, w, 4), image.shape))
    a = np.ascontiguousarray(image, np.float32)
    bufs += _device_buffers(state, 1, a.nbytes)
    _check(state.context, _native.hip().pt_copy_to_device(state.context, bufs[-1], a.ctypes.data, a.nbytes), "copy to device")
    return bufs[-1]


def renderFeatures(state):
    """First-hit feature buffers of the current camera (include/acgpt.h pt_render_features), float32 [height, width, 4] each (row 0 =
    bottom): albedo_prim = diffuse colour + triangle index as uint32 bits (0xFFFFFFFF on a miss), normal_depth = camera-facing unit
    normal + hit distance (-1 on a miss)."""
    nbytes = int(state.params.width) * int(state.params.height) * 16
    bufs = _device_buffers(state, 2, nbytes)
    try:
        _check(state.context, _native.hip().pt_render_features(state.context, C.byref(state.params), bufs[0], bufs[1]), "pt_render_features")
        return _read_image(state, bufs[0]), _read_image(state, bufs[1])
    finally:
        _free_device_buffers(state, bufs)


HIT_DTYPE = np.dtype([("t", np.float32), ("prim", np.uint32), ("uv", np.float32, 2), ("normal", np.float32, 3), ("material", np.uint32)])      # pt_hit
assert HIT_DTYPE.itemsize == 32


def _is_tensor(x):
    """A torch tensor, told without importing torch: only a caller that has one has paid for the import."""
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _tensor_records(what, state, x, width, noun, layout=""):
    """The refusals of a tensor of query records: on the context's device, float32, (n, width), contiguous.  layout: what the shape's
    message adds behind "tensor".  Returns n."""
    import torch
    if x.device.type != "cuda" or x.device.index != state._device:
        raise PathTracerError("%s: the %s are on %s, the context is on cuda:%d" % (what, noun, x.device, state._device))
    if x.dtype != torch.float32:
        raise PathTracerError("%s: the %s must be float32, got %s" % (what, noun, x.dtype))
    if x.dim() != 2 or x.shape[1] != width:
        raise PathTracerError("%s: expected an (n, %d) tensor%s, got shape %s" % (what, width, layout, tuple(x.shape)))
    if not x.is_contiguous():
        raise PathTracerError("%s: the %s must be contiguous (nothing is copied)" % (what, noun))
    return int(x.shape[0])


def _host_call(state, ins, outs, call):
    """The round trip of host arrays: a device buffer per array of ins and of outs, the ins uploaded, call(*device pointers) in that
    order, the outs downloaded, everything freed whatever happens.  An output that is None or holds nothing gets no buffer and goes
    in as a null pointer.  Nothing happens where the first input holds no record."""
    if ins and not ins[0].shape[0]:
        return
    L = _native.hip()
    bufs, ptrs = [], []
    try:
        for a in list(ins) + list(outs):
            if a is not None and a.nbytes:
                bufs += _device_buffers(state, 1, a.nbytes)
            ptrs.append(bufs[-1] if a is not None and a.nbytes else None)
        for a, d in zip(ins, ptrs):
            _check(state.context, L.pt_copy_to_device(state.context, d, a.ctypes.data, a.nbytes), "copy to device")
        call(*ptrs)
        for a, d in zip(outs, ptrs[len(ins):]):
            if d is not None:
                _check(state.context, L.pt_copy_to_host(state.context, a.ctypes.data, d, a.nbytes), "copy to host")
    finally:
        _free_device_buffers(state, bufs)


def _tensor_call(x, outs, call):
    """The call on a tensor of records: the outputs allocated on its device ((shape, torch dtype name) each, or None), torch's current
    stream synchronised once — the records' producer and the allocations; the call returns synchronised —, call(pointers) with null for
    what holds nothing.  Returns the outputs."""
    import torch
    with torch.cuda.device(x.device):
        got = [None if o is None else torch.empty(o[0], dtype=getattr(torch, o[1]), device=x.device) for o in outs]
        torch.cuda.current_stream().synchronize()
    call(*[t.data_ptr() if t is not None and t.numel() else None for t in [x] + got])
    return got


_TENSOR_DTYPE = {np.dtype(np.float32): "float32", np.dtype(np.uint32): "int32", np.dtype(np.uint8): "uint8"}


def _query(state, symbol, recs, outs, *scalars):
    """symbol(context, records, n, *scalars, *outputs) on records that are a checked tensor or an (n, w) float32 array.  outs: (row
    shape, numpy dtype[, what an array holds before the call: 0]) per output, None for one the caller does not ask for.  Returns the
    outputs: tensors for a tensor (uint32 as int32), arrays for an array."""
    n = int(recs.shape[0])
    fn = getattr(_native.hip(), symbol)

    def call(d_recs, *d_outs):
        _check(state.context, fn(state.context, d_recs, n, *(scalars + d_outs)), symbol)
    if _is_tensor(recs):
        return _tensor_call(recs, [None if o is None else ((n,) + o[0], _TENSOR_DTYPE[np.dtype(o[1])]) for o in outs], call)
    got = [None if o is None else np.full((n,) + o[0], o[2] if len(o) > 2 else 0, o[1]) for o in outs]
    _host_call(state, [recs], got, call)
    return got


# The columns of the 32- and 48-byte records the queries write, per layout: (key, first float, floats, whole numbers).  Both the
# arrays and the tensor views of a result come from these, off one float32 array or tensor whose last axis is the record.
_HIT_COLUMNS = (("t", 0, 1, False), ("prim", 1, 1, True), ("uv", 2, 2, False), ("normal", 4, 3, False), ("material", 7, 1, True))                                # pt_hit
_MULTI_COLUMNS = (("t", 0, 1, False), ("prim", 1, 1, True), ("u", 2, 1, False), ("v", 3, 1, False), ("normal", 4, 3, False), ("material", 7, 1, True))           # pt_hit, uv apart
_NEAREST_COLUMNS = (("distance", 0, 1, False), ("prim", 1, 1, True), ("u", 2, 1, False), ("v", 3, 1, False), ("point", 4, 3, False), ("material", 7, 1, True))    # pt_nearest
_SEGMENT_COLUMNS = (("distance", 0, 1, False), ("prim", 1, 1, True), ("s", 2, 1, False), ("feature", 3, 1, False), ("point", 4, 3, False), ("material", 7, 1, True))      # pt_segment_hit
_SWEEP_COLUMNS = (("t", 0, 1, False), ("prim", 1, 1, True), ("u", 2, 1, False), ("v", 3, 1, False), ("point", 4, 3, False), ("material", 7, 1, True))            # pt_sweep_hit
_CAPSULE_CAST_COLUMNS = (("t", 0, 1, False), ("prim", 1, 1, True), ("s", 2, 1, False), ("feature", 3, 1, False), ("point", 4, 3, False), ("material", 7, 1, True))        # pt_capsule_cast_hit
_BOX_CAST_COLUMNS = (("t", 0, 1, False), ("prim", 1, 1, True), ("feature", 2, 1, False), ("material", 3, 1, True), ("normal", 4, 3, False), ("point", 8, 3, False))      # pt_box_cast_hit
_TRIANGLE_DISTANCE_COLUMNS = (("distance", 0, 1, False), ("prim", 1, 1, True), ("feature", 2, 1, False), ("material", 3, 1, True), ("on_query", 4, 3, False),
                              ("point", 8, 3, False))                                                                                                           # pt_triangle_distance_hit
_TRIANGLE_CAST_COLUMNS = (("t", 0, 1, False), ("prim", 1, 1, True), ("feature", 2, 1, False), ("query_triangle", 3, 1, True), ("point", 4, 3, False),
                          ("material", 7, 1, True))                                                                                                             # pt_triangle_cast_hit


def _columns(out, columns):
    """The dict of a result from the float32 records out[..., w]: views of a tensor (whole numbers as int32), contiguous arrays of an
    array (whole numbers as uint32)."""
    tensor = _is_tensor(out)
    if tensor:
        import torch
    got = {}
    for key, first, width, whole in columns:
        col = out[..., first] if width == 1 else out[..., first:first + width]
        if tensor:
            got[key] = col.view(torch.int32) if whole else col
        else:
            got[key] = np.ascontiguousarray(col).view(np.uint32) if whole else np.ascontiguousarray(col)
    return got


def _as_bool(out):
    """the bytes of an any-hit answer as bools, tensor or array"""
    if _is_tensor(out):
        import torch
        return out.view(torch.bool)
    return out.view(np.bool_)


def _records_or_hit(state, recs, any_hit, symbol, any_symbol, width, columns):
    """The calls with an any-hit twin: any_symbol and a bool per record, or symbol, `width` floats per record and their columns."""
    if any_hit:
        return _as_bool(_query(state, any_symbol, recs, [((), np.uint8)])[0])
    return _columns(_query(state, symbol, recs, [((width,), np.float32)])[0], columns)


def _list_or_counts(state, symbol, recs, k, counts):
    """The calls that list up to k triangle indices per record and count them: {"prim", and "count" when asked}."""
    out, cnt = _query(state, symbol, recs, [((k,), np.uint32, 0xFFFFFFFF), ((), np.uint32) if counts else None], k)
    got = {"prim": out}
    if counts:
        got["count"] = cnt
    return got


def queryRays(state, rays, any_hit=False):
    """Rays against the scene on the GPU (include/acgpt.h pt_query_closest / pt_query_any).  rays: (n, 8) float32 records of origin xyz,
    direction xyz (not normalised; t is in units of its length), tmin, tmax (open interval; +inf allowed).

    A NumPy array (or anything np.asarray takes) goes to the device and the answer comes back: a dict of arrays t (n,) float32 (-1 on a
    miss), prim (n,) uint32 (the triangle's index in the scene's order, 0xFFFFFFFF on a miss), uv (n, 2) barycentrics of v1 and v2,
    normal (n, 3) unit geometric normal facing the ray's origin, material (n,) uint32 — or, with any_hit, a bool array: is anything hit
    inside the interval.

    A torch tensor must be float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in, and
    the answer is torch tensors on that device: views of one (n, 8) float32 tensor, prim and material as int32 (-1 on a miss), or a
    bool tensor with any_hit.  torch's current stream is synchronised before the call, and the call returns synchronised."""
    if _is_tensor(rays):
        _tensor_records("queryRays", state, rays, 8, "rays")
        r = rays
    else:
        r = np.asarray(rays)
        if r.ndim != 2 or r.shape[1] != 8:
            raise PathTracerError("queryRays: expected an (n, 8) array, got shape %s" % (r.shape,))
        if r.dtype.kind not in "fiu":
            raise PathTracerError("queryRays: the rays must be numbers, got %s" % r.dtype)
        r = np.ascontiguousarray(r, np.float32)
    return _records_or_hit(state, r, any_hit, "pt_query_closest", "pt_query_any", 8, _HIT_COLUMNS)


# ------------------------------------------------------------------ the first hits in order ----
MULTI_KEYS = ("t", "prim", "u", "v", "normal", "material")


def _multi_args(what, max_hits, counts):
    try:
        k = int(max_hits)
    except (TypeError, ValueError):
        raise PathTracerError("%s: max_hits is a number 0..%d, got %r" % (what, _native.QUERY_MULTI_MAX, max_hits))
    if k != max_hits or k < 0 or k > _native.QUERY_MULTI_MAX:
        raise PathTracerError("%s: max_hits must be 0..%d, got %r" % (what, _native.QUERY_MULTI_MAX, max_hits))
    if k == 0 and not counts:
        raise PathTracerError("%s: max_hits = 0 leaves only the counts to ask for (counts=True)" % what)
    return k


def queryRaysMulti(state, rays, max_hits=4, counts=False):
    """The first max_hits surfaces each ray goes through, in order, and how many it crosses in all (include/acgpt.h pt_query_multi).
    rays: queryRays' (n, 8) float32 records.  max_hits: 0..8.  counts: also the total number of triangles the ray hits inside its
    interval, not clamped to max_hits; it makes the walk visit everything the ray crosses.  max_hits=0, counts=True asks for the
    counts alone.

    A NumPy array (or anything np.asarray takes) goes to the device and the answer comes back: a dict of (n, max_hits) arrays t float32
    (-1 past the ray's last hit), prim uint32 (0xFFFFFFFF there), u, v the barycentrics of v1 and v2, normal (n, max_hits, 3) facing the
    ray's origin, material uint32, plus count (n,) uint32 when asked.  Column j is the ray's j-th hit in ascending (t, prim); column 0
    is queryRays' answer.  The counts are the triangle test's and not watertight: a ray through an edge or vertex that triangles share
    may count that crossing 0, 1 or more times.

    A torch tensor must be float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in, and
    the answer is torch tensors on that device: views of one (n, max_hits, 8) float32 tensor, prim and material as int32 (-1 past the
    last hit), count int32.  torch's current stream is synchronised before the call, and the call returns synchronised."""
    k = _multi_args("queryRaysMulti", max_hits, counts)
    if _is_tensor(rays):
        _tensor_records("queryRaysMulti", state, rays, 8, "rays")
        r = rays
    else:
        r = np.asarray(rays)
        if r.ndim != 2 or r.shape[1] != 8:
            raise PathTracerError("queryRaysMulti: expected an (n, 8) array, got shape %s" % (r.shape,))
        if r.dtype.kind not in "fiu":
            raise PathTracerError("queryRaysMulti: the rays must be numbers, got %s" % r.dtype)
        r = np.ascontiguousarray(r, np.float32)
    out, cnt = _query(state, "pt_query_multi", r, [((k, 8), np.float32), ((), np.uint32) if counts else None], k)
    got = _columns(out, _MULTI_COLUMNS)
    if counts:
        got["count"] = cnt
    return got


INSIDE_DIRECTIONS = ((0.5377, 0.2673, 0.7996), (-0.6124, 0.7071, 0.3536), (0.3015, -0.9045, 0.3015))


def _inside_rays(what, points, directions):
    """The (n * m, 8) float32 rays of pointsInside, point-major: ray i * m + j leaves point i along direction j, tmin 0, tmax +inf."""
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise PathTracerError("%s: expected (n, 3) points, got shape %s" % (what, p.shape))
    if p.dtype.kind not in "fiu":
        raise PathTracerError("%s: the points must be numbers, got %s" % (what, p.dtype))
    d = np.asarray(INSIDE_DIRECTIONS if directions is None else directions)
    if d.ndim != 2 or d.shape[1] != 3 or d.dtype.kind not in "fiu":
        raise PathTracerError("%s: expected (m, 3) directions, got %r" % (what, directions))
    if d.shape[0] % 2 != 1:
        raise PathTracerError("%s: an odd number of directions makes a majority, got %d" % (what, d.shape[0]))
    d = d.astype(np.float32)
    if not (np.isfinite(d).all() and (d != 0).any(axis=1).all()):
        raise PathTracerError("%s: every direction must be finite and not zero" % what)
    n, m = p.shape[0], d.shape[0]
    if n * m > 0x7FFFFFFF:
        raise PathTracerError("%s: %d points x %d directions is more than 2^31 - 1 rays" % (what, n, m))
    rays = np.empty((n, m, 8), np.float32)
    rays[:, :, 0:3] = p.astype(np.float32)[:, None, :]
    rays[:, :, 3:6] = d[None, :, :]
    rays[:, :, 6] = 0.0
    rays[:, :, 7] = np.inf
    return rays.reshape(n * m, 8), n, m


def pointsInside(state, points, directions=None, return_counts=False, method="parity", beta=_native.WINDING_BETA_DEFAULT, threshold=0.5):
    """Which of the points lie inside the scene's surface, by the parity of crossings (queryRaysMulti, counts alone): one ray per point
    and direction with tmin 0 and tmax +inf, a point is inside by one ray if the ray crosses an odd number of triangles, and inside if
    most of its rays say so.  directions: an odd number of them, (m, 3); by default three generic ones, INSIDE_DIRECTIONS.  Returns a
    bool array (n,), and with return_counts also the crossing counts, uint32 (n, m).

    The answer means something only where the mesh is closed: a ray that leaves through a hole counts one crossing too few.  The Cornell
    box's shell is open to the front.  The counts are not watertight either (include/acgpt.h): a ray through a shared edge or vertex
    may miscount, which is what the vote over several generic directions is for.

    method="winding" asks the generalised winding number instead (queryWinding with beta): inside where w > threshold.  It stays
    usable on a mesh with holes, where a hole of solid angle omega lowers the inside value by omega / 4 pi; directions is not used,
    and return_counts returns the winding numbers, float32 (n,), in place of the counts."""
    if method == "winding":
        p = np.asarray(points)
        if p.ndim != 2 or p.shape[1] != 3:
            raise PathTracerError("pointsInside: expected (n, 3) points, got shape %s" % (p.shape,))
        try:
            thr = float(threshold)
        except (TypeError, ValueError):
            raise PathTracerError("pointsInside: threshold is one number, got %r" % (threshold,))
        if thr != thr:
            raise PathTracerError("pointsInside: threshold is a NaN")
        w = queryWinding(state, p, beta)
        inside = w > np.float32(thr)
        return (inside, w) if return_counts else inside
    if method != "parity":
        raise PathTracerError("pointsInside: method is \"parity\" or \"winding\", got %r" % (method,))
    rays, n, m = _inside_rays("pointsInside", points, directions)
    cnt = queryRaysMulti(state, rays, max_hits=0, counts=True)["count"].reshape(n, m)
    inside = 2 * ((cnt & 1) != 0).sum(axis=1) > m
    return (inside, cnt) if return_counts else inside


# ------------------------------------------------------------------ closest point ----
NEAREST_DTYPE = np.dtype([("distance", np.float32), ("prim", np.uint32), ("u", np.float32), ("v", np.float32), ("point", np.float32, 3), ("material", np.uint32)])      # pt_nearest
assert NEAREST_DTYPE.itemsize == 32


def queryNearest(state, points, max_radius=float("inf")):
    """The closest surface point of the scene on the GPU to each query point (include/acgpt.h pt_query_nearest).

    A NumPy array (or anything np.asarray takes) of shape (n, 3), or (n, 4) with a search radius per point in the fourth column — (n, 3)
    points all get max_radius —, goes to the device and the answer comes back: a dict of arrays distance (n,) float32 (-1 where nothing
    lies within the radius), prim (n,) uint32 (the triangle's index in the scene's order, 0xFFFFFFFF), u, v (n,) the weights of v1 and
    v2 at the closest point, point (n, 3) the closest point, material (n,) uint32.

    A torch tensor must be (n, 4) float32 {x, y, z, max_radius}, contiguous and on the context's device; nothing is copied, its data_ptr()
    goes straight in, and the answer is torch tensors on that device: views of one (n, 8) float32 tensor, prim and material as int32
    (-1 on a miss).  torch's current stream is synchronised before the call, and the call returns synchronised."""
    if _is_tensor(points):
        _tensor_records("queryNearest", state, points, 4, "points", " {x, y, z, max_radius}")
        q = points
    else:
        p = np.asarray(points)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise PathTracerError("queryNearest: expected an (n, 3) or (n, 4) array, got shape %s" % (p.shape,))
        if p.dtype.kind not in "fiu":
            raise PathTracerError("queryNearest: the points must be numbers, got %s" % p.dtype)
        if p.shape[1] == 3:
            radius = float(max_radius)
            if not radius >= 0.0:
                raise PathTracerError("queryNearest: max_radius must be non-negative, got %r" % (max_radius,))
            q = np.empty((p.shape[0], 4), np.float32)
            q[:, 0:3] = p
            q[:, 3] = radius
        else:
            q = np.ascontiguousarray(p, np.float32)
    return _columns(_query(state, "pt_query_nearest", q, [((8,), np.float32)])[0], _NEAREST_COLUMNS)


def distanceFieldPoints(resolution, lo, hi):
    """Cell centres of an (nz, ny, nx) grid over the box [lo, hi], float32 (nz * ny * nx, 3), x fastest: centre i of an axis is
    lo + (i + 0.5) * ((hi - lo) / n), computed in float64 and rounded once."""
    try:
        nz, ny, nx = (int(r) for r in resolution)
    except (TypeError, ValueError):
        raise PathTracerError("bakeDistanceField: resolution is (nz, ny, nx), got %r" % (resolution,))
    if min(nz, ny, nx) < 1 or nz * ny * nx > 0x7FFFFFFF:
        raise PathTracerError("bakeDistanceField: every side of the grid must be at least 1 and the grid at most 2^31 - 1 cells, got %r" % (resolution,))
    lo, hi = np.asarray(lo, np.float64).reshape(-1), np.asarray(hi, np.float64).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise PathTracerError("bakeDistanceField: bounds must be finite (lo xyz, hi xyz) with hi >= lo, got %r, %r" % (lo.tolist(), hi.tolist()))
    axes = [lo[k] + (np.arange(m) + 0.5) * ((hi[k] - lo[k]) / m) for k, m in ((0, nx), (1, ny), (2, nz))]
    pts = np.empty((nz, ny, nx, 3), np.float32)
    pts[..., 0] = axes[0][None, None, :]
    pts[..., 1] = axes[1][None, :, None]
    pts[..., 2] = axes[2][:, None, None]
    return pts.reshape(-1, 3)


def bakeDistanceField(state, resolution, bounds=None, max_radius=float("inf"), return_prims=False, signed=False):
    """The distance from the centre of every cell of an (nz, ny, nx) grid to the scene's surface (queryNearest on
    distanceFieldPoints): float32 [nz, ny, nx], -1 where nothing lies within max_radius.  bounds: (lo xyz, hi xyz) of the grid, the
    scene box if not given.  The points go to the device x fastest, so the 64 queries of a wave are neighbours.  return_prims: also the
    closest triangle's index per cell, uint32 [nz, ny, nx] (0xFFFFFFFF where nothing is found).  The distance is unsigned unless
    signed=True, which negates it at the cells that pointsInside calls inside (its default directions; closed meshes only), and leaves
    the -1 of a cell that found nothing as it is.  signed="winding" takes the sign from the generalised winding number instead
    (pointsInside(method="winding"), its default beta and threshold), which holds on meshes with holes."""
    if signed not in (False, True, "winding"):
        raise PathTracerError("bakeDistanceField: signed is False, True or \"winding\", got %r" % (signed,))
    if bounds is None:
        info = getBvhInfo(state)
        lo, hi = [float(x) for x in info.scene_lo], [float(x) for x in info.scene_hi]
    else:
        try:
            lo, hi = bounds
        except (TypeError, ValueError):
            raise PathTracerError("bakeDistanceField: bounds is (lo xyz, hi xyz), got %r" % (bounds,))
    pts = distanceFieldPoints(resolution, lo, hi)
    got = queryNearest(state, pts, max_radius)
    shape = tuple(int(r) for r in resolution)
    dist = got["distance"].reshape(shape)
    if signed:
        inside = (pointsInside(state, pts, method="winding") if signed == "winding" else pointsInside(state, pts)).reshape(shape) & (dist >= 0.0)
        dist = np.where(inside, -dist, dist)
    return (dist, got["prim"].reshape(shape)) if return_prims else dist


# ------------------------------------------------------------------ generalised winding numbers ----
def _winding_beta(beta):
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise PathTracerError("queryWinding: beta is one number, got %r" % (beta,))
    if not b >= 1.0:
        raise PathTracerError("queryWinding: beta must be at least 1 (inf: the exact sum), got %r" % (beta,))
    return b


def queryWinding(state, points, beta=_native.WINDING_BETA_DEFAULT):
    """The generalised winding number of the scene's mesh at each point (include/acgpt.h pt_query_winding): 1 inside and 0 outside a
    closed, outward-wound mesh, degrading smoothly where the mesh has holes, so that w > 0.5 stays an inside test.  beta >= 1 is the
    accuracy knob: a subtree further away than beta times its radius is taken as one dipole; inf is the exact sum over every
    triangle.

    A NumPy array (or anything np.asarray takes) of shape (n, 3), or (n, 4) whose fourth column is ignored (queryNearest's points
    serve both), goes to the device and float32 (n,) comes back; a point with a non-finite coordinate gets a NaN.  A torch tensor
    must be (n, 4) float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in, and the answer
    is a float32 tensor on that device.  torch's current stream is synchronised before the call, and the call returns synchronised."""
    b = _winding_beta(beta)
    if _is_tensor(points):
        _point_tensor("queryWinding", state, points)
        q = points
    else:
        p = np.asarray(points)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise PathTracerError("queryWinding: expected an (n, 3) or (n, 4) array, got shape %s" % (p.shape,))
        if p.dtype.kind not in "fiu":
            raise PathTracerError("queryWinding: the points must be numbers, got %s" % p.dtype)
        q = np.zeros((p.shape[0], 4), np.float32)
        q[:, 0:3] = p[:, 0:3]
    return _query(state, "pt_query_winding", q, [((), np.float32)], b)[0]


def getWindingInfo(state):
    """What pt_query_winding holds on the device for the scene: {"built": bool, "bytes": int, "n_nodes": int}.  The moments are built on
    the first queryWinding after the scene or its vertices changed and are not part of getBvhInfo().device_bytes."""
    w = _native.WindingInfo()
    _check(state.context, _native.hip().pt_get_winding_info(state.context, C.byref(w)), "pt_get_winding_info")
    return {"built": bool(w.built), "bytes": int(w.bytes), "n_nodes": int(w.n_nodes)}


# ------------------------------------------------------------------ the K closest triangles, anything within a radius ----
def _nearest_k_args(what, k, counts):
    try:
        kk = int(k)
    except (TypeError, ValueError):
        raise PathTracerError("%s: k is a number 0..%d, got %r" % (what, _native.QUERY_NEAREST_MAX, k))
    if kk != k or kk < 0 or kk > _native.QUERY_NEAREST_MAX:
        raise PathTracerError("%s: k must be 0..%d, got %r" % (what, _native.QUERY_NEAREST_MAX, k))
    if kk == 0 and not counts:
        raise PathTracerError("%s: k = 0 leaves only the counts to ask for (counts=True)" % what)
    return kk


def _point_records(what, points, max_radius):
    """(n, 4) float32 {x, y, z, max_radius} from an (n, 3) array and one radius, or the (n, 4) array itself"""
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[1] not in (3, 4):
        raise PathTracerError("%s: expected an (n, 3) or (n, 4) array, got shape %s" % (what, p.shape))
    if p.dtype.kind not in "fiu":
        raise PathTracerError("%s: the points must be numbers, got %s" % (what, p.dtype))
    if p.shape[1] == 4:
        return np.ascontiguousarray(p, np.float32)
    try:
        radius = float(max_radius)
    except (TypeError, ValueError):
        raise PathTracerError("%s: the radius is one number, got %r" % (what, max_radius))
    if not radius >= 0.0:
        raise PathTracerError("%s: the radius must be non-negative, got %r" % (what, max_radius))
    q = np.empty((p.shape[0], 4), np.float32)
    q[:, 0:3] = p
    q[:, 3] = radius
    return q


def _point_tensor(what, state, points):
    return _tensor_records(what, state, points, 4, "points", " {x, y, z, max_radius}")


def queryNearestK(state, points, k=4, max_radius=float("inf"), counts=False):
    """The k closest triangles of the scene on the GPU to each query point, in order, and how many lie within the radius
    (include/acgpt.h pt_query_nearest_k).  points: queryNearest's — (n, 3) with max_radius for all, or (n, 4) with a radius per point
    in the fourth column.  k: 0..8.  counts: also the number of triangles within the radius, not clamped to k; it makes the walk
    visit everything the ball holds.  k=0, counts=True asks for the counts alone.

    A NumPy array (or anything np.asarray takes) goes to the device and the answer comes back: a dict of (n, k) arrays of
    queryNearest's fields — distance float32 (-1 past the point's last candidate), prim uint32 (0xFFFFFFFF there), u, v, point
    (n, k, 3), material uint32 —, plus count (n,) uint32 when asked.  Column j is the point's j-th candidate in ascending (squared
    distance, prim); column 0 is queryNearest's answer.

    A torch tensor must be (n, 4) float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in,
    and the answer is torch tensors on that device: views of one (n, k, 8) float32 tensor, prim and material as int32 (-1 past the
    last candidate), count int32.  torch's current stream is synchronised before the call, and the call returns synchronised."""
    kk = _nearest_k_args("queryNearestK", k, counts)
    if _is_tensor(points):
        _point_tensor("queryNearestK", state, points)
        q = points
    else:
        q = _point_records("queryNearestK", points, max_radius)
    out, cnt = _query(state, "pt_query_nearest_k", q, [((kk, 8), np.float32), ((), np.uint32) if counts else None], kk)
    got = _columns(out, _NEAREST_COLUMNS)
    if counts:
        got["count"] = cnt
    return got


def queryWithinAny(state, points, radius=None):
    """Whether anything of the scene lies within the radius of each point (include/acgpt.h pt_query_within_any): the clearance check
    of a spherical probe, answered at the first triangle found instead of by a search for the closest.  points: (n, 3) with radius
    for all — a number >= 0, required —, or (n, 4) with a radius per point in the fourth column (radius stays None).  Returns (n,)
    bool.  A torch tensor must be (n, 4) float32, contiguous and on the context's device; nothing is copied and the answer is a torch
    bool tensor on that device."""
    if _is_tensor(points):
        if radius is not None:
            raise PathTracerError("queryWithinAny: a tensor carries its radii in the fourth column; radius must stay None")
        _point_tensor("queryWithinAny", state, points)
        q = points
    else:
        p = np.asarray(points)
        if p.ndim == 2 and p.shape[1] == 3 and radius is None:
            raise PathTracerError("queryWithinAny: (n, 3) points need a radius")
        if p.ndim == 2 and p.shape[1] == 4 and radius is not None:
            raise PathTracerError("queryWithinAny: (n, 4) points carry their radii in the fourth column; radius must stay None")
        q = _point_records("queryWithinAny", p, radius)
    return _query(state, "pt_query_within_any", q, [((), np.uint8)])[0] != 0


def _sphere_contact_args(centres, radius, max_contacts):
    c = np.asarray(centres)
    if c.ndim != 2 or c.shape[1] != 3:
        raise PathTracerError("sphereContacts: expected (n, 3) centres, got shape %s" % (c.shape,))
    if c.dtype.kind not in "fiu":
        raise PathTracerError("sphereContacts: the centres must be numbers, got %s" % c.dtype)
    r = np.asarray(radius)
    if r.dtype.kind not in "fiu" or r.shape not in ((), (c.shape[0],)):
        raise PathTracerError("sphereContacts: radius is one number or one per ball, got %r" % (radius,))
    r = np.broadcast_to(r.astype(np.float32), (c.shape[0],))
    if not (np.isfinite(r).all() and (r >= 0).all()):
        raise PathTracerError("sphereContacts: every radius must be finite and non-negative")
    try:
        k = int(max_contacts)
    except (TypeError, ValueError):
        raise PathTracerError("sphereContacts: max_contacts is a number 1..%d, got %r" % (_native.QUERY_NEAREST_MAX, max_contacts))
    if k != max_contacts or k < 1 or k > _native.QUERY_NEAREST_MAX:
        raise PathTracerError("sphereContacts: max_contacts must be 1..%d, got %r" % (_native.QUERY_NEAREST_MAX, max_contacts))
    q = np.empty((c.shape[0], 4), np.float32)
    q[:, 0:3] = c
    q[:, 3] = r
    return q, k


def sphereContacts(state, centres, radius, max_contacts=8):
    """The contact manifold of balls against the scene: every triangle within radius of a centre is a contact, the closest
    max_contacts (1..8) of them are listed (queryNearestK with counts).  centres: (n, 3); radius: one number or (n,).  Returns a dict
    of arrays, one row per ball and one column per contact, closest first: point (n, k, 3) float32 the point on the mesh, normal
    (n, k, 3) the unit direction from it to the centre (zero where the centre lies on the triangle, and past the last contact),
    penetration (n, k) float32 = radius - distance (>= 0 at a contact up to the rounding of the difference; NaN past the last
    contact), prim and material (n, k) uint32 (0xFFFFFFFF past the last contact), count (n,) uint32 the number of triangles within
    the radius: count > max_contacts flags a truncated manifold.  Triangles in one plane give one contact each: merge them by
    normal if the solver wants one contact per wall."""
    q, k = _sphere_contact_args(centres, radius, max_contacts)
    got = queryNearestK(state, q, k=k, counts=True)
    found = got["prim"] != 0xFFFFFFFF
    dist = got["distance"]
    away = q[:, None, 0:3] - got["point"]
    with np.errstate(all="ignore"):
        normal = np.where((found & (dist > 0))[..., None], away / dist[..., None], np.float32(0.0)).astype(np.float32)
    penetration = np.where(found, q[:, None, 3] - dist, np.float32(np.nan)).astype(np.float32)
    return {"point": got["point"], "normal": normal, "penetration": penetration, "prim": got["prim"], "material": got["material"], "count": got["count"]}


# ------------------------------------------------------------------ segment to mesh ----
SEGMENT_HIT_DTYPE = np.dtype([("distance", np.float32), ("prim", np.uint32), ("s", np.float32), ("feature", np.float32), ("point", np.float32, 3), ("material", np.uint32)])      # pt_segment_hit
assert SEGMENT_HIT_DTYPE.itemsize == 32


def _segment_records(what, segments, max_radius):
    """(n, 8) float32 {p0, max_radius | p1, 0} from an (n, 6) array {p0, p1} and one radius, or the (n, 8) array itself"""
    g = np.asarray(segments)
    if g.ndim != 2 or g.shape[1] not in (6, 8):
        raise PathTracerError("%s: expected an (n, 6) or (n, 8) array, got shape %s" % (what, g.shape))
    if g.dtype.kind not in "fiu":
        raise PathTracerError("%s: the segments must be numbers, got %s" % (what, g.dtype))
    if g.shape[1] == 8:
        return np.ascontiguousarray(g, np.float32)
    radius = float(max_radius)
    if not radius >= 0.0:
        raise PathTracerError("%s: max_radius must be non-negative, got %r" % (what, max_radius))
    q = np.zeros((g.shape[0], 8), np.float32)
    q[:, 0:3] = g[:, 0:3]
    q[:, 3] = radius
    q[:, 4:7] = g[:, 3:6]
    return q


def querySegments(state, segments, max_radius=float("inf")):
    """How far each line segment is from the scene on the GPU, and where the two come closest (include/acgpt.h pt_query_segments).

    A NumPy array (or anything np.asarray takes) of shape (n, 6) {p0 xyz, p1 xyz} — every segment gets max_radius — or (n, 8)
    {p0 xyz, max_radius, p1 xyz, ignored} goes to the device and the answer comes back: a dict of arrays distance (n,) float32 (0 where
    the segment passes through a triangle, -1 where nothing lies within the radius), prim (n,) uint32 (the triangle's index in the
    scene's order, 0xFFFFFFFF), s (n,) the parameter of the closest point on the segment (p0 + (p1 - p0) s), feature (n,) float32
    (0, 1: an end of the segment; 2, 3, 4: an edge of the triangle; 5: the segment crosses it), point (n, 3) the closest point on the
    triangle, material (n,) uint32.

    A torch tensor must be (n, 8) float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in,
    and the answer is torch tensors on that device: views of one (n, 8) float32 tensor, prim and material as int32 (-1 on a miss).
    torch's current stream is synchronised before the call, and the call returns synchronised."""
    if _is_tensor(segments):
        _tensor_records("querySegments", state, segments, 8, "segments", " {p0, max_radius, p1, ignored}")
        q = segments
    else:
        q = _segment_records("querySegments", segments, max_radius)
    return _columns(_query(state, "pt_query_segments", q, [((8,), np.float32)])[0], _SEGMENT_COLUMNS)


def capsuleClearance(state, p0, p1, radius):
    """The clearance of capsules with axes p0 -> p1, (n, 3) each, and radius (one number or (n,)) from the scene: querySegments with no
    limit on the distance.  Returns a dict: clearance (n,) float32 = distance - radius (negative: the capsule penetrates by that much;
    -radius where its axis passes through the surface; +inf for a scene without triangles), prim (n,) uint32, on_axis (n, 3) and
    on_mesh (n, 3) float32 the witness points — on_mesh - on_axis is the direction to push the mesh away in —, s (n,) and feature (n,)
    as querySegments gives them."""
    a, b = np.asarray(p0), np.asarray(p1)
    if a.ndim != 2 or a.shape[1] != 3 or b.shape != a.shape:
        raise PathTracerError("capsuleClearance: expected two (n, 3) arrays, got shapes %s and %s" % (a.shape, b.shape))
    if a.dtype.kind not in "fiu" or b.dtype.kind not in "fiu":
        raise PathTracerError("capsuleClearance: the end points must be numbers, got %s and %s" % (a.dtype, b.dtype))
    r = np.asarray(radius)
    if r.dtype.kind not in "fiu" or r.shape not in ((), (a.shape[0],)):
        raise PathTracerError("capsuleClearance: radius is one number or one per capsule, got %r" % (radius,))
    r = np.broadcast_to(r.astype(np.float32), (a.shape[0],))
    if not (np.isfinite(r).all() and (r >= 0).all()):
        raise PathTracerError("capsuleClearance: every radius must be finite and non-negative")
    a, b = a.astype(np.float32), b.astype(np.float32)
    got = querySegments(state, np.concatenate([a, b], axis=1))
    found = got["prim"] != 0xFFFFFFFF
    clearance = np.where(found, got["distance"] - r, np.float32(np.inf)).astype(np.float32)
    on_axis = (a + (b - a) * got["s"][:, None]).astype(np.float32)
    return {"clearance": clearance, "prim": got["prim"], "on_axis": on_axis, "on_mesh": got["point"], "s": got["s"], "feature": got["feature"]}


# ------------------------------------------------------------------ box overlap ----
def _overlap_args(what, max_prims, counts):
    try:
        k = int(max_prims)
    except (TypeError, ValueError):
        raise PathTracerError("%s: max_prims is a number 0..%d, got %r" % (what, _native.QUERY_OVERLAP_MAX, max_prims))
    if k != max_prims or k < 0 or k > _native.QUERY_OVERLAP_MAX:
        raise PathTracerError("%s: max_prims must be 0..%d, got %r" % (what, _native.QUERY_OVERLAP_MAX, max_prims))
    if k == 0 and not counts:
        raise PathTracerError("%s: max_prims = 0 leaves only the counts to ask for (counts=True)" % what)
    return k


def _overlap_boxes(what, centres, half_extents):
    """The (n, 8) float32 records {cx, cy, cz, hx, hy, hz, 0, 0} of the NumPy arguments: (n, 8) records as they are, or (n, 3) centres
    with half extents that broadcast against them"""
    c = np.asarray(centres)
    if c.dtype.kind not in "fiu":
        raise PathTracerError("%s: the boxes must be numbers, got %s" % (what, c.dtype))
    if c.ndim == 2 and c.shape[1] == 8:
        if half_extents is not None:
            raise PathTracerError("%s: (n, 8) records carry their half extents; half_extents must be None" % what)
        return np.ascontiguousarray(c, np.float32)
    if c.ndim != 2 or c.shape[1] != 3:
        raise PathTracerError("%s: expected (n, 3) centres or (n, 8) records, got shape %s" % (what, c.shape))
    if half_extents is None:
        raise PathTracerError("%s: (n, 3) centres need half_extents" % what)
    h = np.asarray(half_extents)
    if h.dtype.kind not in "fiu":
        raise PathTracerError("%s: the half extents must be numbers, got %s" % (what, h.dtype))
    try:
        h = np.broadcast_to(h.astype(np.float32), c.shape)
    except ValueError:
        raise PathTracerError("%s: half_extents of shape %s do not broadcast against %s centres" % (what, h.shape, c.shape))
    if not (h >= 0.0).all():
        raise PathTracerError("%s: every half extent must be non-negative" % what)
    b = np.zeros((c.shape[0], 8), np.float32)
    b[:, 0:3] = c
    b[:, 3:6] = h
    return b


def _overlap_tensor(what, state, boxes, half_extents):
    if half_extents is not None:
        raise PathTracerError("%s: a tensor is (n, 8) records that carry their half extents; half_extents must be None" % what)
    return _tensor_records(what, state, boxes, 8, "boxes", " {cx, cy, cz, hx, hy, hz, 0, 0}")


def queryOverlap(state, centres, half_extents=None, max_prims=8, counts=True):
    """Which triangles of the scene on the GPU overlap each axis-aligned box (include/acgpt.h pt_query_overlap).  max_prims: 0..8, how
    many triangle indices to return per box; counts: also the number of overlapping triangles, not clamped to max_prims.  max_prims=0,
    counts=True asks for the counts alone.

    NumPy (or anything np.asarray takes): (n, 3) centres with half_extents (n, 3), (3,) or a number, broadcast; or (n, 8) records
    {cx, cy, cz, hx, hy, hz, 0, 0} with half_extents=None.  A half extent may be 0.  They go to the device and the answer comes back:
    a dict of prim (n, max_prims) uint32, the lowest indices among the overlapping triangles, ascending, 0xFFFFFFFF past the last one,
    and count (n,) uint32 when asked.

    A torch tensor must be (n, 8) float32 records, contiguous and on the context's device; nothing is copied, its data_ptr() goes
    straight in, and the answer is torch tensors on that device, prim and count as int32 (-1 past the last triangle).  torch's current
    stream is synchronised before the call, and the call returns synchronised."""
    k = _overlap_args("queryOverlap", max_prims, counts)
    if _is_tensor(centres):
        _overlap_tensor("queryOverlap", state, centres, half_extents)
        b = centres
    else:
        b = _overlap_boxes("queryOverlap", centres, half_extents)
    return _list_or_counts(state, "pt_query_overlap", b, k, counts)


def queryOverlapAny(state, centres, half_extents=None):
    """Does any triangle of the scene overlap each box (include/acgpt.h pt_query_overlap_any): queryOverlap's arguments, a bool array
    (n,), or a bool tensor for a tensor.  A box's walk ends at the first triangle it accepts."""
    if _is_tensor(centres):
        _overlap_tensor("queryOverlapAny", state, centres, half_extents)
        b = centres
    else:
        b = _overlap_boxes("queryOverlapAny", centres, half_extents)
    return _as_bool(_query(state, "pt_query_overlap_any", b, [((), np.uint8)])[0])


def _occupancy_frame(frame):
    """(rotation float32 (3, 3), translation float64 (3,), the 3 x 3 part in float64) of a 3 x 4 or 4 x 4 frame, local -> world"""
    try:
        f = np.asarray(frame, np.float64)
    except (TypeError, ValueError):
        f = np.zeros(0)
    if f.shape not in ((3, 4), (4, 4), (12,)) or not np.isfinite(f).all():
        raise PathTracerError("bakeOccupancy: frame is a finite 3 x 4 matrix [rotation | origin], local -> world, got %r" % (frame,))
    f = f.reshape(-1, 4)[:3]
    return f[:, :3].astype(np.float32), f[:, 3].copy(), f[:, :3].astype(np.float32).astype(np.float64)


def occupancyBoxes(resolution, lo, hi, frame=None):
    """The cells of an (nz, ny, nx) grid over the box [lo, hi] as (nz * ny * nx, 8) float32 box records, x fastest: the centres are
    distanceFieldPoints', the half extent is half a cell, (hi - lo) / (2 n) per axis computed in float64 and rounded UP to float32, so
    that the cells' union covers the grid.

    frame: a 3 x 4 matrix [rotation | origin], local -> world.  [lo, hi] and the grid are then in the frame's coordinates and the cells
    come as (n, 16) oriented-box records (orientedBoxes): the same half extents, the frame's rotation, the centres taken to the world in
    float64 and rounded to float32."""
    try:
        pts = distanceFieldPoints(resolution, lo, hi)
    except PathTracerError as e:
        raise PathTracerError(str(e).replace("bakeDistanceField", "bakeOccupancy"))
    nz, ny, nx = (int(r) for r in resolution)
    lo, hi = np.asarray(lo, np.float64).reshape(-1), np.asarray(hi, np.float64).reshape(-1)
    half64 = 0.5 * (hi - lo) / np.array([nx, ny, nz], np.float64)
    half = half64.astype(np.float32)
    half = np.where(half.astype(np.float64) < half64, np.nextafter(half, np.float32(np.inf)), half).astype(np.float32)
    if frame is not None:
        rot, origin, rot64 = _occupancy_frame(frame)
        return orientedBoxes((pts.astype(np.float64) @ rot64.T + origin).astype(np.float32), half, rot)
    b = np.zeros((pts.shape[0], 8), np.float32)
    b[:, 0:3] = pts
    b[:, 3:6] = half
    return b


def bakeOccupancy(state, resolution, bounds=None, counts=False, frame=None):
    """Conservative voxelisation: which cells of an (nz, ny, nx) grid does the scene's surface touch.  The cells are occupancyBoxes' —
    centres from distanceFieldPoints, x fastest, so the 64 boxes of a wave are neighbours; half extent half a cell — and go through
    queryOverlapAny: a bool [nz, ny, nx] grid.  counts=True goes through queryOverlap with max_prims = 0 instead and returns how many
    triangles touch each cell, uint32 [nz, ny, nx].  bounds: (lo xyz, hi xyz) of the grid, the scene box if not given.  A cell is
    occupied iff a triangle overlaps it by include/acgpt.h's closed conditions, so a triangle in a face between two cells occupies
    both.

    frame: a 3 x 4 matrix [rotation | origin], local -> world — a vehicle's or a sensor's pose.  The grid then lies in that frame
    (bounds, which must be given, are in its coordinates) and its cells are oriented boxes through queryOverlapOrientedAny /
    queryOverlapOriented: an egocentric occupancy grid.  A frame that is not orthonormal to 2^-10 raises ValueError."""
    if bounds is None:
        if frame is not None:
            raise PathTracerError("bakeOccupancy: bounds must be given with a frame (they are in the frame's coordinates)")
        info = getBvhInfo(state)
        lo, hi = [float(x) for x in info.scene_lo], [float(x) for x in info.scene_hi]
    else:
        try:
            lo, hi = bounds
        except (TypeError, ValueError):
            raise PathTracerError("bakeOccupancy: bounds is (lo xyz, hi xyz), got %r" % (bounds,))
    boxes =occupancyBoxes(resolution, lo, hi) if frame is None else occupancyBoxes(resolution, lo, hi, frame)
    shape = tuple(int(r) for r in resolution)
    if frame is not None:
        if counts:
            return queryOverlapOriented(state, boxes, max_prims=0, counts=True)["count"].reshape(shape)
        return queryOverlapOrientedAny(state, boxes).reshape(shape)
    if counts:
        return queryOverlap(state, boxes, max_prims=0, counts=True)["count"].reshape(shape)
    return queryOverlapAny(state, boxes).reshape(shape)


# ------------------------------------------------------------------ triangle against mesh ----
def _triangle_records(what, triangles):
    """The (n, 12) float32 records {a0.xyz, 0, a1.xyz, 0, a2.xyz, 0} of the NumPy argument: (n, 3, 3) or (n, 9) vertices, or (n, 12)
    records as they are"""
    t = np.asarray(triangles)
    if t.dtype.kind not in "fiu":
        raise PathTracerError("%s: the triangles must be numbers, got %s" % (what, t.dtype))
    if t.ndim == 2 and t.shape[1] == 12:
        return np.ascontiguousarray(t, np.float32)
    if not ((t.ndim == 3 and t.shape[1:] == (3, 3)) or (t.ndim == 2 and t.shape[1] == 9)):
        raise PathTracerError("%s: expected (n, 3, 3) or (n, 9) vertices or (n, 12) records, got shape %s" % (what, t.shape))
    r = np.zeros((t.shape[0], 3, 4), np.float32)
    r[:, :, :3] = t.reshape(-1, 3, 3)
    return r.reshape(-1, 12)


def _triangle_tensor(what, state, tris):
    return _tensor_records(what, state, tris, 12, "triangles", " {a0.xyz, 0, a1.xyz, 0, a2.xyz, 0}")


def queryTriangles(state, triangles, max_prims=8, counts=True):
    """Which triangles of the scene on the GPU intersect each triangle of the caller's (include/acgpt.h pt_query_triangles): the narrow
    phase of mesh-to-mesh collision.  max_prims: 0..8, how many scene triangle indices to return per query; counts: also the number
    of intersecting scene triangles, not clamped to max_prims.  max_prims=0, counts=True asks for the counts alone.  Touching counts
    as intersecting; a triangle with a non-finite coordinate intersects nothing.

    NumPy (or anything np.asarray takes): (n, 3, 3) or (n, 9) vertices, or (n, 12) records {a0.xyz, 0, a1.xyz, 0, a2.xyz, 0}
    (triangleRecords makes them from a mesh).  They go to the device and the answer comes back: a dict of prim (n, max_prims) uint32,
    the lowest indices among the intersecting triangles, ascending, 0xFFFFFFFF past the last one, and count (n,) uint32 when asked.

    A torch tensor must be (n, 12) float32 records, contiguous and on the context's device; nothing is copied, its data_ptr() goes
    straight in, and the answer is torch tensors on that device, prim and count as int32 (-1 past the last triangle).  torch's current
    stream is synchronised before the call, and the call returns synchronised."""
    k = _overlap_args("queryTriangles", max_prims, counts)
    if _is_tensor(triangles):
        _triangle_tensor("queryTriangles", state, triangles)
        r = triangles
    else:
        r = _triangle_records("queryTriangles", triangles)
    return _list_or_counts(state, "pt_query_triangles", r, k, counts)


def queryTrianglesAny(state, triangles):
    """Does any triangle of the scene intersect each triangle (include/acgpt.h pt_query_triangles_any): queryTriangles' argument, a bool
    array (n,), or a bool tensor for a tensor.  A query's walk ends at the first scene triangle it accepts."""
    if _is_tensor(triangles):
        _triangle_tensor("queryTrianglesAny", state, triangles)
        r = triangles
    else:
        r = _triangle_records("queryTrianglesAny", triangles)
    return _as_bool(_query(state, "pt_query_triangles_any", r, [((), np.uint8)])[0])


# ------------------------------------------------------------------ complete lists in CSR form ----
def _list_total(state, what, d_counts, n, d_offsets):
    """pt_list_offsets on device pointers: the total, or PathTracerError where it does not fit 32-bit offsets"""
    L = _native.hip()
    total = C.c_uint64(0)
    rc = L.pt_list_offsets(state.context, d_counts, n, d_offsets, C.byref(total))
    if rc != 0 and total.value > 0xFFFFFFFF:
        raise PathTracerError("%s: the lists hold %d indices in all, more than 32-bit offsets describe (2^32 - 1): split the batch into "
                              "several calls" % (what, total.value))
    _check(state.context, rc, "pt_list_offsets")
    return int(total.value)


def _query_lists(what, state, recs, count_call, lists_call):
    """The four steps on records that are an (n, w) float32 array or a device tensor: count, offsets, allocate, fill"""
    if _is_tensor(recs):
        import torch
        n = int(recs.shape[0])
        with torch.cuda.device(recs.device):
            cnt = torch.empty((n,), dtype=torch.int32, device=recs.device)
            off = torch.zeros((n + 1,), dtype=torch.int32, device=recs.device)
            torch.cuda.current_stream().synchronize()      # the records' producer and the allocations; every call below returns synchronised
            total = 0
            if n:
                _check(state.context, count_call(state.context, recs.data_ptr(), n, 0, None, cnt.data_ptr()), what + " (counts)")
                total = _list_total(state, what, cnt.data_ptr(), n, off.data_ptr())
            prim = torch.empty((total,), dtype=torch.int32, device=recs.device)
            torch.cuda.current_stream().synchronize()
            if n:
                _check(state.context, lists_call(state.context, recs.data_ptr(), n, off.data_ptr(), prim.data_ptr() if total else None, total, None), what)
            return {"offsets": off.to(torch.int64) & 0xFFFFFFFF, "prim": prim, "count": cnt}
    n = recs.shape[0]
    cnt, off = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32)
    got = {"offsets": off, "prim": np.zeros(0, np.uint32), "count": cnt}

    def call(d_recs, d_cnt, d_off):
        _check(state.context, count_call(state.context, d_recs, n, 0, None, d_cnt), what + " (counts)")
        total = _list_total(state, what, d_cnt, n, d_off)
        got["prim"] = np.zeros(total, np.uint32)      # allocated once the total is known, filled while the records and offsets are still up
        _host_call(state, [], [got["prim"]], lambda d_prim: _check(state.context, lists_call(state.context, d_recs, n, d_off, d_prim, total, None), what))
    _host_call(state, [recs], [cnt, off], call)
    return got


def queryOverlapLists(state, centres, half_extents=None):
    """Every triangle of the scene on the GPU that overlaps each axis-aligned box, not the first 8 (include/acgpt.h
    pt_query_overlap_lists): queryOverlap's boxes, and the lists in compressed-sparse-row form.  One call counts (pt_query_overlap with
    max_prims = 0), pt_list_offsets turns the counts into offsets, the result is allocated, a second walk fills it.

    Returns a dict: offsets (n + 1,), prim (offsets[n],) and count (n,).  Box i's triangles are prim[offsets[i]:offsets[i + 1]], in
    the caller's index-buffer order, ascending, whatever tree the scene has; count[i] is their number.  NumPy input gives uint32
    arrays.  A torch tensor — (n, 8) float32 records, contiguous, on the context's device — goes in by data_ptr() without a copy and
    comes back as tensors allocated by torch on that device: prim and count int32, offsets int64.

    Lists of more than 2^32 - 1 indices in all raise PathTracerError naming the total: split the batch."""
    L = _native.hip()
    if _is_tensor(centres):
        _overlap_tensor("queryOverlapLists", state, centres, half_extents)
        recs = centres
    else:
        recs = _overlap_boxes("queryOverlapLists", centres, half_extents)
    return _query_lists("pt_query_overlap_lists", state, recs, L.pt_query_overlap, L.pt_query_overlap_lists)


def queryTrianglesLists(state, triangles):
    """Every triangle of the scene on the GPU that intersects each triangle of the caller's, not the first 8 (include/acgpt.h
    pt_query_triangles_lists): queryTriangles' triangles, queryOverlapLists' result — a dict of offsets (n + 1,), prim (offsets[n],)
    and count (n,), query i's scene triangles in prim[offsets[i]:offsets[i + 1]], ascending.  Arrays for arrays, tensors for an
    (n, 12) float32 tensor on the context's device, which is not copied."""
    L = _native.hip()
    if _is_tensor(triangles):
        _triangle_tensor("queryTrianglesLists", state, triangles)
        recs = triangles
    else:
        recs = _triangle_records("queryTrianglesLists", triangles)
    return _query_lists("pt_query_triangles_lists", state, recs, L.pt_query_triangles, L.pt_query_triangles_lists)


# ------------------------------------------------------------------ oriented-box overlap ----
OBOX_ORTHO_TOL = np.float32(2.0 ** -10)      # kOBoxOrthoTol (csrc/oriented.h)


def orientedBoxes(centres, half_extents, rotations):
    """(n, 16) float32 oriented-box records {m[0..11] | hx, hy, hz, 0} (include/acgpt.h pt_query_overlap_oriented): centres (n, 3),
    half_extents (n, 3), (3,) or a number, rotations (3, 3) or (n, 3, 3), applied local -> world: the box's axes are a rotation's
    columns.  m is the row-major 3 x 4 matrix [rotation | centre], a pose of queryPosesAny."""
    what = "orientedBoxes"
    c, h, r = np.asarray(centres), np.asarray(half_extents), np.asarray(rotations)
    for a, name in ((c, "centres"), (h, "half extents"), (r, "rotations")):
        if a.dtype.kind not in "fiu":
            raise PathTracerError("%s: the %s must be numbers, got %s" % (what, name, a.dtype))
    if c.ndim != 2 or c.shape[1] != 3:
        raise PathTracerError("%s: expected (n, 3) centres, got shape %s" % (what, c.shape))
    n = c.shape[0]
    try:
        h = np.broadcast_to(h.astype(np.float32), (n, 3))
    except ValueError:
        raise PathTracerError("%s: half_extents of shape %s do not broadcast against %s centres" % (what, h.shape, c.shape))
    if not (h >= 0.0).all():
        raise PathTracerError("%s: every half extent must be non-negative" % what)
    if r.shape not in ((3, 3), (n, 3, 3)):
        raise PathTracerError("%s: expected (3, 3) or (n, 3, 3) rotations for %d centres, got shape %s" % (what, n, r.shape))
    b = np.zeros((n, 16), np.float32)
    m = b[:, :12].reshape(n, 3, 4)
    m[:, :, :3] = r
    m[:, :, 3] = c
    b[:, 12:15] = h
    return b


def _oriented_searchable_axes(b):
    """The orthonormality rule of include/acgpt.h on (n, 16) float32 records, in fp32 as the device evaluates it"""
    m = b[:, :12].reshape(-1, 3, 4)
    u, v, w = m[:, :, 0], m[:, :, 1], m[:, :, 2]
    dot = lambda a, c: (a[:, 0] * c[:, 0] + a[:, 1] * c[:, 1]) + a[:, 2] * c[:, 2]
    one, tol = np.float32(1.0), OBOX_ORTHO_TOL
    with np.errstate(all="ignore"):
        return (np.abs(dot(u, u) - one) <= tol) & (np.abs(dot(v, v) - one) <= tol) & (np.abs(dot(w, w) - one) <= tol) & \
               (np.abs(dot(u, v)) <= tol) & (np.abs(dot(v, w)) <= tol) & (np.abs(dot(w, u)) <= tol)


def _oriented_records(what, state, boxes):
    """The records of an oriented query: a contiguous float32 (n, 16) tensor on the context's device as it is, or an (n, 16) float32
    array of anything np.asarray takes.  NumPy records whose axes are finite and not orthonormal to 2^-10 raise ValueError (on the
    device such a record is silently a miss, as a bad box is)."""
    if _is_tensor(boxes):
        _tensor_records(what, state, boxes, 16, "boxes", " {m[0..11], hx, hy, hz, 0}")
        return boxes
    b = np.asarray(boxes)
    if b.dtype.kind not in "fiu":
        raise PathTracerError("%s: the boxes must be numbers, got %s" % (what, b.dtype))
    if b.ndim != 2 or b.shape[1] != 16:
        raise PathTracerError("%s: expected (n, 16) records {m[0..11], hx, hy, hz, 0} (orientedBoxes makes them), got shape %s" % (what, b.shape))
    b = np.ascontiguousarray(b, np.float32)
    axes = b[:, :12].reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9)
    bad = np.isfinite(axes).all(axis=1) & ~_oriented_searchable_axes(b)
    if bad.any():
        raise ValueError("%s: the axes of box %d are not orthonormal to 2^-10 (an oriented box is a rotation or a mirror, not a scale or a shear)"
                         % (what, int(np.flatnonzero(bad)[0])))
    return b


def queryOverlapOriented(state, boxes, max_prims=8, counts=True):
    """Which triangles of the scene on the GPU overlap each oriented box (include/acgpt.h pt_query_overlap_oriented): queryOverlap for
    (n, 16) records {m[0..11] | hx, hy, hz, 0}, which orientedBoxes and poseBoxes make.  max_prims, counts and the result are
    queryOverlap's: a dict of prim (n, max_prims), the lowest indices among the overlapping triangles, ascending, 0xFFFFFFFF past the
    last one, and count (n,) when asked.

    NumPy input goes through device buffers and comes back as uint32 arrays; axes that are not orthonormal to 2^-10 raise ValueError.  A
    contiguous float32 (n, 16) tensor on the context's device goes in by data_ptr() without a copy and is answered with int32 tensors
    (-1 past the last triangle); there a record that is not orthonormal is a miss."""
    k = _overlap_args("queryOverlapOriented", max_prims, counts)
    return _list_or_counts(state, "pt_query_overlap_oriented", _oriented_records("queryOverlapOriented", state, boxes), k, counts)


def queryOverlapOrientedAny(state, boxes):
    """Does any triangle of the scene overlap each oriented box (include/acgpt.h pt_query_overlap_oriented_any): queryOverlapOriented's
    records, a bool array (n,), or a bool tensor for a tensor.  A box's walk ends at the first triangle it accepts."""
    return _as_bool(_query(state, "pt_query_overlap_oriented_any", _oriented_records("queryOverlapOrientedAny", state, boxes), [((), np.uint8)])[0])


def queryOverlapOrientedLists(state, boxes):
    """Every triangle of the scene on the GPU that overlaps each oriented box (include/acgpt.h pt_query_overlap_oriented_lists):
    queryOverlapOriented's records, queryOverlapLists' result — a dict of offsets (n + 1,), prim (offsets[n],) and count (n,), box i's
    triangles in prim[offsets[i]:offsets[i + 1]], ascending.  Arrays for arrays, tensors for a tensor, which is not copied."""
    L = _native.hip()
    recs = _oriented_records("queryOverlapOrientedLists", state, boxes)
    return _query_lists("pt_query_overlap_oriented_lists", state, recs, L.pt_query_overlap_oriented, L.pt_query_overlap_oriented_lists)


def _local_box(what, lo, hi):
    """(cx, cy, cz, hx, hy, hz) float32 of the box [lo, hi]: the centre rounded to float32, the half extent the larger of hi - c and
    c - lo per axis, rounded UP, so that the record's box covers [lo, hi]"""
    try:
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    except (TypeError, ValueError):
        raise PathTracerError("%s: lo and hi are xyz, got %r and %r" % (what, lo, hi))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise PathTracerError("%s: lo and hi must be finite with lo <= hi, got %s and %s" % (what, lo, hi))
    c = (0.5 * (lo + hi)).astype(np.float32)
    h64 = np.maximum(hi - c.astype(np.float64), c.astype(np.float64) - lo)
    h = h64.astype(np.float32)
    h = np.where(h.astype(np.float64) < h64, np.nextafter(h, np.float32(np.inf)), h).astype(np.float32)
    return np.concatenate([c, h]).astype(np.float32)


def poseBoxes(state, poses, lo, hi):
    """One oriented-box record per pose, made on the device (include/acgpt.h pt_pose_boxes): the box [lo, hi] of the mesh's own frame
    under each pose.  Record p is pose p with its translation replaced by the posed centre of [lo, hi], then the half extent: what
    queryOverlapOriented* take.  Poses: queryPosesAny's forms; an (P, 16) float32 array for arrays, a tensor on the device for a tensor,
    which is not copied."""
    lb = _local_box("poseBoxes", lo, hi)
    recs = _pose_records("poseBoxes", state, poses)
    return _query(state, "pt_pose_boxes", recs, [((16,), np.float32)], lb.ctypes.data_as(C.POINTER(C.c_float)))[0]


def posedMeshBoxPad(vertices, max_translation):
    """The default pad of posedMeshBoxes, float64.  With lc the centre of the mesh's bounding box, rho the largest distance of a vertex
    from it, T the largest |translation entry| of the poses and u = 2^-24: a posed vertex ((m0 x + m1 y) + m2 z) + m3 differs from the
    exact one by at most 4.1 u |x| + u T per component, the posed centre likewise, their difference rounds by u rho, each of the
    statement's local coordinates by 3.03 u rho more, and the component errors pass through the axes with a factor sqrt 3:
    14.2 u |lc| + 11.9 u rho + 3.5 u T in all.  A rotation that was built in fp32 is orthonormal to 2^-22 or better; one that is off by
    e moves a local coordinate by up to 1.74 e rho.  The pad is 2^-20 (|lc| + rho + T) + 2^-19 rho: the rounding with a third to spare,
    and poses orthonormal to 2^-20."""
    v = np.asarray(vertices, np.float64).reshape(-1, np.asarray(vertices).shape[-1])[:, :3]
    lo, hi = v.min(axis=0), v.max(axis=0)
    lc = 0.5 * (lo + hi)
    rho = float(np.sqrt(((v - lc) ** 2).sum(axis=1).max()))
    return 2.0 ** -20 * (float(np.sqrt((lc * lc).sum())) + rho + float(max_translation)) + 2.0 ** -19 * rho


def posedMeshBoxes(state, vertices, poses, pad=None):
    """The bounding box of a mesh under every pose as oriented-box records: poseBoxes of the mesh's own bounding box, grown by pad on
    every side.  pad=None takes posedMeshBoxPad's, under which every posed vertex of posedTriangles lies inside its pose's box by the
    fp32 statement of queryOverlapOriented, for poses orthonormal to 2^-20 — so a pose whose box is free of the scene
    (queryOverlapOrientedAny) cannot collide (queryPosesAny).  vertices: (V, 3) or (V, 4); poses: queryPosesAny's forms."""
    v = np.asarray(vertices)
    if v.dtype.kind not in "fiu" or v.ndim != 2 or v.shape[1] not in (3, 4) or v.shape[0] == 0 or not np.isfinite(v[:, :3].astype(np.float64)).all():
        raise PathTracerError("posedMeshBoxes: expected finite (V, 3) or (V, 4) vertices, V >= 1, got %s %s" % (v.dtype, v.shape))
    recs = _pose_records("posedMeshBoxes", state, poses)
    if pad is None:
        if _is_tensor(recs):
            t = float(recs[:, 3::4].abs().nan_to_num(nan=0.0, posinf=0.0, neginf=0.0).max()) if recs.shape[0] else 0.0
        else:
            t = float(np.nan_to_num(np.abs(recs[:, 3::4]), nan=0.0, posinf=0.0, neginf=0.0).max()) if recs.shape[0] else 0.0
        pad = posedMeshBoxPad(v, t)
    try:
        pad = float(pad)
    except (TypeError, ValueError):
        raise PathTracerError("posedMeshBoxes: pad is a number >= 0 or None, got %r" % (pad,))
    if not (pad >= 0.0 and np.isfinite(pad)):
        raise PathTracerError("posedMeshBoxes: pad is a number >= 0 or None, got %r" % (pad,))
    v64 = v[:, :3].astype(np.float32).astype(np.float64)      # the vertices as setQueryMesh stores them
    return poseBoxes(state, recs, v64.min(axis=0) - pad, v64.max(axis=0) + pad)


def _posed_records(what, vertices, indices, poses):
    """(P, T, 12) float32 records of a mesh under P poses (poses None: the mesh as it is, P = 1).  Tensors in, a tensor out."""
    tensors = _is_tensor(vertices)
    if tensors:
        import torch
        v = vertices
        if v.dim() != 2 or v.shape[1] not in (3, 4) or not v.dtype.is_floating_point:
            raise PathTracerError("%s: expected (V, 3) or (V, 4) floating-point vertices, got %s %s" % (what, tuple(v.shape), v.dtype))
        v = v[:, :3].to(torch.float32)
        idx = indices if _is_tensor(indices) else torch.as_tensor(np.asarray(indices).astype(np.int64), device=v.device)
        if idx.dtype.is_floating_point or idx.numel() % 3:
            raise PathTracerError("%s: the indices are whole numbers, three per triangle" % what)
        idx = idx.to(device=v.device, dtype=torch.int64).reshape(-1, 3)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= v.shape[0]):
            raise PathTracerError("%s: an index is outside the %d vertices" % (what, v.shape[0]))
        if poses is None:
            moved = v[None]
        else:
            p = poses if _is_tensor(poses) else torch.as_tensor(np.asarray(poses, np.float32))
            if p.dim() not in (2, 3) or tuple(p.shape[-2:]) not in ((3, 4), (4, 4)):
                raise PathTracerError("%s: a pose is a 3 x 4 or 4 x 4 matrix, got shape %s" % (what, tuple(p.shape)))
            p = p.to(device=v.device, dtype=torch.float32).reshape(-1, p.shape[-2], 4)
            moved = torch.matmul(v[None], p[:, :3, :3].transpose(1, 2)) + p[:, None, :3, 3]
        rec = torch.zeros((moved.shape[0], idx.shape[0], 3, 4), dtype=torch.float32, device=v.device)
        rec[..., :3] = moved[:, idx]
        return rec.reshape(moved.shape[0], idx.shape[0], 12)
    v = np.asarray(vertices)
    if v.dtype.kind not in "fiu" or v.ndim != 2 or v.shape[1] not in (3, 4):
        raise PathTracerError("%s: expected (V, 3) or (V, 4) vertices, got %s %s" % (what, v.shape, v.dtype))
    v = v[:, :3].astype(np.float32)
    idx = np.asarray(indices)
    if idx.dtype.kind not in "iu" or idx.size % 3:
        raise PathTracerError("%s: the indices are whole numbers, three per triangle" % what)
    idx = idx.astype(np.int64).reshape(-1, 3)
    if idx.size and (idx.min() < 0 or idx.max() >= v.shape[0]):
        raise PathTracerError("%s: an index is outside the %d vertices" % (what, v.shape[0]))
    if poses is None:
        moved = v[None]
    else:
        p = np.asarray(poses)
        if p.dtype.kind not in "fiu" or p.ndim not in (2, 3) or p.shape[-2:] not in ((3, 4), (4, 4)):
            raise PathTracerError("%s: a pose is a 3 x 4 or 4 x 4 matrix, got shape %s" % (what, p.shape))
        p = p.astype(np.float32).reshape(-1, p.shape[-2], 4)
        moved = (np.matmul(v[None], p[:, :3, :3].transpose(0, 2, 1)) + p[:, None, :3, 3]).astype(np.float32)
    rec = np.zeros((moved.shape[0], idx.shape[0], 3, 4), np.float32)
    rec[..., :3] = moved[:, idx]
    return rec.reshape(moved.shape[0], idx.shape[0], 12)


def triangleRecords(vertices, indices, pose=None):
    """The (T, 12) float32 records queryTriangles takes, of a mesh: vertices (V, 3) or (V, 4), indices (T, 3) or flat, optionally moved
    by a 3 x 4 or 4 x 4 pose (x -> R x + t, in float32).  NumPy arrays give an array; torch tensors are transformed with torch ops on
    their device and give a tensor there."""
    if pose is not None and (pose.dim() if _is_tensor(pose) else np.ndim(pose)) != 2:
        raise PathTracerError("triangleRecords: a pose is a 3 x 4 or 4 x 4 matrix (meshCollisions takes several)")
    rec = _posed_records("triangleRecords", vertices, indices, pose)
    return rec.reshape(-1, 12)


def meshCollisions(state, vertices, indices, poses=None, pairs=False):
    """P poses of one mesh against the scene on the GPU.  poses: (P, 3, 4) or (P, 4, 4) (or one matrix, or None for the mesh as it is).
    By default one queryTrianglesAny call over the P x T records, reduced per pose: a bool (P,), does the mesh in this pose touch the
    scene.  pairs=True asks queryTriangles instead and returns a dict: pairs (m, 3), the (pose, mesh triangle, scene triangle) triples
    of the lists, and counts (P, T), the number of scene triangles each mesh triangle intersects — where it is above 8 that triangle's
    list was cut.  pairs="all" goes through queryTrianglesLists and returns the same dict with every triple, none cut, ordered by pose, mesh
    triangle and scene triangle.  Arrays for arrays, tensors for tensors.
    setQueryMesh + queryPosesAny answer the yes / no per pose on the device, without the P x T records (posedTriangles gives those)."""
    if isinstance(pairs, str) and pairs != "all":
        raise PathTracerError("meshCollisions: pairs is False, True or \"all\", got %r" % (pairs,))
    rec = _posed_records("meshCollisions", vertices, indices, poses)
    P, T = int(rec.shape[0]), int(rec.shape[1])
    flat = rec.reshape(P * T, 12)
    if isinstance(pairs, str):
        got = queryTrianglesLists(state, flat)
        if _is_tensor(got["prim"]):
            import torch
            row = torch.repeat_interleave(torch.arange(P * T, device=got["prim"].device), got["count"].to(torch.int64))
            triples = torch.stack([row // max(T, 1), row % max(T, 1), got["prim"].to(torch.int64)], dim=1)
        else:
            row = np.repeat(np.arange(P * T, dtype=np.int64), got["count"].astype(np.int64))
            triples = np.stack([row // max(T, 1), row % max(T, 1), got["prim"].astype(np.int64)], axis=1)
        return {"pairs": triples, "counts": got["count"].reshape(P, T)}
    if not pairs:
        return queryTrianglesAny(state, flat).reshape(P, T).any(1)
    got = queryTriangles(state, flat, max_prims=_native.QUERY_TRIANGLES_MAX, counts=True)
    prim = got["prim"]
    if _is_tensor(prim):
        import torch
        row, col = torch.nonzero(prim >= 0, as_tuple=True)
        triples = torch.stack([row // max(T, 1), row % max(T, 1), prim[row, col].to(torch.int64)], dim=1)
    else:
        row, col = np.nonzero(prim != 0xFFFFFFFF)
        triples = np.stack([row // max(T, 1), row % max(T, 1), prim[row, col].astype(np.int64)], axis=1)
    return {"pairs": triples, "counts": got["count"].reshape(P, T)}


# ------------------------------------------------------------------ triangle to mesh distance ----
TRIANGLE_DISTANCE_DTYPE = np.dtype([("distance", np.float32), ("prim", np.uint32), ("feature", np.float32), ("material", np.uint32), ("on_query", np.float32, 3),
                                    ("pad0", np.float32), ("point", np.float32, 3), ("pad1", np.float32)])      # pt_triangle_distance_hit
assert TRIANGLE_DISTANCE_DTYPE.itemsize == 48


def _checked_radius(what, max_radius):
    radius = float(max_radius)
    if not radius >= 0.0:
        raise PathTracerError("%s: max_radius must be non-negative, got %r" % (what, max_radius))
    return radius


def queryTriangleDistance(state, triangles, max_radius=float("inf")):
    """How far each triangle of the caller's is from the scene on the GPU, and where the two come closest (include/acgpt.h
    pt_query_triangle_distance): the distance query of mesh-to-mesh clearance.

    NumPy (or anything np.asarray takes): (n, 3, 3) or (n, 9) vertices — every triangle gets max_radius — or (n, 12) records
    {a0.xyz, max_radius, a1.xyz, ignored, a2.xyz, ignored} as they are.  They go to the device and the answer comes back: a dict of
    arrays distance (n,) float32 (0 where the two intersect, -1 where nothing lies within the radius), prim (n,) uint32 (the scene
    triangle's index in the scene's order, 0xFFFFFFFF), feature (n,) float32 (0..2: a vertex of the query; 3..5: a vertex of the scene
    triangle; 6..14: an edge pair; 15..17: a query edge crosses the scene triangle; 18..20: a scene edge crosses the query), material
    (n,) uint32, on_query (n, 3) the closest point on the query triangle and point (n, 3) the closest point on the scene.

    A torch tensor must be (n, 12) float32 records, contiguous and on the context's device; nothing is copied, its data_ptr() goes
    straight in, and the answer is torch tensors on that device: views of one (n, 12) float32 tensor, prim and material as int32 (-1
    on a miss).  torch's current stream is synchronised before the call, and the call returns synchronised."""
    if _is_tensor(triangles):
        _triangle_tensor("queryTriangleDistance", state, triangles)
        r = triangles
    else:
        r = _triangle_records("queryTriangleDistance", triangles)
        if np.asarray(triangles).shape[-1] != 12:
            r[:, 3] = _checked_radius("queryTriangleDistance", max_radius)
    return _columns(_query(state, "pt_query_triangle_distance", r, [((12,), np.float32)])[0], _TRIANGLE_DISTANCE_COLUMNS)


def meshClearance(state, vertices, indices, poses=None, max_radius=float("inf")):
    """How close P poses of one mesh come to the scene on the GPU, and where.  poses: (P, 3, 4) or (P, 4, 4) (or one matrix, or None for
    the mesh as it is).  One queryTriangleDistance call over the P x T records (triangleRecords' with max_radius in the fourth
    column), reduced per pose to its closest pair.  Returns a dict, one row per pose: clearance (P,) float32 (0 where the mesh touches
    the scene, +inf where nothing lies within max_radius), query_triangle (P,) int64 the mesh triangle of the closest pair (ties to
    the lowest; -1 where there is none), prim (P,) the scene triangle (0xFFFFFFFF, or -1 in a tensor, where there is none), on_query
    (P, 3) and on_mesh (P, 3) the closest points on the posed mesh and on the scene — on_mesh - on_query is the direction to push the
    scene away in.  Arrays for arrays, tensors for tensors.
    setQueryMesh + queryPosesDistance answer the closest pair per pose on the device, without the P x T records and their answers."""
    radius = _checked_radius("meshClearance", max_radius)
    rec = _posed_records("meshClearance", vertices, indices, poses)
    P, T = int(rec.shape[0]), int(rec.shape[1])
    rec[:, :, 3] = radius
    got = queryTriangleDistance(state, rec.reshape(P * T, 12))
    dist = got["distance"].reshape(P, T)
    if _is_tensor(dist):
        import torch
        inf = torch.full_like(dist, float("inf"))
        d = torch.where(dist >= 0, dist, inf)
        if T == 0:
            zeros = torch.zeros((P, 3), dtype=torch.float32, device=dist.device)
            return {"clearance": torch.full((P,), float("inf"), dtype=torch.float32, device=dist.device), "query_triangle": torch.full((P,), -1, dtype=torch.int64, device=dist.device),
                    "prim": torch.full((P,), -1, dtype=torch.int32, device=dist.device), "on_query": zeros, "on_mesh": zeros.clone()}
        best = d.min(dim=1).values
        cols = torch.arange(T, device=dist.device)[None].expand(P, T)
        tri = torch.where(d == best[:, None], cols, torch.full_like(cols, T)).min(dim=1).values      # the lowest mesh triangle among the ties
        found = torch.isfinite(best)
        row = torch.arange(P, device=dist.device) * T + tri
        return {"clearance": best, "query_triangle": torch.where(found, tri, torch.full_like(tri, -1)), "prim": got["prim"][row],
                "on_query": got["on_query"][row], "on_mesh": got["point"][row]}
    d = np.where(dist >= 0, dist, np.float32(np.inf)).astype(np.float32)
    if T == 0:
        return {"clearance": np.full(P, np.inf, np.float32), "query_triangle": np.full(P, -1, np.int64), "prim": np.full(P, 0xFFFFFFFF, np.uint32),
                "on_query": np.zeros((P, 3), np.float32), "on_mesh": np.zeros((P, 3), np.float32)}
    tri = d.argmin(axis=1)                                 # the first (lowest) mesh triangle among the ties
    row = np.arange(P) * T + tri
    best = d[np.arange(P), tri]
    return {"clearance": best, "query_triangle": np.where(np.isfinite(best), tri, -1).astype(np.int64), "prim": got["prim"][row], "on_query": got["on_query"][row],
            "on_mesh": got["point"][row]}


# ------------------------------------------------------------------ posed-mesh queries ----
POSE_DISTANCE_DTYPE = np.dtype([("distance", np.float32), ("prim", np.uint32), ("feature", np.float32), ("material", np.uint32), ("on_query", np.float32, 3),
                                ("query_triangle", np.uint32), ("point", np.float32, 3), ("pad1", np.float32)])      # pt_pose_distance_hit
assert POSE_DISTANCE_DTYPE.itemsize == 48
POSED_TRIANGLES_MAX = 0x7FFFFFFF      # posed triangles per call of the library; the wrappers split more over whole poses


def setQueryMesh(state, vertices, indices):
    """Register the mesh the posed-mesh queries move through the scene (include/acgpt.h pt_set_query_mesh): vertices (V, 3) or (V, 4),
    indices (T, 3) or flat, in the mesh's own frame, with meshCollisions' checks.  The mesh is de-indexed on the host and copied to
    device memory the context owns; it stays through scene changes, a second call replaces it, a mesh without triangles frees it.
    Returns the number of triangles."""
    rec = _posed_records("setQueryMesh", vertices, indices, None)
    if _is_tensor(rec):
        rec = rec.cpu().numpy()
    rec = np.ascontiguousarray(rec.reshape(-1, 12), np.float32)
    if rec.shape[0] > _native.QUERY_MESH_MAX:
        raise PathTracerError("setQueryMesh: %d triangles, the limit is %d" % (rec.shape[0], _native.QUERY_MESH_MAX))
    _check(state.context, _native.hip().pt_set_query_mesh(state.context, rec.ctypes.data if rec.shape[0] else None, rec.shape[0]), "pt_set_query_mesh")
    return int(rec.shape[0])


def getQueryMesh(state):
    """The registered query mesh: a dict of triangles and device_bytes (0, 0 while there is none)."""
    n, b = C.c_size_t(0), C.c_size_t(0)
    _check(state.context, _native.hip().pt_get_query_mesh(state.context, C.byref(n), C.byref(b)), "pt_get_query_mesh")
    return {"triangles": int(n.value), "device_bytes": int(b.value)}


def _pose_records(what, state, poses):
    """The poses as (P, 12) float32 rows of the 3 x 4 matrices.  NumPy (or anything np.asarray takes): (P, 3, 4), (P, 4, 4), (P, 12) or
    one 3 x 4 or 4 x 4 matrix.  A torch tensor: float32 on the context's device, contiguous (P, 12) or (P, 3, 4), viewed and not
    copied; (P, 4, 4) is sliced to its first three rows, which is a copy."""
    if _is_tensor(poses):
        import torch
        if poses.device.type != "cuda" or poses.device.index != state._device:
            raise PathTracerError("%s: the poses are on %s, the context is on cuda:%d" % (what, poses.device, state._device))
        if poses.dtype != torch.float32:
            raise PathTracerError("%s: the poses must be float32, got %s" % (what, poses.dtype))
        shape = tuple(poses.shape)
        if poses.dim() == 3 and shape[1:] == (4, 4):
            return poses[:, :3, :].contiguous().view(-1, 12)
        if not ((poses.dim() == 2 and shape[1] == 12) or (poses.dim() == 3 and shape[1:] == (3, 4))):
            raise PathTracerError("%s: expected a (P, 12), (P, 3, 4) or (P, 4, 4) tensor, got shape %s" % (what, shape))
        if not poses.is_contiguous():
            raise PathTracerError("%s: the poses must be contiguous (nothing is copied)" % what)
        return poses.view(-1, 12)
    p = np.asarray(poses)
    if p.dtype.kind not in "fiu":
        raise PathTracerError("%s: the poses must be numbers, got %s" % (what, p.dtype))
    if p.ndim == 2 and p.shape in ((3, 4), (4, 4)):
        p = p[None]
    if p.ndim == 2 and p.shape[1] == 12:
        return np.ascontiguousarray(p, np.float32)
    if p.ndim != 3 or p.shape[1:] not in ((3, 4), (4, 4)):
        raise PathTracerError("%s: expected (P, 3, 4), (P, 4, 4) or (P, 12) poses or one matrix, got shape %s" % (what, p.shape))
    return np.ascontiguousarray(p[:, :3, :], np.float32).reshape(-1, 12)


def _pose_call(what, state, poses, outs, call, limit):
    """Run call(d_poses, n, [d_out ...]) over the poses, split over whole poses so that no call has more than `limit` posed
    triangles.  outs: one (row shape, numpy dtype, torch dtype name) per output, or None for one the caller does not want; a row is a
    pose's share of the output.  Returns the outputs, arrays for an array and tensors for a tensor (None where not wanted)."""
    recs = _pose_records(what, state, poses)
    P = int(recs.shape[0])
    T = getQueryMesh(state)["triangles"] if P or state.context else 0
    step = max(1, int(limit) // max(T, 1))
    if _is_tensor(recs):
        import torch
        with torch.cuda.device(recs.device):
            got = [None if o is None else torch.empty((P,) + tuple(o[0](T)), dtype=getattr(torch, o[2]), device=recs.device) for o in outs]
            torch.cuda.current_stream().synchronize()      # the poses' producer and the allocations; every call below returns synchronised
        for s in range(0, P, step):
            n = min(P, s + step) - s
            call(recs.data_ptr() + 48 * s, n, [None if g is None else g.data_ptr() + s * g[0].numel() * g.element_size() for g in got])
        return got
    got = [None if o is None else np.zeros((P,) + tuple(o[0](T)), o[1]) for o in outs]

    def slices(d_poses, *d_outs):
        for s in range(0, P, step):
            call(d_poses + 48 * s, min(P, s + step) - s, [None if d is None else d + s * (g.nbytes // P) for d, g in zip(d_outs, got)])
    _host_call(state, [recs], got, slices)
    return got


def posedTriangles(state, poses, _limit=POSED_TRIANGLES_MAX):
    """The query mesh under every pose (include/acgpt.h pt_pose_triangles): (P, T, 12) float32 records {a0.xyz, 0, a1.xyz, 0, a2.xyz,
    0}, what queryTriangles, queryTrianglesLists and queryTriangleDistance take once reshaped to (P * T, 12).  The transform is the
    header's statement, x' = ((m[0] x + m[1] y) + m[2] z) + m[3] in float32 in that order, so the records are the bits the posed-mesh
    queries test.  Poses: _pose_records' forms; an array for arrays, a tensor on the device for a tensor."""
    L = _native.hip()

    def call(d_poses, n, d_outs):
        _check(state.context, L.pt_pose_triangles(state.context, d_poses, n, d_outs[0]), "pt_pose_triangles")
    return _pose_call("posedTriangles", state, poses, [(lambda T: (T, 12), np.float32, "float32")], call, _limit)[0]


def queryPosesAny(state, poses, first=False, _limit=POSED_TRIANGLES_MAX):
    """Does the query mesh (setQueryMesh) touch the scene on the GPU in each pose (include/acgpt.h pt_query_poses_any): a bool (P,).
    first=True returns (hit, first): first (P,) is the lowest mesh triangle index that intersects the scene, uint32 with 0xFFFFFFFF
    where there is none (int32 with -1 in a tensor).  One call, one byte per pose: the P x T posed triangles are formed in registers,
    and a pose that is decided stops costing walks.

    Poses: NumPy (P, 3, 4), (P, 4, 4), (P, 12) or one matrix, answered with arrays; or a float32 tensor on the context's device,
    contiguous (P, 12) or (P, 3, 4), which goes in by data_ptr() without a copy and is answered with tensors ((P, 4, 4) is sliced,
    which copies).  More than 2^31 - 1 posed triangles are split over whole poses."""
    L = _native.hip()

    def call(d_poses, n, d_outs):
        _check(state.context, L.pt_query_poses_any(state.context, d_poses, n, d_outs[0], d_outs[1]), "pt_query_poses_any")
    hit, fst = _pose_call("queryPosesAny", state, poses, [(lambda T: (), np.uint8, "uint8"), (lambda T: (), np.uint32, "int32") if first else None], call, _limit)
    if _is_tensor(hit):
        import torch
        hit = hit.view(torch.bool)
    else:
        hit = hit.view(np.bool_)
    return (hit, fst) if first else hit


def queryPosesDistance(state, poses, max_radius=float("inf"), _limit=POSED_TRIANGLES_MAX):
    """How close the query mesh (setQueryMesh) comes to the scene on the GPU in each pose, and where (include/acgpt.h
    pt_query_poses_distance).  Returns meshClearance's dict, one row per pose: clearance (P,) float32 (0 where the mesh touches the
    scene, +inf where nothing lies within max_radius), query_triangle (P,) int64 the mesh triangle of the closest pair (the smallest
    squared distance, ties to the lowest index; -1 where there is none), prim (P,) the scene triangle (0xFFFFFFFF, or -1 in a tensor,
    where there is none), feature (P,), material (P,), on_query (P, 3) and on_mesh (P, 3) the closest points on the posed mesh and on
    the scene.  Poses as queryPosesAny takes them; arrays for arrays, tensors for a tensor."""
    radius = _checked_radius("queryPosesDistance", max_radius)
    L = _native.hip()

    def call(d_poses, n, d_outs):
        _check(state.context, L.pt_query_poses_distance(state.context, d_poses, n, radius, d_outs[0]), "pt_query_poses_distance")
    out = _pose_call("queryPosesDistance", state, poses, [(lambda T: (12,), np.float32, "float32")], call, _limit)[0]
    if _is_tensor(out):
        import torch
        found = out[:, 0] >= 0
        tri = out[:, 7].view(torch.int32).to(torch.int64)
        return {"clearance": torch.where(found, out[:, 0], torch.full_like(out[:, 0], float("inf"))), "query_triangle": tri,
                "prim": out[:, 1].view(torch.int32), "feature": out[:, 2], "material": out[:, 3].view(torch.int32), "on_query": out[:, 4:7], "on_mesh": out[:, 8:11]}
    rec = out.reshape(-1).view(POSE_DISTANCE_DTYPE)
    found = rec["distance"] >= 0
    return {"clearance": np.where(found, rec["distance"], np.float32(np.inf)).astype(np.float32), "query_triangle": np.where(found, rec["query_triangle"].astype(np.int64), -1),
            "prim": np.ascontiguousarray(rec["prim"]), "feature": np.ascontiguousarray(rec["feature"]), "material": np.ascontiguousarray(rec["material"]),
            "on_query": np.ascontiguousarray(rec["on_query"]), "on_mesh": np.ascontiguousarray(rec["point"])}


# ------------------------------------------------------------------ swept spheres ----
SWEEP_DTYPE = np.dtype([("t", np.float32), ("prim", np.uint32), ("u", np.float32), ("v", np.float32), ("point", np.float32, 3), ("material", np.uint32)])      # pt_sweep_hit
assert SWEEP_DTYPE.itemsize == 32


def _sweep_records(origins_or_sweeps, directions, radius, tmax):
    """The (n, 8) float32 records {o, d, radius, tmax} of a NumPy call, every refusal before any device work."""
    p = np.asarray(origins_or_sweeps)
    if p.dtype.kind not in "fiu":
        raise PathTracerError("querySweep: the sweeps must be numbers, got %s" % p.dtype)
    if directions is None:
        if p.ndim != 2 or p.shape[1] != 8:
            raise PathTracerError("querySweep: expected an (n, 8) array {o, d, radius, tmax}, or (n, 3) origins with directions, got shape %s" % (p.shape,))
        if radius is not None:
            raise PathTracerError("querySweep: the radius is in the seventh column of (n, 8) sweeps; radius= goes with origins and directions")
        return np.ascontiguousarray(p, np.float32)
    d = np.asarray(directions)
    if p.ndim != 2 or p.shape[1] != 3 or d.shape != p.shape or d.dtype.kind not in "fiu":
        raise PathTracerError("querySweep: expected (n, 3) origins and as many directions, got shapes %s and %s" % (p.shape, d.shape))
    if radius is None:
        raise PathTracerError("querySweep: origins and directions need a radius")
    s = np.empty((p.shape[0], 8), np.float32)
    s[:, 0:3], s[:, 3:6] = p, d
    for k, val, what in ((6, radius, "radius"), (7, tmax, "tmax")):
        a = np.asarray(val, np.float64)
        if a.ndim not in (0, 1) or (a.ndim == 1 and a.shape[0] != p.shape[0]):
            raise PathTracerError("querySweep: %s is one number or one per sweep, got shape %s" % (what, a.shape))
        if not (a >= 0.0).all() or (k == 6 and np.isinf(a).any()):
            raise PathTracerError("querySweep: %s must be non-negative%s, got %r" % (what, " and finite" if k == 6 else "", val))
        s[:, k] = a
    return s


def _sweep_tensor(state, sweeps, directions, radius):
    if directions is not None or radius is not None:
        raise PathTracerError("querySweep: a tensor holds whole records (n, 8) {o, d, radius, tmax}; directions and radius go with arrays")
    return _tensor_records("querySweep", state, sweeps, 8, "sweeps", " {o, d, radius, tmax}")


def querySweep(state, origins_or_sweeps, directions=None, radius=None, tmax=float("inf"), any_hit=False):
    """How far a sphere travels before it touches the scene on the GPU, and where (include/acgpt.h pt_query_sweep): the centre moves along
    o + t d for 0 <= t <= tmax, t in units of |d|.

    NumPy (or anything np.asarray takes): (n, 8) records {o, d, radius, tmax}, or (n, 3) origins with (n, 3) directions, a radius (one
    number or one per sweep) and tmax.  The answer is a dict of arrays t (n,) float32 (-1 on a miss), prim (n,) uint32 (0xFFFFFFFF), u, v
    the weights of v1 and v2 at the contact point, point (n, 3) the contact point on the triangle, material (n,) uint32.  sweepContacts
    turns it into centres and normals.  any_hit=True asks pt_query_sweep_any instead and returns a bool array (n,): blocked or not.

    A torch tensor must be (n, 8) float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in, and
    the answer is torch tensors on that device: views of one (n, 8) float32 tensor, prim and material as int32 (-1 on a miss), or a bool
    tensor with any_hit.  torch's current stream is synchronised before the call, and the call returns synchronised."""
    if _is_tensor(origins_or_sweeps):
        _sweep_tensor(state, origins_or_sweeps, directions, radius)
        s = origins_or_sweeps
    else:
        s = _sweep_records(origins_or_sweeps, directions, radius, tmax)
    return _records_or_hit(state, s, any_hit, "pt_query_sweep", "pt_query_sweep_any", 8, _SWEEP_COLUMNS)


def sweepContacts(result, sweeps):
    """What a slide-and-step controller needs of querySweep's answer: (centres, normals, start_overlap) — the sphere's centre at impact
    o + d * t (n, 3), the unit contact normal (centre - point) / |centre - point| (n, 3), from the surface towards the centre, and where
    the sphere touched the scene before it moved, t == 0 (n,) bool.  A miss has NaN centres and normals; a centre on the surface itself
    (radius 0, or a start overlap with the centre on a triangle) has a zero normal.  sweeps: the (n, 8) records the result answers; arrays
    with arrays, tensors with tensors."""
    if _is_tensor(sweeps):
        import torch
        if sweeps.dim() != 2 or sweeps.shape[1] != 8 or result["t"].shape[0] != sweeps.shape[0]:
            raise PathTracerError("sweepContacts: expected the (n, 8) sweeps of the result, got shape %s" % (tuple(sweeps.shape),))
        t = result["t"]
        hit = t >= 0
        centre = sweeps[:, 0:3] + sweeps[:, 3:6] * t[:, None]
        diff = centre - result["point"]
        length = torch.sqrt((diff * diff).sum(dim=1, keepdim=True))
        normal = torch.where(length > 0, diff / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(diff))
        nan = torch.full_like(centre, float("nan"))
        return torch.where(hit[:, None], centre, nan), torch.where(hit[:, None], normal, nan), t == 0
    s = np.asarray(sweeps, np.float32)
    t = np.asarray(result["t"], np.float32)
    if s.ndim != 2 or s.shape[1] != 8 or t.shape != (s.shape[0],):
        raise PathTracerError("sweepContacts: expected the (n, 8) sweeps of the result, got shape %s" % (s.shape,))
    hit = t >= 0
    with np.errstate(all="ignore"):
        centre = s[:, 0:3] + s[:, 3:6] * t[:, None]
        diff = centre - np.asarray(result["point"], np.float32)
        length = np.sqrt((diff * diff).sum(axis=1, keepdims=True))
        normal = np.where(length > 0, diff / np.where(length > 0, length, np.float32(1.0)), np.float32(0.0))
    nan = np.float32(np.nan)
    return np.where(hit[:, None], centre, nan).astype(np.float32), np.where(hit[:, None], normal, nan).astype(np.float32), t == 0


# ------------------------------------------------------------------ swept capsules ----
CAPSULE_CAST_DTYPE = np.dtype([("t", np.float32), ("prim", np.uint32), ("s", np.float32), ("feature", np.float32), ("point", np.float32, 3),
                               ("material", np.uint32)])      # pt_capsule_cast_hit
assert CAPSULE_CAST_DTYPE.itemsize == 32


def _capsule_records(casts_or_p0, p1, directions, radius, tmax):
    """The (n, 12) float32 records {p0, radius | p1, tmax | d, ignored} of a NumPy call, every refusal before any device work."""
    p = np.asarray(casts_or_p0)
    if p.dtype.kind not in "fiu":
        raise PathTracerError("queryCapsuleCast: the casts must be numbers, got %s" % p.dtype)
    if p1 is None and directions is None:
        if p.ndim != 2 or p.shape[1] != 12:
            raise PathTracerError("queryCapsuleCast: expected an (n, 12) array {p0, radius, p1, tmax, d, ignored}, or (n, 3) p0 with p1 and directions, got shape %s" % (p.shape,))
        if radius is not None:
            raise PathTracerError("queryCapsuleCast: the radius is in the fourth column of (n, 12) casts; radius= goes with p0, p1 and directions")
        return np.ascontiguousarray(p, np.float32)
    if p1 is None or directions is None:
        raise PathTracerError("queryCapsuleCast: p0 goes with both p1 and directions")
    q, d = np.asarray(p1), np.asarray(directions)
    if p.ndim != 2 or p.shape[1] != 3 or q.shape != p.shape or d.shape != p.shape or q.dtype.kind not in "fiu" or d.dtype.kind not in "fiu":
        raise PathTracerError("queryCapsuleCast: expected (n, 3) p0 and as many p1 and directions, got shapes %s, %s and %s" % (p.shape, q.shape, d.shape))
    if radius is None:
        raise PathTracerError("queryCapsuleCast: p0, p1 and directions need a radius")
    s = np.zeros((p.shape[0], 12), np.float32)
    s[:, 0:3], s[:, 4:7], s[:, 8:11] = p, q, d
    for k, val, what in ((3, radius, "radius"), (7, tmax, "tmax")):
        a = np.asarray(val, np.float64)
        if a.ndim not in (0, 1) or (a.ndim == 1 and a.shape[0] != p.shape[0]):
            raise PathTracerError("queryCapsuleCast: %s is one number or one per capsule, got shape %s" % (what, a.shape))
        if not (a >= 0.0).all() or (k == 3 and np.isinf(a).any()):
            raise PathTracerError("queryCapsuleCast: %s must be non-negative%s, got %r" % (what, " and finite" if k == 3 else "", val))
        s[:, k] = a
    return s


def _capsule_tensor(state, casts, p1, directions, radius):
    if p1 is not None or directions is not None or radius is not None:
        raise PathTracerError("queryCapsuleCast: a tensor holds whole records (n, 12) {p0, radius, p1, tmax, d, ignored}; p1, directions and radius go with arrays")
    return _tensor_records("queryCapsuleCast", state, casts, 12, "casts", " {p0, radius, p1, tmax, d, ignored}")


def queryCapsuleCast(state, casts_or_p0, p1=None, directions=None, radius=None, tmax=float("inf"), any_hit=False):
    """How far a capsule travels before it touches the scene on the GPU, and where (include/acgpt.h pt_query_capsule_cast): the axis is
    {p0 + t d, p1 + t d} for 0 <= t <= tmax, t in units of |d|.

    NumPy (or anything np.asarray takes): (n, 12) records {p0, radius | p1, tmax | d, ignored}, or (n, 3) p0 with (n, 3) p1, (n, 3)
    directions, a radius (one number or one per capsule) and tmax.  The answer is a dict of arrays t (n,) float32 (-1 on a miss), prim
    (n,) uint32 (0xFFFFFFFF), s the parameter on the axis and feature the kind of pt_query_segments' closest pair at impact, point (n, 3)
    the contact point on the triangle, material (n,) uint32.  capsuleContacts turns it into axis ends, axis points and normals.
    any_hit=True asks pt_query_capsule_cast_any instead and returns a bool array (n,): blocked or not.

    A torch tensor must be (n, 12) float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in,
    and the answer is torch tensors on that device: views of one (n, 8) float32 tensor, prim and material as int32 (-1 on a miss), or a
    bool tensor with any_hit.  torch's current stream is synchronised before the call, and the call returns synchronised."""
    if _is_tensor(casts_or_p0):
        _capsule_tensor(state, casts_or_p0, p1, directions, radius)
        s = casts_or_p0
    else:
        s = _capsule_records(casts_or_p0, p1, directions, radius, tmax)
    return _records_or_hit(state, s, any_hit, "pt_query_capsule_cast", "pt_query_capsule_cast_any", 8, _CAPSULE_CAST_COLUMNS)


def capsuleContacts(result, casts):
    """What a controller needs of queryCapsuleCast's answer: (p0, p1, axis_point, normal, start_overlap) — the axis' ends at impact
    p0 + d * t and p1 + d * t (n, 3), the point of the axis that touches, p0' + (p1' - p0') * s (n, 3), the unit contact normal
    (axis point - point) / |axis point - point| (n, 3), from the surface towards the axis, and where the capsule touched the scene before
    it moved, t == 0 (n,) bool.  A miss has NaN ends, axis points and normals; an axis point on the surface itself (radius 0, or a start
    overlap with the axis through a triangle) has a zero normal.  casts: the (n, 12) records the result answers; arrays with arrays,
    tensors with tensors."""
    if _is_tensor(casts):
        import torch
        if casts.dim() != 2 or casts.shape[1] != 12 or result["t"].shape[0] != casts.shape[0]:
            raise PathTracerError("capsuleContacts: expected the (n, 12) casts of the result, got shape %s" % (tuple(casts.shape),))
        t = result["t"]
        hit = t >= 0
        move = casts[:, 8:11] * t[:, None]
        q0, q1 = casts[:, 0:3] + move, casts[:, 4:7] + move
        on_axis = q0 + (q1 - q0) * result["s"][:, None]
        diff = on_axis - result["point"]
        length = torch.sqrt((diff * diff).sum(dim=1, keepdim=True))
        normal = torch.where(length > 0, diff / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(diff))
        nan = torch.full_like(q0, float("nan"))
        return tuple(torch.where(hit[:, None], x, nan) for x in (q0, q1, on_axis, normal)) + (t == 0,)
    c = np.asarray(casts, np.float32)
    t = np.asarray(result["t"], np.float32)
    if c.ndim != 2 or c.shape[1] != 12 or t.shape != (c.shape[0],):
        raise PathTracerError("capsuleContacts: expected the (n, 12) casts of the result, got shape %s" % (c.shape,))
    hit = t >= 0
    with np.errstate(all="ignore"):
        move = c[:, 8:11] * t[:, None]
        q0, q1 = c[:, 0:3] + move, c[:, 4:7] + move
        on_axis = q0 + (q1 - q0) * np.asarray(result["s"], np.float32)[:, None]
        diff = on_axis - np.asarray(result["point"], np.float32)
        length = np.sqrt((diff * diff).sum(axis=1, keepdims=True))
        normal = np.where(length > 0, diff / np.where(length > 0, length, np.float32(1.0)), np.float32(0.0))
    nan = np.float32(np.nan)
    return tuple(np.where(hit[:, None], x, nan).astype(np.float32) for x in (q0, q1, on_axis, normal)) + (t == 0,)


# ------------------------------------------------------------------ swept oriented boxes ----
BOX_CAST_DTYPE = _native.BOX_CAST_DTYPE      # pt_box_cast_hit


def _box_cast_records(casts_or_boxes, directions, tmax):
    """The (n, 20) float32 records {m0..m11 | hx hy hz - | d, tmax} of a NumPy call, every refusal before any device work."""
    what = "queryBoxCast"
    b = np.asarray(casts_or_boxes)
    if b.dtype.kind not in "fiu":
        raise PathTracerError("%s: the casts must be numbers, got %s" % (what, b.dtype))
    if directions is None:
        if b.ndim != 2 or b.shape[1] != 20:
            raise PathTracerError("%s: expected an (n, 20) array {m[0..11], hx, hy, hz, 0, d, tmax}, or (n, 16) oriented boxes with directions, got shape %s" % (what, b.shape))
        return np.ascontiguousarray(b, np.float32)
    d = np.asarray(directions)
    if b.ndim != 2 or b.shape[1] != 16:
        raise PathTracerError("%s: directions go with (n, 16) oriented boxes (orientedBoxes makes them), got shape %s" % (what, b.shape))
    if d.dtype.kind not in "fiu" or d.shape not in ((b.shape[0], 3), (3,)):
        raise PathTracerError("%s: expected (n, 3) directions or one (3,) for %d boxes, got shape %s" % (what, b.shape[0], d.shape))
    t = np.asarray(tmax, np.float64)
    if t.ndim not in (0, 1) or (t.ndim == 1 and t.shape[0] != b.shape[0]):
        raise PathTracerError("%s: tmax is one number or one per box, got shape %s" % (what, t.shape))
    if not (t >= 0.0).all():
        raise PathTracerError("%s: tmax must be non-negative, got %r" % (what, tmax))
    s = np.zeros((b.shape[0], 20), np.float32)
    s[:, :16], s[:, 16:19], s[:, 19] = b, d, t
    return s


def _box_cast_tensor(state, casts, directions):
    what = "queryBoxCast"
    if directions is not None:
        raise PathTracerError("%s: a tensor holds whole records (n, 20) {m[0..11], hx, hy, hz, 0, d, tmax}; directions go with arrays" % what)
    return _tensor_records(what, state, casts, 20, "casts", " {m[0..11], hx, hy, hz, 0, d, tmax}")


def queryBoxCast(state, casts_or_boxes, directions=None, tmax=float("inf"), any_hit=False):
    """How far an oriented box travels before it touches the scene on the GPU, which triangle it touches, with which normal and where
    (include/acgpt.h pt_query_box_cast): the box is at centre + t d for 0 <= t <= tmax, t in units of |d|.

    NumPy (or anything np.asarray takes): (n, 20) records {m[0..11] | hx, hy, hz, 0 | d, tmax}, or (n, 16) oriented boxes
    (orientedBoxes' output) with (n, 3) or (3,) directions and tmax (one number or one per box).  The answer is a dict of arrays t (n,)
    float32 (-1 on a miss), prim (n,) uint32 (0xFFFFFFFF), feature (n,) float32 (the winning axis 0..12 of the 13-axis test, 13 for a
    box that starts in contact), material (n,) uint32, normal (n, 3) the unit normal from the triangle to the box and point (n, 3) the
    contact point (both zero on a miss and on a start overlap).  boxCastContacts turns it into what a controller needs.
    any_hit=True asks pt_query_box_cast_any instead and returns a bool array (n,): blocked or not.

    A torch tensor must be (n, 20) float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in,
    and the answer is torch tensors on that device: views of one (n, 12) float32 tensor, prim and material as int32 (-1 on a miss), or a
    bool tensor with any_hit.  torch's current stream is synchronised before the call, and the call returns synchronised."""
    if _is_tensor(casts_or_boxes):
        _box_cast_tensor(state, casts_or_boxes, directions)
        s = casts_or_boxes
    else:
        s = _box_cast_records(casts_or_boxes, directions, tmax)
    return _records_or_hit(state, s, any_hit, "pt_query_box_cast", "pt_query_box_cast_any", 12, _BOX_CAST_COLUMNS)


def boxCastContacts(result, casts):
    """What a controller needs of queryBoxCast's answer: (centre, normal, point, start_overlap, slide) — the box's centre at impact
    c + d * t (n, 3), the unit contact normal from the surface towards the box and the contact point as the result gives them, where
    the box touched the scene before it moved, t == 0 (n,) bool, and the direction the box can go on in without entering the surface,
    d - n (n . d) (n, 3): d itself on a start overlap, whose normal is zero.  A miss has NaN centres, normals, points and slides.
    casts: the (n, 20) records the result answers; arrays with arrays, tensors with tensors."""
    if _is_tensor(casts):
        import torch
        if casts.dim() != 2 or casts.shape[1] != 20 or result["t"].shape[0] != casts.shape[0]:
            raise PathTracerError("boxCastContacts: expected the (n, 20) casts of the result, got shape %s" % (tuple(casts.shape),))
        t = result["t"]
        hit = t >= 0
        d = casts[:, 16:19]
        centre = torch.stack([casts[:, 3], casts[:, 7], casts[:, 11]], dim=1) + d * t[:, None]
        nrm = result["normal"]
        slide = d - nrm * (nrm * d).sum(dim=1, keepdim=True)
        nan = torch.full_like(centre, float("nan"))
        return tuple(torch.where(hit[:, None], x, nan) for x in (centre, nrm, result["point"])) + (t == 0, torch.where(hit[:, None], slide, nan))
    c = np.asarray(casts, np.float32)
    t = np.asarray(result["t"], np.float32)
    if c.ndim != 2 or c.shape[1] != 20 or t.shape != (c.shape[0],):
        raise PathTracerError("boxCastContacts: expected the (n, 20) casts of the result, got shape %s" % (c.shape,))
    hit = t >= 0
    nrm, point = np.asarray(result["normal"], np.float32), np.asarray(result["point"], np.float32)
    with np.errstate(all="ignore"):
        d = c[:, 16:19]
        centre = c[:, [3, 7, 11]] + d * t[:, None]
        slide = d - nrm * (nrm * d).sum(axis=1, keepdims=True)
    nan = np.float32(np.nan)
    return tuple(np.where(hit[:, None], x, nan).astype(np.float32) for x in (centre, nrm, point)) + (t == 0, np.where(hit[:, None], slide, nan).astype(np.float32))


def poseBoxCasts(state, poses, local_box, motions):
    """The (P, 20) casts of a box of the mesh's own frame under each pose, assembled on the device: poseBoxes' record (pt_pose_boxes)
    with the motion {d, tmax} behind it, what queryBoxCast takes — a registered hull's bounding box cast per pose ahead of
    queryPosesCast.  local_box: (lo, hi) of the box in the mesh's frame, as poseBoxes takes them.  motions: queryPosesCast's ((P, 4)
    {d, tmax}, (P, 3) directions, or one row for all poses); with a poses tensor a (P, 4) float32 tensor on the same device, and the
    answer is a tensor there."""
    try:
        lo, hi = local_box
    except (TypeError, ValueError):
        raise PathTracerError("poseBoxCasts: local_box is (lo, hi), two xyz, got %r" % (local_box,))
    if _is_tensor(poses):
        if not _is_tensor(motions):
            raise PathTracerError("poseBoxCasts: tensor poses take a (P, 4) tensor of motions")
        import torch
        _cast_tensor("poseBoxCasts", state, motions, 4, "motions")
        boxes = poseBoxes(state, poses, lo, hi)
        if int(motions.shape[0]) != int(boxes.shape[0]):
            raise PathTracerError("poseBoxCasts: %d poses and %d motions" % (int(boxes.shape[0]), int(motions.shape[0])))
        return torch.cat([boxes, motions], dim=1).contiguous()
    _local_box("poseBoxCasts", lo, hi)
    recs = _pose_records("poseBoxCasts", state, poses)
    m = _motion_records("poseBoxCasts", motions, int(recs.shape[0]))
    return np.ascontiguousarray(np.concatenate([poseBoxes(state, recs, lo, hi), m], axis=1))


# ------------------------------------------------------------------ translating-triangle casts ----
TRIANGLE_CAST_DTYPE = np.dtype([("t", np.float32), ("prim", np.uint32), ("feature", np.float32), ("query_triangle", np.uint32), ("point", np.float32, 3),
                                ("material", np.uint32)])      # pt_triangle_cast_hit
assert TRIANGLE_CAST_DTYPE.itemsize == 32


def _cast_records(what, casts, directions, tmax):
    """The (n, 16) float32 records {a0, tmax | a1, . | a2, . | d, .} of a NumPy call, every refusal before any device work."""
    p = np.asarray(casts)
    if p.dtype.kind not in "fiu":
        raise PathTracerError("%s: the casts must be numbers, got %s" % (what, p.dtype))
    if directions is None:
        if p.ndim != 2 or p.shape[1] != 16:
            raise PathTracerError("%s: expected an (n, 16) array {a0, tmax, a1, ., a2, ., d, .}, or triangles with directions, got shape %s" % (what, p.shape))
        return np.ascontiguousarray(p, np.float32)
    if p.ndim == 3 and p.shape[1:] == (3, 3):
        tri = p.astype(np.float32)
    elif p.ndim == 2 and p.shape[1] == 9:
        tri = p.astype(np.float32).reshape(-1, 3, 3)
    elif p.ndim == 2 and p.shape[1] == 12:
        tri = p.astype(np.float32).reshape(-1, 3, 4)[:, :, :3]
    else:
        raise PathTracerError("%s: expected (n, 3, 3), (n, 9) or (n, 12) triangles with directions, got shape %s" % (what, p.shape))
    n = tri.shape[0]
    d = np.asarray(directions)
    if d.dtype.kind not in "fiu" or d.shape not in ((3,), (n, 3)):
        raise PathTracerError("%s: expected one direction (3,) or one per triangle (n, 3), got shape %s" % (what, d.shape))
    a = np.asarray(tmax, np.float64)
    if a.ndim not in (0, 1) or (a.ndim == 1 and a.shape[0] != n):
        raise PathTracerError("%s: tmax is one number or one per cast, got shape %s" % (what, a.shape))
    if not (a >= 0.0).all():
        raise PathTracerError("%s: tmax must be non-negative, got %r" % (what, tmax))
    s = np.zeros((n, 16), np.float32)
    s[:, 0:3], s[:, 4:7], s[:, 8:11] = tri[:, 0], tri[:, 1], tri[:, 2]
    s[:, 12:15] = d
    s[:, 3] = a
    return s


def _cast_tensor(what, state, x, width, name):
    return _tensor_records(what, state, x, width, name, " of " + name)


def queryTriangleCast(state, casts_or_triangles, directions=None, tmax=float("inf"), any_hit=False):
    """How far a triangle translates along d before it first touches the scene on the GPU, and where (include/acgpt.h
    pt_query_triangle_cast): the triangle occupies a_i + t d for 0 <= t <= tmax, t in units of |d|.

    NumPy (or anything np.asarray takes): (n, 16) records {a0, tmax | a1, . | a2, . | d, .}, or (n, 3, 3), (n, 9) or (n, 12) triangles
    with directions (3,) or (n, 3) and tmax (one number or one per cast).  The answer is a dict of arrays t (n,) float32 (-1 on a miss,
    0 on a start overlap), prim (n,) uint32 (0xFFFFFFFF), feature (n,) float32 (0..2: a corner of the query meets the scene triangle;
    3..5: a corner of the scene triangle meets the query; 6..14: edge 3 i + j, an edge pair; 15: start overlap), query_triangle (n,)
    uint32 (0 here), point (n, 3) the contact in world space (zero on a start overlap), material (n,) uint32.  castContacts turns it
    into normals.  any_hit=True asks pt_query_triangle_cast_any instead and returns a bool array (n,): blocked or not.

    A torch tensor must be (n, 16) float32, contiguous and on the context's device; nothing is copied, its data_ptr() goes straight in,
    and the answer is torch tensors on that device: views of one (n, 8) float32 tensor, prim, query_triangle and material as int32
    (-1 on a miss), or a bool tensor with any_hit.  torch's current stream is synchronised before the call, and the call returns
    synchronised."""
    if _is_tensor(casts_or_triangles):
        if directions is not None:
            raise PathTracerError("queryTriangleCast: a tensor holds whole records (n, 16); directions go with arrays")
        _cast_tensor("queryTriangleCast", state, casts_or_triangles, 16, "casts")
        s = casts_or_triangles
    else:
        s = _cast_records("queryTriangleCast", casts_or_triangles, directions, tmax)
    return _records_or_hit(state, s, any_hit, "pt_query_triangle_cast", "pt_query_triangle_cast_any", 8, _TRIANGLE_CAST_COLUMNS)


def _motion_records(what, motions, P):
    m = np.asarray(motions)
    if m.dtype.kind not in "fiu" or m.shape not in ((P, 4), (P, 3), (4,), (3,)):
        raise PathTracerError("%s: expected (P, 4) motions {d, tmax}, (P, 3) directions or one of either, got shape %s" % (what, m.shape))
    out = np.full((P, 4), np.inf, np.float32)
    out[:, :m.shape[-1]] = m
    return out


def queryPosesCast(state, poses, motions):
    """How far the query mesh (setQueryMesh) translates from each pose before it first touches the scene on the GPU, and where
    (include/acgpt.h pt_query_poses_cast).  motions: (P, 4) {d, tmax} in the world frame, applied after the pose ((P, 3): tmax = +inf;
    one row for all poses).  Returns queryTriangleCast's dict, one row per pose, with query_triangle the mesh triangle that touches
    first (the smallest t, ties to the lowest index; 0xFFFFFFFF, or -1 in a tensor, where nothing is touched).  The P x T posed
    triangles are formed in registers.  Poses as queryPosesAny takes them; with a poses tensor the motions are a (P, 4) float32 tensor on
    the same device, and the answer is tensors."""
    recs = _pose_records("queryPosesCast", state, poses)
    P = int(recs.shape[0])
    fn = _native.hip().pt_query_poses_cast

    def call(d_poses, d_motions, d_out):
        _check(state.context, fn(state.context, d_poses, d_motions, P, d_out), "pt_query_poses_cast")
    if _is_tensor(recs):
        if not _is_tensor(motions):
            raise PathTracerError("queryPosesCast: tensor poses take a (P, 4) tensor of motions")
        _cast_tensor("queryPosesCast", state, motions, 4, "motions")
        if int(motions.shape[0]) != P:
            raise PathTracerError("queryPosesCast: %d poses and %d motions" % (P, int(motions.shape[0])))
        out = _tensor_call(recs, [((P, 8), "float32")], lambda d_poses, d_out: call(d_poses, motions.data_ptr() if P else None, d_out))[0]
    else:
        out = np.zeros((P, 8), np.float32)
        _host_call(state, [recs, _motion_records("queryPosesCast", motions, P)], [out], call)
    return _columns(out, _TRIANGLE_CAST_COLUMNS)


def meshCast(state, vertices, indices, poses, motions):
    """queryPosesCast by the materialising route, kept for comparison: the P x T posed triangles are formed on the host by the header's
    statement (x' = ((m[0] x + m[1] y) + m[2] z) + m[3], float32, in that order), cast with one queryTriangleCast call and reduced per
    pose to the smallest t, ties to the lowest mesh triangle.  NumPy only.  The same dict, the same bits."""
    rec = _posed_records("meshCast", vertices, indices, None)[0].reshape(-1, 3, 4)[:, :, :3]
    p = _pose_records("meshCast", state, poses).reshape(-1, 3, 4)
    P, T = p.shape[0], rec.shape[0]
    m = _motion_records("meshCast", motions, P)
    out = np.zeros(P, TRIANGLE_CAST_DTYPE)
    out["t"], out["prim"], out["query_triangle"], out["material"] = -1.0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF
    if P and T:
        casts = np.zeros((P, T, 16), np.float32)
        with np.errstate(all="ignore"):
            x, y, z = rec[None, :, :, 0], rec[None, :, :, 1], rec[None, :, :, 2]
            for j in range(3):
                m0, m1, m2, m3 = (p[:, j, c, None, None] for c in range(4))
                casts[:, :, j:12:4] = ((m0 * x + m1 * y) + m2 * z) + m3
        casts[:, :, 3] = m[:, None, 3]
        casts[:, :, 12:15] = m[:, None, 0:3]
        got = queryTriangleCast(state, casts.reshape(P * T, 16))
        t = got["t"].reshape(P, T)
        key = np.where(t >= 0, t, np.float32(np.inf))
        tri = key.argmin(axis=1)                           # the first (lowest) mesh triangle among the ties
        found = (t >= 0).any(axis=1)
        row = np.arange(P) * T + tri
        for k in ("t", "prim", "feature", "point", "material"):
            out[k][found] = got[k][row][found]
        out["query_triangle"][found] = tri[found]
    return _columns(out.view(np.float32).reshape(P, 8), _TRIANGLE_CAST_COLUMNS)


def castContacts(result, casts, vertices, indices):
    """What a slide-and-step controller needs of queryTriangleCast's answer: (normals, start_overlap) — the unit contact normal (n, 3)
    by the winning feature, facing against d: the scene triangle's normal (features 0..2), the query triangle's (3..5), or cross(D, E)
    of the two edges that met (6 + 3 i + j: the query's edge i of (a1 - a0, a2 - a0, a2 - a1), the scene triangle's edge j of (v1 - v0,
    v2 - v0, v2 - v1)); and where the triangle touched the scene before it moved, t == 0 with feature 15 (n,) bool.  A miss has NaN
    normals, a start overlap and a degenerate feature a zero normal.  casts: the (n, 16) records the result answers; vertices, indices:
    the scene's.  NumPy; tensors are read back."""
    def host(a):
        return a.cpu().numpy() if _is_tensor(a) else np.asarray(a)
    s = host(casts).astype(np.float64)
    t, feature, prim = host(result["t"]), host(result["feature"]), host(result["prim"]).astype(np.int64) & 0xFFFFFFFF
    if s.ndim != 2 or s.shape[1] != 16 or t.shape != (s.shape[0],):
        raise PathTracerError("castContacts: expected the (n, 16) casts of the result, got shape %s" % (s.shape,))
    v = host(vertices).astype(np.float64).reshape(-1, 4)[:, :3] if host(vertices).ndim == 1 else host(vertices).astype(np.float64)[:, :3]
    idx = host(indices).astype(np.int64).reshape(-1, 3)
    hit = t >= 0
    tri = v[idx[np.where(hit, prim, 0)]] if idx.shape[0] else np.zeros((s.shape[0], 3, 3))
    a0, a1, a2, d = s[:, 0:3], s[:, 4:7], s[:, 8:11], s[:, 12:15]
    q_edges = np.stack([a1 - a0, a2 - a0, a2 - a1], axis=1)
    s_edges = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], tri[:, 2] - tri[:, 1]], axis=1)
    f = np.where(hit, feature, 15).astype(np.int64)
    k = np.clip(f - 6, 0, 8)
    rows = np.arange(s.shape[0])
    normal = np.where((f <= 2)[:, None], np.cross(s_edges[:, 0], s_edges[:, 1]),
                      np.where((f <= 5)[:, None], np.cross(q_edges[:, 0], q_edges[:, 1]), np.cross(q_edges[rows, k // 3], s_edges[rows, k % 3])))
    normal = np.where((f == 15)[:, None], 0.0, normal)
    with np.errstate(all="ignore"):
        length = np.sqrt((normal * normal).sum(axis=1, keepdims=True))
        normal = np.where(length > 0, normal / np.where(length > 0, length, 1.0), 0.0)
        normal = np.where(((normal * d).sum(axis=1) > 0)[:, None], -normal, normal)
    return np.where(hit[:, None], normal, np.nan).astype(np.float32), hit & (f == 15)


def advanceUntilContact(state, poses):
    """Step the query mesh (setQueryMesh) along a polyline of K poses until it first touches the scene: leg k moves the mesh in pose k
    by the translation from pose k to pose k + 1 (the rotation changes between the legs, not within one).  All K - 1 legs are one
    queryPosesCast call with tmax = 1.  Returns a dict: leg (the first blocked leg, -1 when the whole path is free), t (its time of
    impact in [0, 1]; 1 when free), pose (3, 4) float32 (where the mesh stops: pose `leg` moved by t of the leg; the last pose when
    free) and contact (queryPosesCast's row of that leg, None when free)."""
    p = np.asarray(_pose_records("advanceUntilContact", state, poses.cpu().numpy() if _is_tensor(poses) else poses)).reshape(-1, 3, 4)
    if p.shape[0] < 2:
        raise PathTracerError("advanceUntilContact: a path has at least two poses, got %d" % p.shape[0])
    motions = np.ones((p.shape[0] - 1, 4), np.float32)
    motions[:, 0:3] = p[1:, :, 3] - p[:-1, :, 3]
    got = queryPosesCast(state, p[:-1], motions)
    blocked = np.flatnonzero(got["t"] >= 0)
    if blocked.size == 0:
        return {"leg": -1, "t": 1.0, "pose": p[-1].copy(), "contact": None}
    k = int(blocked[0])
    pose = p[k].copy()
    pose[:, 3] = pose[:, 3] + motions[k, 0:3] * got["t"][k]
    return {"leg": k, "t": float(got["t"][k]), "pose": pose, "contact": {name: got[name][k] for name in got}}


# ------------------------------------------------------------------ ambient occlusion ----
def aoSamples(K):
    """The default sample pattern of the ambient-occlusion calls: K points of a Vogel spiral on the unit disk, float32 (K, 2):
    r = sqrt((k + 0.5) / K), angle k * pi * (3 - sqrt(5)), computed in float64 and rounded; a point that rounding pushed outside the disk
    (x * x + y * y > 1 in fp32) is pulled back in, one fp32 step towards zero per component at a time.  Lifted over the hemisphere its
    points are cosine-distributed."""
    import math
    K = int(K)
    if not 1 <= K <= _native.AO_MAX_SAMPLES:
        raise PathTracerError("aoSamples: K must be 1..%d, got %d" % (_native.AO_MAX_SAMPLES, K))
    golden = math.pi * (3.0 - math.sqrt(5.0))
    out = np.zeros((K, 2), np.float32)
    zero, one = np.float32(0.0), np.float32(1.0)
    for k in range(K):
        r = math.sqrt((k + 0.5) / K)
        x, y = np.float32(r * math.cos(k * golden)), np.float32(r * math.sin(k * golden))
        while x * x + y * y > one:
            x, y = np.nextafter(x, zero), np.nextafter(y, zero)
        out[k] = (x, y)
    return out


def _ao_disk(disk, samples, what):
    """The (K, 2) float32 pattern of a call: the caller's, checked as the library checks it, or the default one for `samples`."""
    if disk is None:
        return aoSamples(samples)
    d = np.asarray(disk)
    if d.ndim != 2 or d.shape[1] != 2 or d.dtype.kind not in "fiu":
        raise PathTracerError("%s: the disk pattern must be a (K, 2) array of numbers, got %s %s" % (what, d.dtype, d.shape))
    if not 1 <= d.shape[0] <= _native.AO_MAX_SAMPLES:
        raise PathTracerError("%s: the disk pattern must have 1..%d points, got %d" % (what, _native.AO_MAX_SAMPLES, d.shape[0]))
    d = np.ascontiguousarray(d, np.float32)
    with np.errstate(all="ignore"):
        inside = np.isfinite(d).all(axis=1) & (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= np.float32(1.0))
    if not inside.all():
        raise PathTracerError("%s: disk point %d is outside the unit disk" % (what, int(np.flatnonzero(~inside)[0])))
    return d


def _ao_reach(state, radius, bias, what):
    """(radius, bias): the caller's, or a quarter and a thousandth of the scene box's diagonal."""
    if radius is None or bias is None:
        info = getBvhInfo(state)
        diag = float(np.sqrt(sum((float(info.scene_hi[k]) - float(info.scene_lo[k])) ** 2 for k in range(3))))
        radius = 0.25 * diag if radius is None else radius
        bias = 1e-3 * diag if bias is None else bias
    radius, bias = float(radius), float(bias)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise PathTracerError("%s: radius must be positive and finite, got %r" % (what, radius))
    if not (bias >= 0.0 and np.isfinite(bias)):
        raise PathTracerError("%s: bias must be non-negative and finite, got %r" % (what, bias))
    return radius, bias


def _ao_params(disk, radius, bias, seed=0, accumulate=False, total=None):
    K = disk.shape[0]
    return _native.AoParams(K, radius, bias, int(seed) & 0xFFFFFFFF, 1 if accumulate else 0, K if total is None else int(total), (C.c_uint32 * 2)(0, 0))


def _ao_image_call(state, nd_ptr, disk, ap, visible_ptr):
    """pt_ao_image on a feature buffer on the device: the AO image, float32 [height, width]"""
    h, w = int(state.params.height), int(state.params.width)
    out = np.zeros((h, w), np.float32)
    bufs = _device_buffers(state, 1, max(w * h * 4, 4))
    try:
        _check(state.context, _native.hip().pt_ao_image(state.context, C.byref(state.params), nd_ptr, disk.ctypes.data, C.byref(ap), visible_ptr, bufs[0]), "pt_ao_image")
        if out.size:
            _check(state.context, _native.hip().pt_copy_to_host(state.context, out.ctypes.data, bufs[0], out.nbytes), "copy to host")
    finally:
        _free_device_buffers(state, bufs)
    return out


def _ao_features(state, normal_depth, bufs, what):
    """The device pointer of the normal_depth buffer of the current view: rendered now (None), uploaded (an array) or the caller's
    (a device pointer).  New buffers are appended to bufs; the caller frees those."""
    h, w = int(state.params.height), int(state.params.width)
    if normal_depth is not None and not isinstance(normal_depth, np.ndarray):
        return int(normal_depth)
    bufs += _device_buffers(state, 2 if normal_depth is None else 1, max(w * h * 16, 16))
    if normal_depth is None:
        _check(state.context, _native.hip().pt_render_features(state.context, C.byref(state.params), bufs[-2], bufs[-1]), "pt_render_features")
    else:
        if normal_depth.shape != (h, w, 4):
            raise PathTracerError("%s: normal_depth of shape %s, got %s" % (what, (h, w, 4), normal_depth.shape))
        a = np.ascontiguousarray(normal_depth, np.float32)
        _check(state.context, _native.hip().pt_copy_to_device(state.context, bufs[-1], a.ctypes.data, a.nbytes), "copy to device")
    return bufs[-1]


def ambientOcclusion(state, samples=16, radius=None, bias=None, disk=None, normal_depth=None, seed=0):
    """Ambient occlusion of the current view (include/acgpt.h pt_ao_image): float32 [height, width] (row 0 = bottom), the share of
    `samples` rays over each pixel's first hit that find nothing within `radius`; 1 where the pixel sees no surface.  radius defaults to a
    quarter of the scene box's diagonal, bias (the rays' start above the surface) to a thousandth of it; disk: a (K, 2) pattern on the unit
    disk instead of aoSamples(samples).  normal_depth: renderFeatures' second output for this view (an array, or a device pointer), rendered
    here if not given."""
    disk = _ao_disk(disk, samples, "ambientOcclusion")
    radius, bias = _ao_reach(state, radius, bias, "ambientOcclusion")
    h, w = int(state.params.height), int(state.params.width)
    bufs = []
    try:
        nd = _ao_features(state, normal_depth, bufs, "ambientOcclusion")
        bufs += _device_buffers(state, 1, max(w * h * 4, 4))
        return _ao_image_call(state, nd, disk, _ao_params(disk, radius, bias, seed), bufs[-1])
    finally:
        _free_device_buffers(state, bufs)


class AmbientOcclusion:
    """Progressive ambient occlusion of a view (include/acgpt.h pt_ao_image with accumulate): every update(state) adds `samples` rays
    per pixel under a new seed — the pattern turned by another angle per pixel — and returns the AO image of all of them so far, float32
    [height, width].  The counts start over, silently, when the image size, the camera, the geometry or the reach differ from the last
    update.  Owns its device buffer: close() frees it, and so does CleanAllTheThings for the context."""

    def __init__(self, samples=16, radius=None, bias=None, disk=None):
        self.disk = _ao_disk(disk, samples, "AmbientOcclusion")
        self.radius, self.bias = radius, bias
        self.calls = 0              # the next call's seed
        self.total = 0              # rays per pixel so far
        self._state = None
        self._bufs = []             # visible
        self._key = None
        self._shape = None

    def _bind(self, state):
        if self._state is None:
            self._state = state
            state._temporal.append(self)
        elif self._state is not state:
            raise PathTracerError("AmbientOcclusion: bound to another PathTracerState")

    def reset(self):
        """The next update is a first one."""
        self.calls, self.total = 0, 0

    def update(self, state, normal_depth=None):
        self._bind(state)
        p = state.params
        w, h = int(p.width), int(p.height)
        radius, bias = _ao_reach(state, self.radius, self.bias, "AmbientOcclusion")
        key = Convergence._key_of(state)[:-1] + (state._verts_serial, radius, bias)
        if self._shape != (w, h):
            _free_device_buffers(state, self._bufs)
            self._bufs, self._shape = [], None
            self._bufs = _device_buffers(state, 1, max(w * h * 4, 4))
            self._shape, self._key = (w, h), None
        if key != self._key:
            self.reset()
            self._key = key
        K = self.disk.shape[0]
        bufs = []
        try:
            nd = _ao_features(state, normal_depth, bufs, "AmbientOcclusion")
            out = _ao_image_call(state, nd, self.disk, _ao_params(self.disk, radius, bias, self.calls, self.calls > 0, self.total + K), self._bufs[0])
        finally:
            _free_device_buffers(state, bufs)
        self.calls += 1
        self.total += K
        return out

    def visible(self):
        """uint32 [height, width]: the rays that found nothing, of `total` per pixel"""
        if self._state is None or not self.calls:
            raise PathTracerError("AmbientOcclusion.visible: update(state) first")
        w, h = self._shape
        out = np.zeros((h, w), np.uint32)
        _check(self._state.context, _native.hip().pt_copy_to_host(self._state.context, out.ctypes.data, self._bufs[0], out.nbytes), "copy to host")
        return out

    def close(self):
        state = self._state
        if state is None:
            return
        if state.context:
            _free_device_buffers(state, self._bufs)
        self._bufs, self._shape, self._key = [], None, None
        self.reset()
        if self in state._temporal:
            state._temporal.remove(self)
        self._state = None


def _bake_ao_tensor(state, points, normals, disk, ap):
    import torch
    for t, name in ((points, "points"),) + (((normals, "normals"),) if normals is not None else ()):
        if not _is_tensor(t):
            raise PathTracerError("bakeAO: points and normals must both be tensors or both arrays")
        if t.device.type != "cuda" or t.device.index != state._device:
            raise PathTracerError("bakeAO: the %s are on %s, the context is on cuda:%d" % (name, t.device, state._device))
        if t.dtype != torch.float32:
            raise PathTracerError("bakeAO: the %s must be float32, got %s" % (name, t.dtype))
        if t.dim() != 2 or t.shape[1] != (3 if normals is not None else 8) or t.shape[0] != points.shape[0]:
            raise PathTracerError("bakeAO: expected an (n, 8) tensor of records or (n, 3) points and normals, got shape %s" % (tuple(t.shape),))
    if normals is None and not points.is_contiguous():
        raise PathTracerError("bakeAO: the records must be contiguous (nothing is copied)")
    n = int(points.shape[0])
    with torch.cuda.device(points.device):
        rec = points
        if normals is not None:
            rec = torch.zeros((n, 8), dtype=torch.float32, device=points.device)      # the records the library reads, built by torch
            rec[:, 0:3] = points
            rec[:, 4:7] = normals
        visible = torch.empty((n,), dtype=torch.int32, device=points.device)
        ao = torch.empty((n,), dtype=torch.float32, device=points.device)
        torch.cuda.current_stream().synchronize()      # the records' producer and the allocations; the call below returns synchronised
    _check(state.context, _native.hip().pt_ao_points(state.context, rec.data_ptr() if n else None, n, disk.ctypes.data, C.byref(ap),
                                                     visible.data_ptr() if n else None, ao.data_ptr() if n else None), "pt_ao_points")
    return ao


def bakeAO(state, points, normals=None, samples=64, radius=None, bias=None, disk=None, seed=0):
    """Ambient occlusion at n surface points (include/acgpt.h pt_ao_points): the share of `samples` rays over the hemisphere of each
    point's normal that find nothing within `radius`.  points, normals: (n, 3) each — or, with normals None, points is the (n, 8) array
    of records the library reads: P.xyz, unused, N.xyz, unused.  The normals are used as they are (unit length is the caller's
    business); a point with a non-finite component or a zero normal comes out fully open.

    NumPy arrays (or anything np.asarray takes) go to the device and a float32 (n,) array comes back.  Float32 torch tensors on the
    context's device stay there and a float32 tensor on that device comes back: an (n, 8) tensor of records must be contiguous, nothing
    is copied and its data_ptr() goes straight in; (n, 3) points and normals are put into records by torch.  torch's current stream is
    synchronised before the call, and the call returns synchronised."""
    disk = _ao_disk(disk, samples, "bakeAO")
    if _is_tensor(points) or _is_tensor(normals):
        radius, bias = _ao_reach(state, radius, bias, "bakeAO")
        return _bake_ao_tensor(state, points, normals, disk, _ao_params(disk, radius, bias, seed))
    P = np.asarray(points)
    N = None if normals is None else np.asarray(normals)
    if P.ndim != 2 or P.shape[1] != (8 if N is None else 3) or (N is not None and N.shape != P.shape):
        raise PathTracerError("bakeAO: expected an (n, 8) array of records or (n, 3) points and normals, got shapes %s and %s" % (P.shape, None if N is None else N.shape))
    if P.dtype.kind not in "fiu" or (N is not None and N.dtype.kind not in "fiu"):
        raise PathTracerError("bakeAO: points and normals must be numbers, got %s" % P.dtype)
    n = P.shape[0]
    out = np.zeros(n, np.float32)
    if n == 0:
        return out
    radius, bias = _ao_reach(state, radius, bias, "bakeAO")
    rec = np.zeros((n, 8), np.float32)
    if N is None:
        rec[:] = P
    else:
        rec[:, 0:3] = P
        rec[:, 4:7] = N
    L = _native.hip()
    bufs = _device_buffers(state, 3, rec.nbytes)
    try:
        _check(state.context, L.pt_copy_to_device(state.context, bufs[0], rec.ctypes.data, rec.nbytes), "copy to device")
        ap = _ao_params(disk, radius, bias, seed)
        _check(state.context, L.pt_ao_points(state.context, bufs[0], n, disk.ctypes.data, C.byref(ap), bufs[1], bufs[2]), "pt_ao_points")
        _check(state.context, L.pt_copy_to_host(state.context, out.ctypes.data, bufs[2], out.nbytes), "copy to host")
    finally:
        _free_device_buffers(state, bufs)
    return out


def vertexNormals(verts, idx):
    """Area-weighted vertex normals, float32 (n_verts, 3): the sum of cross(v1 - v0, v2 - v0) over the triangles at a vertex (the cross
    product's length is twice the area), normalised; (0, 0, 0) at a vertex no triangle with an area uses."""
    v = np.asarray(verts, np.float64).reshape(len(verts), -1)[:, :3]
    t = np.asarray(idx, np.int64).reshape(-1, 3)
    c = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, t[:, k], c)
    length = np.sqrt((acc * acc).sum(axis=1, keepdims=True))
    return np.where(length > 0.0, acc / np.where(length > 0.0, length, 1.0), 0.0).astype(np.float32)


def bakeVertexAO(state, samples=64, radius=None, bias=None, disk=None, seed=0):
    """One ambient-occlusion value per vertex of the scene as it stands (after updateVertices: the moved one), float32 (n_verts,): bakeAO
    at the vertices with their area-weighted normals.  A vertex no triangle uses comes out 1."""
    if state._scene_verts is None:
        raise PathTracerError("bakeVertexAO: no scene (buildTheAccelarationStructure first)")
    verts = state._scene_verts[:, :3]
    return bakeAO(state, verts, vertexNormals(verts, state._scene_idx), samples=samples, radius=radius, bias=bias, disk=disk, seed=seed)


# pt_firefly_params' defaults (include/acgpt.h; DESIGN.md section 20 has the calibration)
FIREFLY_DEFAULTS = {"ratio": 16.0, "rank": 1, "radius": 1, "floor": 0.01}


def _firefly_params(settings, what):
    unknown = set(settings) - set(FIREFLY_DEFAULTS)
    if unknown:
        raise ValueError("%s: unknown firefly settings %s (known: %s)" % (what, sorted(unknown), sorted(FIREFLY_DEFAULTS)))
    d = dict(FIREFLY_DEFAULTS)
    d.update(settings)
    return _native.FireflyParams(float(d["ratio"]), float(d["floor"]), int(d["rank"]), int(d["radius"]))


def _firefly_info(info):
    total, removed = int(info.total_luma_q16), int(info.removed_luma_q16)
    return {"clamped_pixels": int(info.clamped_pixels), "replaced_pixels": int(info.replaced_pixels), "passed_pixels": int(info.passed_pixels),
            "total_luma_q16": total, "removed_luma_q16": removed, "max_ratio": float(info.max_ratio), "removed_share": removed / total if total else 0.0}


def fireflyFilter(state, image=None, ratio=FIREFLY_DEFAULTS["ratio"], rank=FIREFLY_DEFAULTS["rank"], radius=FIREFLY_DEFAULTS["radius"],
                  floor=FIREFLY_DEFAULTS["floor"]):
    """Outlier pixels clamped and invalid ones replaced (include/acgpt.h pt_firefly_filter): (float32 [height, width, 4], info).  image:
    None for the state's accumulation buffer, a device pointer to float4[height * width], or a float32 [height, width, 4] array
    (uploaded).  A pixel may be `ratio` times brighter than the rank-th brightest valid pixel of its (2 radius + 1)^2 window, taken no
    darker than `floor`.  info: clamped_pixels, replaced_pixels, passed_pixels, total_luma_q16, removed_luma_q16, max_ratio and
    removed_share, the part of the image's luminance the clamp took.  The source image is left as it is."""
    L = _native.hip()
    h, w = int(state.params.height), int(state.params.width)
    fp = _firefly_params({"ratio": ratio, "rank": rank, "radius": radius, "floor": floor}, "fireflyFilter")
    bufs = _device_buffers(state, 1, w * h * 16)
    try:
        src = _source_image(state, image, bufs, "fireflyFilter")
        info = _native.FireflyInfo()
        _check(state.context, L.pt_firefly_filter(state.context, src, w, h, C.byref(fp), bufs[0], C.byref(info)), "pt_firefly_filter")
        out = _read_image(state, bufs[0])
    finally:
        _free_device_buffers(state, bufs)
    return out, _firefly_info(info)


def _denoise_filtered(state, params, albedo, normal_depth, out, iterations, firefly, width, height):
    """pt_denoise of params' accumulation through pt_firefly_filter first: the filter writes a buffer of its own and the denoiser gets
    a copy of params that names it; params and the accumulation are left as they are."""
    L = _native.hip()
    fp = _firefly_params(firefly, "denoise")
    tmp = _device_buffers(state, 1, width * height * 16)
    try:
        _check(state.context, L.pt_firefly_filter(state.context, params.accumulationBuffer, width, height, C.byref(fp), tmp[0], None), "pt_firefly_filter")
        q = PathTraceParams()
        C.memmove(C.byref(q), C.byref(params), C.sizeof(q))
        q.accumulationBuffer = tmp[0]
        _check(state.context, L.pt_denoise(state.context, C.byref(q), albedo, normal_depth, out, int(iterations)), "pt_denoise")
    finally:
        _free_device_buffers(state, tmp)


def denoise(state, iterations=5, firefly=None):
    """The accumulation buffer through the edge-avoiding a-trous filter (include/acgpt.h pt_denoise), guided by the features of the
    current camera: float32 [height, width, 4] linear radiance, alpha 1.  The accumulation itself is left as it is.  firefly: None, or
    a dict of fireflyFilter's settings ({} for the defaults): the accumulation goes through pt_firefly_filter first."""
    nbytes = int(state.params.width) * int(state.params.height) * 16
    bufs = _device_buffers(state, 3, nbytes)
    try:
        L = _native.hip()
        _check(state.context, L.pt_render_features(state.context, C.byref(state.params), bufs[0], bufs[1]), "pt_render_features")
        if firefly is None:
            _check(state.context, L.pt_denoise(state.context, C.byref(state.params), bufs[0], bufs[1], bufs[2], int(iterations)), "pt_denoise")
        else:
            _denoise_filtered(state, state.params, bufs[0], bufs[1], bufs[2], iterations, firefly, int(state.params.width), int(state.params.height))
        return _read_image(state, bufs[2])
    finally:
        _free_device_buffers(state, bufs)


TONE_CURVES = {"linear": _native.TONE_LINEAR, "reinhard": _native.TONE_REINHARD, "aces": _native.TONE_ACES}


# pt_bloom_params' defaults (include/acgpt.h; DESIGN.md section 21 has the table the intensity was picked from)
BLOOM_DEFAULTS = {"threshold": 1.0, "knee": 0.5, "clamp": 0.0, "intensity": 0.02, "spread": 1.0, "levels": 6}


def _bloom_settings(settings, what):
    """BLOOM_DEFAULTS overlaid with `settings`, checked against pt_bloom_params' ranges here on the host"""
    unknown = set(settings) - set(BLOOM_DEFAULTS)
    if unknown:
        raise ValueError("%s: unknown bloom settings %s (known: %s)" % (what, sorted(unknown), sorted(BLOOM_DEFAULTS)))
    d = dict(BLOOM_DEFAULTS)
    d.update(settings)
    v = {k: float(d[k]) for k in ("threshold", "knee", "clamp", "intensity", "spread")}
    for k in ("threshold", "clamp", "intensity"):
        if not (np.isfinite(v[k]) and v[k] >= 0.0):
            raise ValueError("%s: %s must be finite and >= 0" % (what, k))
    if not (np.isfinite(v["knee"]) and 0.0 <= v["knee"] <= v["threshold"]):
        raise ValueError("%s: knee must be finite and in [0, threshold]" % what)
    if not (np.isfinite(v["spread"]) and 0.0 <= v["spread"] <= 4.0):
        raise ValueError("%s: spread must be finite and in [0, 4]" % what)
    if int(d["levels"]) != d["levels"] or not 1 <= int(d["levels"]) <= _native.BLOOM_MAX_LEVELS:
        raise ValueError("%s: levels must be an integer in [1, %d]" % (what, _native.BLOOM_MAX_LEVELS))
    v["levels"] = int(d["levels"])
    return v


def _bloom_params(v, exposure=None):
    """pt_bloom_params of checked settings; with an exposure, threshold, knee and clamp are in display units (multiples of exposed
    white) and are divided by it, in fp32"""
    t, k, c = (np.float32(v[name]) for name in ("threshold", "knee", "clamp"))
    if exposure is not None:
        e = np.float32(exposure)
        t, k, c = t / e, k / e, c / e
    return _native.BloomParams(float(t), float(k), float(c), v["intensity"], v["spread"], v["levels"])


def _bloom_info(info):
    total, bright = int(info.total_luma_q16), int(info.bright_luma_q16)
    return {"levels": int(info.levels), "bright_pixels": int(info.bright_pixels), "invalid_pixels": int(info.invalid_pixels), "total_luma_q16": total,
            "bright_luma_q16": bright, "max_luma": float(info.max_luma), "bright_share": bright / total if total else 0.0}


def bloom(state, image=None, threshold=BLOOM_DEFAULTS["threshold"], knee=BLOOM_DEFAULTS["knee"], clamp=BLOOM_DEFAULTS["clamp"],
          intensity=BLOOM_DEFAULTS["intensity"], spread=BLOOM_DEFAULTS["spread"], levels=BLOOM_DEFAULTS["levels"]):
    """The glare of the pixels brighter than `threshold` added to a linear HDR image (include/acgpt.h pt_bloom): (float32 [height,
    width, 4], info).  image: None for the state's accumulation buffer, a device pointer to float4[height * width], or a float32
    [height, width, 4] array (uploaded).  threshold, knee and clamp are in the image's radiance units here (displayTransform(bloom=)
    takes them in display units).  info: levels, bright_pixels, invalid_pixels, total_luma_q16, bright_luma_q16, max_luma and
    bright_share, the part of the image's luminance that went into the pyramid.  The source image is left as it is."""
    v = _bloom_settings({"threshold": threshold, "knee": knee, "clamp": clamp, "intensity": intensity, "spread": spread, "levels": levels}, "bloom")
    L = _native.hip()
    h, w = int(state.params.height), int(state.params.width)
    bp = _bloom_params(v)
    bufs = _device_buffers(state, 1, w * h * 16)
    try:
        src = _source_image(state, image, bufs, "bloom")
        info = _native.BloomInfo()
        _check(state.context, L.pt_bloom(state.context, src, w, h, C.byref(bp), bufs[0], C.byref(info)), "pt_bloom")
        out = _read_image(state, bufs[0])
    finally:
        _free_device_buffers(state, bufs)
    return out, _bloom_info(info)


def _display_info(info):
    return {"exposure": float(info.exposure), "metered_luminance": float(info.metered_luminance), "metered_pixels": int(info.metered_pixels),
            "unmetered_pixels": int(info.unmetered_pixels), "histogram": np.array(info.histogram, np.uint32)}


def _display_bloomed(state, image, dp, settings):
    """displayTransform(bloom=settings): the exposure first (metered on the image without its glare, or the manual one), pt_bloom with
    threshold, knee and clamp divided by it, then the curve at that exposure as a manual one"""
    L = _native.hip()
    h, w = int(state.params.height), int(state.params.width)
    bufs = _device_buffers(state, 1, w * h * 4) + _device_buffers(state, 1, w * h * 16)
    try:
        src = _source_image(state, image, bufs, "displayTransform")
        info = _native.DisplayInfo()
        if dp.exposure > 0.0:
            info.exposure = dp.exposure             # as the manual call reports it: nothing metered
        else:
            _check(state.context, L.pt_display_transform(state.context, src, w * h, C.byref(dp), None, bufs[0], C.byref(info)), "pt_display_transform")
        bp = _bloom_params(settings, info.exposure)
        binfo = _native.BloomInfo()
        _check(state.context, L.pt_bloom(state.context, src, w, h, C.byref(bp), bufs[1], C.byref(binfo)), "pt_bloom")
        manual = _native.DisplayParams()
        C.memmove(C.byref(manual), C.byref(dp), C.sizeof(manual))
        manual.exposure = info.exposure
        _check(state.context, L.pt_display_transform(state.context, bufs[1], w * h, C.byref(manual), None, bufs[0], None), "pt_display_transform")
        rgba = np.zeros((h, w, 4), np.uint8)
        _check(state.context, L.pt_copy_to_host(state.context, rgba.ctypes.data, bufs[0], rgba.nbytes), "copy to host")
    finally:
        _free_device_buffers(state, bufs)
    out = _display_info(info)
    out["bloom"] = _bloom_info(binfo)
    return rgba, out


def displayTransform(state, image=None, curve="aces", exposure=None, key=0.18, white=4.0, window=(100, 900), limits=(2.0 ** -16, 2.0 ** 16),
                     prev_exposure=None, adapt=1.0, bloom=None):
    """Exposure and tone mapping of a linear HDR image (include/acgpt.h pt_display_transform): (rgba8 [height, width, 4] with row 0 =
    bottom, info).  image: None for the state's accumulation buffer, a device pointer to float4[height * width], or a float32
    [height, width, 4] array (uploaded).  exposure: None for the histogram auto-exposure (key, window = (lo, hi) in permille of the
    metered pixels, limits = (min, max) exposure, prev_exposure / adapt for eye adaptation), else the manual factor.  curve: "linear",
    "reinhard" (white point `white`) or "aces".  info: exposure, metered_luminance, metered_pixels, unmetered_pixels, histogram.  The
    source image is left as it is.  bloom: None, or a dict of bloom()'s settings ({} for the defaults): the image goes through pt_bloom
    before the curve.  threshold, knee and clamp are then in display units, multiples of exposed white, and are divided by the
    exposure; an automatic exposure is metered on the image without its glare (one more pt_display_transform call, which honours
    prev_exposure and adapt) and applied as a manual one.  info is the metering call's, plus "bloom": bloom()'s info."""
    if curve not in TONE_CURVES:
        raise ValueError("displayTransform: curve must be one of %s" % sorted(TONE_CURVES))
    if exposure is not None and not float(exposure) > 0.0:
        raise ValueError("displayTransform: a manual exposure must be > 0 (None: automatic)")
    settings = None if bloom is None else _bloom_settings(bloom, "displayTransform")
    L = _native.hip()
    h, w = int(state.params.height), int(state.params.width)
    dp = _native.DisplayParams(TONE_CURVES[curve], 0.0 if exposure is None else float(exposure), float(key), float(white), int(window[0]), int(window[1]),
                               float(limits[0]), float(limits[1]), 0.0 if prev_exposure is None else float(prev_exposure), float(adapt))
    if settings is not None:
        return _display_bloomed(state, image, dp, settings)
    bufs = _device_buffers(state, 1, w * h * 4)
    try:
        src = _source_image(state, image, bufs, "displayTransform")
        info = _native.DisplayInfo()
        _check(state.context, L.pt_display_transform(state.context, src, w * h, C.byref(dp), None, bufs[0], C.byref(info)), "pt_display_transform")
        rgba = np.zeros((h, w, 4), np.uint8)
        _check(state.context, L.pt_copy_to_host(state.context, rgba.ctypes.data, bufs[0], rgba.nbytes), "copy to host")
    finally:
        _free_device_buffers(state, bufs)
    return rgba, _display_info(info)


class AutoExposure:
    """Eye adaptation over displayTransform: carries the exposure from call to call.  frame(state, dt) meters the image and moves the
    exposure towards its target by adapt = 1 - exp(-dt * speed), computed here on the host (dt in seconds since the last call; the
    first call jumps).  The other arguments are displayTransform's, bloom= among them: every frame then gets the glare, at the adapted
    exposure."""

    def __init__(self, speed=3.0, **settings):
        self.speed = float(speed)
        self.settings = settings
        self.exposure = None

    def adapt(self, dt):
        return float(min(1.0, max(0.0, 1.0 - np.exp(-float(dt) * self.speed))))

    def reset(self):
        self.exposure = None

    def frame(self, state, dt, image=None):
        rgba, info = displayTransform(state, image=image, prev_exposure=self.exposure, adapt=self.adapt(dt), **self.settings)
        self.exposure = info["exposure"]
        return rgba, info


TEMPORAL_HISTORY_CAP = 256.0      # include/acgpt.h pt_temporal_blend: the default cap, calibrated in tests/test_temporal_host.py
TEMPORAL_CLIP_GAMMA = 4.0         # include/acgpt.h PT_TEMPORAL_CLIP_GAMMA: the default clip, calibrated in tests/test_motion_host.py


class _TemporalView:
    """One view's device buffers: history {rgb, samples} and the two feature buffers, plus what they were made under."""

    def __init__(self):
        self.bufs = []              # history, albedo_prim, normal_depth
        self.pixels = 0
        self.params = PathTraceParams()
        self.key = None             # (width, height, camera) of the view
        self.samples = 0            # N of the accumulation the history was last blended from
        self.valid = False
        self.verts_buf = []         # motion=True: the positions the view was traced with, on the device ...
        self.verts = None           # ... and on the host
        self.verts_serial = 0


class TemporalHistory:
    """The accumulated image carried across camera moves (include/acgpt.h pt_temporal_blend).

    update(state) traces the current view's features and blends the history of the last view the camera left with the accumulation;
    the result is this view's history, and becomes the source when the camera moves on.  Called again at the same camera, it blends
    the same source with the newer accumulation (the accumulation already holds the samples the last call blended in).  The history
    is dropped, silently, when the scene, maxDepth, a toggle, the light mode or the math mode differ from what it was made under, and
    when the accumulation at an unmoved camera stands for fewer samples than last time (a reset).  Owns its device buffers: close()
    frees them, and so does CleanAllTheThings for the context.

    motion=True (pt_temporal_blend_motion): a vertex update (updateVertices) between two update() calls keeps the history.  Each view
    keeps the positions it was traced with; the blend moves every hit point by its triangle's motion between the two views, and clips
    the history mean to the current neighbourhood (TEMPORAL_CLIP_GAMMA) when the positions differ.  A new scene
    (buildTheAccelarationStructure), the toggles, the modes and a reset still drop it.

    A material edit (updateMaterials) drops the history in both modes: a changed material changes the lighting wherever its light
    reaches, not only on its own pixels, and the motion path's clip bounds only part of that."""

    def __init__(self, cap=TEMPORAL_HISTORY_CAP, motion=False):
        self.cap = float(cap)
        self.motion = bool(motion)
        self._state = None
        self._views = [_TemporalView(), _TemporalView()]
        self._cur = 0               # index of the view last blended into
        self._settings = None

    def _bind(self, state):
        if self._state is None:
            self._state = state
            state._temporal.append(self)
        elif self._state is not state:
            raise PathTracerError("TemporalHistory: bound to another PathTracerState")

    def _settings_of(self, state):
        p = state.params
        scene = ("scene", state._scene_serial) if self.motion else _native.hip().pt_scene_handle(state.context)
        return (scene, getattr(state, "_mats_serial", 0), int(p.maxDepth), int(p.useDirectLighting), int(p.useImportanceSampling),
                getattr(state, "_light_mode", 0) | (getattr(state, "_material_model", 0) << 8), getattr(state, "_math_mode", _native.MATH_FAST))

    def _key_of(self, state):
        p = state.params
        key = (int(p.width), int(p.height)) + tuple(v.tuple() for v in (p.cameraEye, p.cameraU, p.cameraV, p.cameraW))
        return key + (state._verts_serial,) if self.motion else key      # with motion, moved vertices make a new view

    def _drop(self):
        for v in self._views:
            v.valid = False

    def update(self, state, accum_samples=None):
        """Blend and keep: float32 [height, width, 4] {linear rgb, samples it stands for}.  accum_samples: the samples the
        accumulation stands for, by default currentFrameIdx * samplesPerPixel."""
        self._bind(state)
        L = _native.hip()
        p = state.params
        n = int(p.currentFrameIdx) * int(p.samplesPerPixel) if accum_samples is None else int(accum_samples)
        key, settings = self._key_of(state), self._settings_of(state)
        cur = self._views[self._cur]
        if settings != self._settings or (cur.valid and cur.key == key and n < cur.samples):
            self._drop()
        self._settings = settings
        if cur.valid and cur.key != key:                 # the camera moved: the last result is the history from now on
            self._cur ^= 1
        cur, prev = self._views[self._cur], self._views[self._cur ^ 1]
        pixels = int(p.width) * int(p.height)
        if cur.pixels != pixels:
            _free_device_buffers(state, cur.bufs)
            cur.bufs, cur.pixels = [], 0
            cur.bufs, cur.pixels = _device_buffers(state, 3, pixels * 16), pixels
        cur.valid = False
        C.memmove(C.byref(cur.params), C.byref(p), C.sizeof(p))
        hist, alb, nd = cur.bufs
        _check(state.context, L.pt_render_features(state.context, C.byref(p), alb, nd), "pt_render_features")
        if self.motion:
            rc = self._blend_motion(state, p, n, cur, prev)
        elif prev.valid:
            rc = L.pt_temporal_blend(state.context, C.byref(p), n, alb, nd, C.byref(prev.params), prev.bufs[0], prev.bufs[1], prev.bufs[2],
                                     self.cap, hist)
        else:
            rc = L.pt_temporal_blend(state.context, C.byref(p), n, alb, nd, None, None, None, None, self.cap, hist)
        _check(state.context, rc, "pt_temporal_blend")
        cur.key, cur.samples, cur.valid = key, n, True
        return _read_image(state, hist)

    def _blend_motion(self, state, p, n, cur, prev):
        """pt_temporal_blend_motion into cur, with the positions each view was traced with (uploaded into the views' own buffers)."""
        L = _native.hip()
        verts = state._scene_verts
        n_verts = verts.shape[0]
        if cur.verts_serial != state._verts_serial:
            if cur.verts is None or cur.verts.shape != verts.shape:
                _free_device_buffers(state, cur.verts_buf)
                cur.verts_buf, cur.verts = [], None
                cur.verts_buf = _device_buffers(state, 1, verts.nbytes)
            _check(state.context, L.pt_copy_to_device(state.context, cur.verts_buf[0], verts.ctypes.data, verts.nbytes), "vertex upload")
            cur.verts, cur.verts_serial = verts, state._verts_serial
        hist, alb, nd = cur.bufs
        if not prev.valid:
            return L.pt_temporal_blend_motion(state.context, C.byref(p), n, alb, nd, None, None, None, None, None, None, n_verts, self.cap, 0.0,
                                              hist)
        gamma = TEMPORAL_CLIP_GAMMA if not np.array_equal(prev.verts, cur.verts) else 0.0
        return L.pt_temporal_blend_motion(state.context, C.byref(p), n, alb, nd, C.byref(prev.params), prev.bufs[0], prev.bufs[1], prev.bufs[2],
                                          cur.verts_buf[0], prev.verts_buf[0], n_verts, self.cap, gamma, hist)

    def denoise(self, state, iterations=5, firefly=None):
        """The last update's history through pt_denoise (guided by the same features): float32 [height, width, 4], alpha 1.  firefly:
        None, or a dict of fireflyFilter's settings: the history goes through pt_firefly_filter first (and is left as it is)."""
        cur = self._views[self._cur]
        if self._state is not state or not cur.valid:
            raise PathTracerError("TemporalHistory.denoise: update(state) first")
        q = PathTraceParams()
        C.memmove(C.byref(q), C.byref(cur.params), C.sizeof(q))
        q.accumulationBuffer = cur.bufs[0]              # pt_denoise reads .xyz only
        out = _device_buffers(state, 1, cur.pixels * 16)
        try:
            if firefly is None:
                _check(state.context, _native.hip().pt_denoise(state.context, C.byref(q), cur.bufs[1], cur.bufs[2], out[0], int(iterations)), "pt_denoise")
            else:
                _denoise_filtered(state, q, cur.bufs[1], cur.bufs[2], out[0], iterations, firefly, int(q.width), int(q.height))
            h, w = int(q.height), int(q.width)
            img = np.zeros((h, w, 4), np.float32)
            _check(state.context, _native.hip().pt_copy_to_host(state.context, img.ctypes.data, out[0], img.nbytes), "copy to host")
            return img
        finally:
            _free_device_buffers(state, out)

    def close(self):
        state = self._state
        if state is None:
            return
        if state.context:
            for v in self._views:
                _free_device_buffers(state, v.bufs)
                _free_device_buffers(state, v.verts_buf)
        for v in self._views:
            v.bufs, v.pixels, v.valid = [], 0, False
            v.verts_buf, v.verts, v.verts_serial = [], None, 0
        if self in state._temporal:
            state._temporal.remove(self)
        self._state = None


class Convergence:
    """The noise of the accumulated image, and a stopping rule (include/acgpt.h pt_convergence_update).

    update(state) after every launch (or batch of frames) feeds the accumulation to the per-pixel estimate and returns the info
    record as a dict; `converged` is then true when every pixel has an error, none is invalid and at least `permille` of them have
    a relative standard error <= threshold.  errorImage() is the per-pixel error, float32 [height, width] with row 0 = bottom and
    -1 where a pixel has none yet; tiles() the max per 16 x 16 tile, float32 [ceil(height / 16), ceil(width / 16)].  The state is
    zero-filled, silently, when the image size, the camera or the samples per frame differ from the last update; an accumulation
    that was restarted (fewer frames than last time) restarts its pixels by itself.  Owns its device buffers: close() frees
    them, and so does CleanAllTheThings for the context.  maps=False leaves the error image and the tiles out."""

    def __init__(self, threshold=0.02, permille=950, floor=0.01, maps=True):
        self.threshold, self.permille, self.floor = float(threshold), int(permille), float(floor)
        self.maps = bool(maps)
        self.info = None
        self._state = None
        self._bufs = []             # state, then out_error and out_tiles
        self._key = None
        self._shape = None

    def _bind(self, state):
        if self._state is None:
            self._state = state
            state._temporal.append(self)
        elif self._state is not state:
            raise PathTracerError("Convergence: bound to another PathTracerState")

    @staticmethod
    def _key_of(state):
        p = state.params
        return (int(p.width), int(p.height)) + tuple(v.tuple() for v in (p.cameraEye, p.cameraU, p.cameraV, p.cameraW)) + (int(p.samplesPerPixel),)

    @property
    def converged(self):
        i = self.info
        return bool(i) and i["unmeasured_pixels"] == 0 and i["invalid_pixels"] == 0 and i["converged_pixels"] * 1000 >= i["measured_pixels"] * self.permille

    def reset(self):
        """Zero-fill the state: the next update is a first observation."""
        if self._bufs:
            w, h = self._shape
            _check(self._state.context, _native.hip().pt_device_memset(self._state.context, self._bufs[0], 0, w * h * 16), "state clear")
        self.info = None

    def update(self, state, accum_frames=None):
        """accum_frames: the frames the accumulation stands for, by default currentFrameIdx (which the caller advances after a
        launch)."""
        self._bind(state)
        L = _native.hip()
        p = state.params
        w, h = int(p.width), int(p.height)
        key = self._key_of(state)
        if self._shape != (w, h):
            _free_device_buffers(state, self._bufs)
            self._bufs, self._shape = [], None
            tiles = ((w + _native.CONVERGENCE_TILE - 1) // _native.CONVERGENCE_TILE) * ((h + _native.CONVERGENCE_TILE - 1) // _native.CONVERGENCE_TILE)
            self._bufs = _device_buffers(state, 1, w * h * 16)
            if self.maps:
                self._bufs += _device_buffers(state, 1, w * h * 4) + _device_buffers(state, 1, tiles * 4)
            self._shape, self._key = (w, h), None
        if key != self._key:
            self.reset()
            self._key = key
        n = int(p.currentFrameIdx) if accum_frames is None else int(accum_frames)
        cp = _native.ConvergenceParams(self.floor, self.threshold, self.permille, 0)
        info = _native.ConvergenceInfo()
        err, til = (self._bufs[1], self._bufs[2]) if self.maps else (None, None)
        _check(state.context, L.pt_convergence_update(state.context, C.byref(p), n, C.byref(cp), self._bufs[0], err, til, C.byref(info)), "pt_convergence_update")
        self.info = {"frames": int(info.frames), "measured_pixels": int(info.measured_pixels), "unmeasured_pixels": int(info.unmeasured_pixels),
                     "invalid_pixels": int(info.invalid_pixels), "converged_pixels": int(info.converged_pixels), "max_error": float(info.max_error),
                     "quantile_error": float(info.quantile_error), "histogram": np.array(info.histogram, np.uint32)}
        return self.info

    def _read(self, index, shape, what):
        if self._state is None or self.info is None or not self.maps:
            raise PathTracerError("Convergence.%s: update(state) first (with maps=True)" % what)
        out = np.zeros(shape, np.float32)
        _check(self._state.context, _native.hip().pt_copy_to_host(self._state.context, out.ctypes.data, self._bufs[index], out.nbytes), "copy to host")
        return out

    def stateImage(self):
        """float32 [height, width, 4] {l0, M2, k0, B} (row 0 = bottom)."""
        if self._state is None or not self._bufs:
            raise PathTracerError("Convergence.stateImage: update(state) first")
        w, h = self._shape
        out = np.zeros((h, w, 4), np.float32)
        _check(self._state.context, _native.hip().pt_copy_to_host(self._state.context, out.ctypes.data, self._bufs[0], out.nbytes), "copy to host")
        return out

    def errorImage(self):
        w, h = self._shape or (0, 0)
        return self._read(1, (h, w), "errorImage")

    def tiles(self):
        w, h = self._shape or (0, 0)
        t = _native.CONVERGENCE_TILE
        return self._read(2, ((h + t - 1) // t, (w + t - 1) // t), "tiles")

    def close(self):
        state = self._state
        if state is None:
            return
        if state.context:
            _free_device_buffers(state, self._bufs)
        self._bufs, self._shape, self._key, self.info = [], None, None, None
        if self in state._temporal:
            state._temporal.remove(self)
        self._state = None


def renderUntil(output_buffer, state, conv, max_frames, sub_frames=1):
    """Launch and update until conv.converged or the accumulation stands for max_frames frames: sub_frames frames per launch
    (LaunchCurrentFrame; the last batch is cut to the cap), currentFrameIdx advanced here, one conv.update per launch.  Returns the
    frames the accumulation stands for."""
    sub_frames = max(1, int(sub_frames))
    while int(state.params.currentFrameIdx) < int(max_frames):
        n = min(sub_frames, int(max_frames) - int(state.params.currentFrameIdx))
        LaunchCurrentFrame(output_buffer, state, n)
        state.params.currentFrameIdx += n
        conv.update(state)
        if conv.converged:
            break
    return int(state.params.currentFrameIdx)


def saveAccumulation(state, filename):
    """The progressive state of the reference — params.accumulationBuffer and currentFrameIdx
    (pathTracerPrograms.cu:803-811) — as a file; same format as acgpt_main --save-accum."""
    acc = readAccumulation(state)
    with open(filename, "wb") as fh:
        fh.write(b"ACGPTACC")
        fh.write(np.array([state.params.width, state.params.height, state.params.currentFrameIdx], np.uint32).tobytes())
        fh.write(acc.tobytes())


def restoreAccumulation(state, filename):
    """Continue a saved run: fills params.accumulationBuffer and sets currentFrameIdx to the frames accumulated so far."""
    if state.refreshAccumulationBuffer:      # a pending reset (setMathMode, setLightMode, a key toggle) would discard what is restored here
        updateState(None, state)
    h, w = int(state.params.height), int(state.params.width)
    with open(filename, "rb") as fh:
        blob = fh.read()
    hdr = np.frombuffer(blob[8:20], np.uint32) if len(blob) >= 20 else None
    if blob[:8] != b"ACGPTACC" or hdr is None or int(hdr[0]) != w or int(hdr[1]) != h or len(blob) != 20 + h * w * 16:
        raise PathTracerError("%s is not an accumulation dump of a %dx%d image" % (filename, w, h))
    acc = np.frombuffer(blob[20:], np.float32).copy()
    _check(state.context, _native.hip().pt_copy_to_device(state.context, state.params.accumulationBuffer, acc.ctypes.data, acc.nbytes),
           "restoreAccumulation")
    state.params.currentFrameIdx = int(hdr[2])


def saveImage(filename, rgba):
    """sutil::saveImage conventions (sutil/sutil.cpp:542-655): `rgba` is uint8 [height, width, 4] with row 0
    at the BOTTOM; the file is written top-down; alpha is dropped.  Suffix .ppm or .png."""
    a = np.ascontiguousarray(rgba, np.uint8)
    h, w = a.shape[0], a.shape[1]
    if _native.host().pth_save_image(os.fsencode(filename), a.ctypes.data, w, h) != 0:
        raise PathTracerError("cannot write %s" % filename)


def keyCallback(state, key):
    """PathTracerMain.cpp:100-141.  key: '0' direct lighting, '1' importance sampling,
    'UP' / 'DOWN' max depth +-1 clamped to [1, 28], 'R' reset.  Every change resets accumulation."""
    p = state.params
    if key == "0":
        p.useDirectLighting = 0 if p.useDirectLighting else 1
        state.refreshAccumulationBuffer = True
    elif key == "1":
        p.useImportanceSampling = 0 if p.useImportanceSampling else 1
        state.refreshAccumulationBuffer = True
    elif key == "UP":
        p.maxDepth = min(maxiumumRecursionDepth, int(p.maxDepth) + 1)
        state.refreshAccumulationBuffer = True
    elif key == "DOWN":
        p.maxDepth = max(1, int(p.maxDepth) - 1)
        state.refreshAccumulationBuffer = True
    elif key == "R":
        state.refreshAccumulationBuffer = True


def CleanAllTheThings(state):
    """PathTracerMain.cpp:629-646."""
    L = _native.hip()
    if state.context:
        for hist in list(getattr(state, "_temporal", ())):
            hist.close()
        if state.params.accumulationBuffer:
            L.pt_device_free(state.context, state.params.accumulationBuffer)
            state.params.accumulationBuffer = None
        L.pt_destroy(state.context)
        state.context = None


def setup(obj_path, width=512, height=512, max_depth=4, direct_lighting=False, importance_sampling=False,
          spp=samples_per_launch, device_id=0, build_mode=None, device_ids=None, math_mode=None):
    """The body of main() up to the frame loop (PathTracerMain.cpp:650-684) as one call.  math_mode: None (the library's default,
    "fast"), "ieee" or "fast" (setMathMode)."""
    obj = TinyObjWrapper(obj_path)
    if not obj.dataLoaded:
        raise PathTracerError("cannot load %s: %s" % (obj_path, obj.error))
    state = PathTracerState()
    state.params.width, state.params.height = int(width), int(height)
    state.params.useDirectLighting = 1 if direct_lighting else 0
    state.params.useImportanceSampling = 1 if importance_sampling else 0
    state.params.maxDepth = int(max_depth)
    cam = initCamera()
    cam.setAspectRatio(np.float32(width) / np.float32(height))
    state.params.cameraEye = _f3(cam.eye())
    U, V, W = cam.UVWFrame()
    state.params.cameraU, state.params.cameraV, state.params.cameraW = _f3(U), _f3(V), _f3(W)
    createDeviceContext(state, device_id, device_ids)
    if build_mode is not None:
        _check(state.context, _native.hip().pt_set_build_mode(state.context, int(build_mode)), "pt_set_build_mode")
    buildTheAccelarationStructure(state, obj)
    createModule(state); createProgramGroups(state); createPipeline(state)
    createShaderBindingTable(state, obj)
    initializeTheLaunch(state)
    state.params.samplesPerPixel = int(spp)
    if math_mode is not None:
        setMathMode(state, math_mode)
    return state, obj
