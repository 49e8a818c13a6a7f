"""Case tables of tests/test_gpu_small_kernel_cases.py: cameras, sample shapes, toggles and the scenes of the stack-depth cases of the
small-scene render path (csrc/render_small.hip).  Plain data and NumPy: no GPU, no library.  tests/test_small_kernel_cases_host.py
holds every table to what its names claim."""
import itertools

import numpy as np

F = np.float32

# ---- cameras -----------------------------------------------------------------------------------------------------------------------
# the reference's view of the Cornell box (eye, look-at, up, vertical field of view in degrees) and the box of cornell_box_diffuse.obj
REF_EYE, REF_LOOKAT, REF_UP, REF_FOVY = (278.0, 273.0, -900.0), (278.0, 273.0, 330.0), (0.0, 1.0, 0.0), 35.0
SCENE_LO, SCENE_HI = (0.0, 0.0, 0.0), (556.0, 548.8, 559.2)

CAMERAS = ("reference", "inside", "pulled_back", "off_axis", "grazing", "away")
PARTIAL_CAMERAS = ("pulled_back", "off_axis", "grazing")


def cull_box(lo=SCENE_LO, hi=SCENE_HI):
    """the scene box as the camera-ray cull of launch_batch sees it: grown by ext / 1024 + 1e-6, float32 arithmetic"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    grow = F((hi - lo).max() * F(1.0 / 1024.0) + F(1e-6))
    return (lo - grow).astype(np.float64), (hi + grow).astype(np.float64)


def reference_frame(aspect):
    """(eye, U, V, W) of the reference camera at an aspect ratio: W to the look-at point, V and U spanning the field of view there"""
    eye, up = np.array(REF_EYE), np.array(REF_UP)
    W = np.array(REF_LOOKAT) - eye
    U = np.cross(W, up); U /= np.linalg.norm(U)
    V = np.cross(U, W); V /= np.linalg.norm(V)
    vlen = np.linalg.norm(W) * np.tan(0.5 * np.radians(REF_FOVY))
    return eye, U * (vlen * aspect), V * vlen, W


def _turn(v, deg):
    """v turned about the y axis"""
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2]])


def camera(name, w, h):
    """(eye, U, V, W) as float32 [3] each, for a w x h image"""
    eye, U, V, W = reference_frame(w / h)
    lo, hi = cull_box()
    if name == "inside":                     # in the middle of the room, looking at the back wall
        eye = np.array([278.0, 273.0, 280.0])
    elif name == "pulled_back":              # 4000 units in front of the box, the horizontal field narrowed until the front face spans every column:
        eye = np.array([278.0, 273.0, -4000.0])       # the box fills the full width of a band of rows, a fifth of the image
        U = U * (0.06 * np.linalg.norm(W) / np.linalg.norm(U))
    elif name == "off_axis":                 # turned by 20 degrees: the box leaves the image through one vertical edge
        U, W = _turn(U, 20.0), _turn(W, 20.0)
    elif name == "grazing":                  # turned until the nearest vertical edge of the (grown) box is 1.25 columns inside the image
        edge = np.arctan2(hi[0] - eye[0], lo[2] - eye[2])
        tan_half = np.linalg.norm(U) / np.linalg.norm(W)
        inner = np.arctan(tan_half * (1.0 - 2.0 * 1.25 / w))
        U, W = _turn(U, np.degrees(edge + inner)), _turn(W, np.degrees(edge + inner))
    elif name == "away":                     # the reference camera turned round
        U, W = -U, -W
    elif name != "reference":
        raise KeyError(name)
    return tuple(np.asarray(x, F) for x in (eye, U, V, W))


def aimed(target, eye, span, w, h):
    """(eye, U, V, W) of a camera at `eye` looking at `target`, `span` units of the target's plane from top to bottom"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    W = target - eye
    up = np.array([0.0, 1.0, 0.0])
    U = np.cross(W, up); U /= np.linalg.norm(U)
    V = np.cross(U, W); V /= np.linalg.norm(V)
    return tuple(np.asarray(x, F) for x in (eye, U * (0.5 * span * w / h), V * (0.5 * span), W))


def reach(cam, w, h, lo=SCENE_LO, hi=SCENE_HI):
    """bool [h, w]: does the ray through the pixel centre hit the grown scene box (float64 slabs)"""
    eye, U, V, W = (np.asarray(x, np.float64) for x in cam)
    blo, bhi = cull_box(lo, hi)
    dx = 2.0 * (np.arange(w) + 0.5) / w - 1.0
    dy = 2.0 * (np.arange(h) + 0.5) / h - 1.0
    D = dx[None, :, None] * U + dy[:, None, None] * V + W
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (blo - eye) / D, (bhi - eye) / D
    tn = np.fmax(np.minimum(t0, t1).max(axis=-1), 0.0)
    tf = np.maximum(t0, t1).min(axis=-1)
    return tn <= tf


# ---- sample shapes -----------------------------------------------------------------------------------------------------------------
# (samples per pixel, pt_set_sample_chunks value (0: automatic), frames of one pt_launch_frames)
SAMPLE_SHAPES = (
    (64, 0, 1),      # chunk_shift 4
    (32, 0, 4),      # 3, and 4 << 3 = 32
    (16, 0, 3),      # 2, three sub-frames in four slots
    (8, 0, 2),       # 1
    (4, 0, 5),       # 0 with an even count
    (7, 0, 2),       # odd: 0
    (1, 0, 1),       # one sample, one frame: one item a pixel
    (1, 0, 7),
    (64, 0, 2),      # 2 << 4 = 32
    (64, 32, 1),     # 32 explicit runs: the LCG skip table to its last entry
    (48, 16, 2),     # explicit runs of three samples
    (6, 2, 3),
)


def shifts(spp, chunks, frames, pixels=96 * 64):
    """(chunk_shift, sub_shift) of launch_batch for one rank"""
    if chunks > 0:
        assert spp % chunks == 0
        cs = chunks.bit_length() - 1
    else:
        cs = 4 if pixels < (1 << 20) else 3
        while cs > 0 and (spp % (1 << cs) != 0 or (spp >> cs) < 4):
            cs -= 1
    ss = cs
    while (1 << (ss - cs)) < frames:
        ss += 1
    return cs, ss


# ---- toggles -----------------------------------------------------------------------------------------------------------------------
# (direct lighting, importance sampling, maxDepth)
TOGGLES = tuple(itertools.product((False, True), (False, True), (1, 4, 28)))

# ---- scenes of the stack-depth cases -----------------------------------------------------------------------------------------------
# (verts float32 [n, 4], indices uint32 [t, 3], material ids uint32 [t]); materials: 0 white, 1 red, 2 green
ROOM = (556.0, 548.8, 559.2)


def _pack(tris, ids):
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    v = np.ones((len(tris) * 3, 4), F)
    v[:, :3] = tris.reshape(-1, 3)
    return v, np.arange(len(tris) * 3, dtype=np.uint32).reshape(-1, 3), np.asarray(ids, np.uint32)


def _room():
    """floor, ceiling, back, right and left wall of a Cornell box, two triangles each, open towards the reference camera"""
    X, Y, Z = ROOM
    quads = [((0, 0, 0), (X, 0, 0), (X, 0, Z), (0, 0, Z), 0), ((0, Y, 0), (0, Y, Z), (X, Y, Z), (X, Y, 0), 0),
             ((0, 0, Z), (X, 0, Z), (X, Y, Z), (0, Y, Z), 0), ((0, 0, 0), (0, 0, Z), (0, Y, Z), (0, Y, 0), 1),
             ((X, 0, 0), (X, Y, 0), (X, Y, Z), (X, 0, Z), 2)]
    tris, ids = [], []
    for a, b, c, d, m in quads:
        tris += [(a, b, c), (a, c, d)]
        ids += [m, m]
    return tris, ids


def lattice(nx, nz):
    """nx x nz cells of two triangles over the floor of the room, heights on a gentle egg-box so that the cells shade and shadow"""
    X, _, Z = ROOM
    i, k = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="ij")
    P = np.stack([X * i / nx, 60.0 + 40.0 * np.sin(0.9 * i) * np.cos(0.7 * k), Z * k / nz], axis=-1)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    tris = np.concatenate([np.stack([a, b, c], axis=2).reshape(-1, 3, 3), np.stack([a, c, d], axis=2).reshape(-1, 3, 3)])
    return _pack(tris, np.arange(len(tris)) % 3)


def tail_centres(steps):
    """centres of the tail: every step halves one coordinate in turn, so every step is one level of a Morton-ordered tree"""
    X, Y, Z = ROOM
    k = np.arange(steps)
    return np.stack([X * 0.5 ** (1 + (k + 2) // 3), Y * 0.5 ** (1 + (k + 1) // 3), Z * 0.5 ** (1 + k // 3)], axis=-1)


def tail(steps, copies):
    """a room, `steps` triangles shrinking towards its corner at the origin and `copies` coincident copies of the last one;
    the triangles face the room's diagonal"""
    tris, ids = _room()
    c = tail_centres(steps)
    s = 0.3 * c.min(axis=1)[:, None]
    one = np.stack([c + s * np.array([1.0, -1.0, 0.0]), c + s * np.array([0.0, 1.0, -1.0]), c + s * np.array([-1.0, 0.0, 1.0])], axis=1)
    one = np.concatenate([one, np.repeat(one[-1:], copies, axis=0)])
    return _pack(np.concatenate([np.asarray(tris, np.float64), one]), ids + [(1 + j) % 3 for j in range(len(one))])


def tail_camera(steps, w, h):
    """looks at the coincident copies from the side, three times their distance to the corner away: the end of the tail and the corner
    fill the image, the larger triangles of the tail are beside and behind the eye"""
    c = tail_centres(steps)[-1]
    r = np.linalg.norm(c)
    d = np.array([1.0, 0.2, 0.1])
    return aimed(c, c + 3.0 * r * d / np.linalg.norm(d), 2.5 * r, w, h)


def spread(verts, n_room=10):
    """the triangles behind the room's moved onto a regular grid above the floor, each shrunk to a cell: the same arrays' shapes, a shallow tree"""
    v = verts.copy().reshape(-1, 3, 4)
    n = len(v) - n_room
    side = int(np.ceil(np.sqrt(n)))
    j = np.arange(n)
    cell = np.array([ROOM[0] / side, ROOM[2] / side])
    base = np.stack([(j % side + 0.5) * cell[0], np.full(n, 120.0), (j // side + 0.5) * cell[1]], axis=-1)
    shape = np.array([[-0.4, 0.0, -0.4], [0.4, 0.0, -0.4], [0.0, 30.0, 0.4]]) * np.array([cell[0], 1.0, cell[1]])
    v[n_room:, :, :3] = (base[:, None, :] + shape[None, :, :]).astype(F)
    return v.reshape(-1, 4)
