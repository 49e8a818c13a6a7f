"""NumPy statement of pt_ao_points / pt_ao_image (include/acgpt.h states the same definition): the rays of every point, the counts
and the division.

Everything is float32 / uint32 in the operation order of csrc/ao.hip — plain multiplies and adds, left to right, IEEE division and
square root — so the rays here are the kernel's rays bit for bit, and the kernel's counts are the any-hit query's answers on them.
A point that is no surface gets rays with a NaN origin: a miss before any traversal under pt_query_any's rules, so it counts K."""
import numpy as np

import query_ref as qr

F = np.float32
U32 = np.uint32


def tea4(v0, v1):
    """tea4 (csrc/pt_device.h) on uint32 arrays: four rounds of TEA, the first word"""
    v0, v1 = np.broadcast_arrays(np.asarray(v0, U32), np.asarray(v1, U32))
    v0, v1 = v0.astype(U32).reshape(-1), v1.astype(U32).reshape(-1)
    s0 = U32(0)
    with np.errstate(over="ignore"):
        for _ in range(4):
            s0 = U32((int(s0) + 0x9e3779b9) & 0xFFFFFFFF)
            v0 = v0 + ((((v1 << U32(4)) + U32(0xa341316c)) ^ (v1 + s0)) ^ ((v1 >> U32(5)) + U32(0xc8013ea4)))
            v1 = v1 + ((((v0 << U32(4)) + U32(0xad90777d)) ^ (v0 + s0)) ^ ((v0 >> U32(5)) + U32(0x7e95761e)))
    return v0


def rotation(h):
    """(c, s, q) of the hash h: the rational point of the unit circle at a = (h & 0xFFFF) / 2^16, then q = (h >> 16) & 3 exact
    quarter turns"""
    h = np.asarray(h, U32)
    a = (h & U32(0xFFFF)).astype(F) * F(2.0 ** -16)
    a2 = a * a
    den = F(1.0) + a2
    c0, s0 = (F(1.0) - a2) / den, (a + a) / den
    q = (h >> U32(16)) & U32(3)
    c = np.select([q == 1, q == 2, q == 3], [-s0, -c0, s0], c0).astype(F)
    s = np.select([q == 1, q == 2, q == 3], [c0, -s0, -c0], s0).astype(F)
    return c, s, q


def frame(N):
    """(T, S) of Duff et al. 2017 for normals N [n, 3]"""
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    with np.errstate(all="ignore"):
        sg = np.copysign(F(1.0), nz)
        A = F(-1.0) / (sg + nz)
        B = nx * ny * A
        T = np.stack([F(1.0) + sg * nx * nx * A, sg * B, -sg * nx], axis=1)
        S = np.stack([B, sg + ny * ny * A, -ny], axis=1)
    return T.astype(F), S.astype(F)


def surface(points, normals):
    """False where a point is no surface: a non-finite component of P or N, or N = (0, 0, 0)"""
    P, N = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    return np.isfinite(P).all(axis=1) & np.isfinite(N).all(axis=1) & ~(N == 0).all(axis=1)


def rays(points, normals, disk, params, first=0):
    """The (n * K, 8) rays of the n points, point-major (ray i * K + k is sample k of point i): {o, d, tmin 0, tmax radius}.
    params: {"radius", "bias", "seed"}; K = len(disk); first: the index of points[0] (the hash takes the point's index)."""
    P, N = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    disk = np.asarray(disk, F).reshape(-1, 2)
    n, K = P.shape[0], disk.shape[0]
    c, s, _ = rotation(tea4(np.arange(first, first + n, dtype=np.uint64).astype(U32), U32(params["seed"])))
    with np.errstate(all="ignore"):
        T, S = frame(N)
        o = P + F(params["bias"]) * N
        x, y = disk[None, :, 0], disk[None, :, 1]
        xr = c[:, None] * x - s[:, None] * y
        yr = s[:, None] * x + c[:, None] * y
        z = np.sqrt(np.fmax(F(0.0), (F(1.0) - xr * xr) - yr * yr))
        d = (xr[..., None] * T[:, None, :] + yr[..., None] * S[:, None, :]) + z[..., None] * N[:, None, :]
    assert d.dtype == F and o.dtype == F
    out = np.zeros((n, K, 8), F)
    out[:, :, 0:3] = np.where(surface(P, N)[:, None], o, F(np.nan))[:, None, :]
    out[:, :, 3:6] = d
    out[:, :, 7] = F(params["radius"])
    return out.reshape(n * K, 8)


def image_points(normal_depth, camera, w, h):
    """(points, normals) [w * h, 3] of pt_ao_image from pt_render_features' normal_depth [h, w, 4] and camera = (eye, U, V, W):
    P = eye + t * dir per component, dir the pixel-centre direction (denoise_ref.pixel_rays).  A pixel with normal_depth.w < 0 is no
    surface: its point is NaN."""
    import denoise_ref as dr
    nd = np.asarray(normal_depth, F).reshape(w * h, 4)
    r = dr.pixel_rays(w, h, *camera)
    with np.errstate(all="ignore"):
        P = r[:, 0:3] + nd[:, 3:4] * r[:, 3:6]
        P = np.where((nd[:, 3] < F(0.0))[:, None], F(np.nan), P).astype(F)
    return P, nd[:, 0:3].copy()


def occlusion_points(verts, idx, camera):
    """(points, normals) [SET_SIZE, 3] of the GPU tests: the origins of query_ref's "occlusion" ray set — random points on random
    triangles — with their triangles' geometric normals, normalize(cross(e1, e2)) as the scene build computes it"""
    r = qr.ray_set("occlusion", verts, idx, camera)
    v = np.asarray(verts, F).reshape(-1, 4)[:, :3]
    t = np.asarray(idx, U32).reshape(-1, 3)
    tri = v[t[np.random.default_rng(303).integers(0, t.shape[0], qr.SET_SIZE)]]          # ray_set's first draw: the triangles
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    inv = F(1.0) / np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    # the points lie in their triangles' planes: the draw above is the one the origins were made from
    assert (np.abs(((r[:, 0:3] - tri[:, 0]) * (c * inv[:, None])).sum(axis=1)) <= F(1e-2)).all()
    return r[:, 0:3].copy(), (c * inv[:, None]).astype(F)


def gpu_test_parameters(verts, idx):
    """What tests/test_gpu_ao.py shoots with: the reach of the Python wrappers' defaults, a quarter and a thousandth of the scene box's
    diagonal, as fp32"""
    lo, hi = qr.scene_box(verts, idx)
    diag = float(np.sqrt(((hi.astype(np.float64) - lo.astype(np.float64)) ** 2).sum()))
    return {"radius": float(F(0.25 * diag)), "bias": float(F(1e-3 * diag)), "seed": 0}


def counts(occluded, the_rays, K):
    """visible [n] uint32 from the any-hit answers on rays(): the rays that are not occluded; a ray that is a miss before any
    traversal is not, whatever `occluded` says"""
    occ = np.asarray(occluded).astype(bool) & qr.traceable(the_rays)
    return (K - occ.reshape(-1, K).sum(axis=1)).astype(U32)


def ao_value(visible, total_samples):
    """float(visible) / float(total_samples), one fp32 division"""
    return np.asarray(visible, U32).astype(F) / F(U32(total_samples))
