"""NumPy reference of pt_temporal_blend (include/acgpt.h states the same definition), and the orbited camera of acgpt_main --orbit.

Everything is fp32 in the operation order of csrc/temporal.hip, taps ty-major, so that the GPU result agrees with this one bit for
bit: the kernel has no transcendental, and the ray directions are those of denoise_ref.pixel_rays, which pt_render_features matches
exactly.  A rejected tap adds nothing here, as it is skipped there.  Images are [h, w, 4] float32 with row 0 at the bottom.

dtype=np.float64 evaluates the same formulas from the same fp32 inputs in double precision.  The rules for invalid inputs are those
of include/acgpt.h: a non-finite accumulation pixel passes through, a non-finite history tap is not accepted, a blend that is not
finite passes through.  No expression here leaves the treatment of a NaN to a library's maximum or minimum."""
import ctypes as C

import numpy as np

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native
import denoise_ref as dr

F = np.float32
BSDF_DIFFUSE = 0


# ---- cameras -------------------------------------------------------------------------------------------------------------------
def orbit_camera(w, h, dx, dy=0):
    """(eye, U, V, W) of the reference's camera (PathTracerMain.cpp:228-233, aspect w / h) after acgpt_main's --orbit dx,dy: the
    same Trackball script (look-at fixed, move speed 10, gimbal lock, startTracking(0, 0), updateTracking(dx, dy, w, h)) through the
    host library, then Camera::UVWFrame.  0.5 degree per pixel: --orbit 20,0 turns the eye 10 degrees about the look-at point."""
    cam = pt.initCamera()
    aspect = F(w) / F(h)
    eye, look, up = (np.ascontiguousarray(v, np.float32) for v in (cam.eye(), cam.lookat(), cam.up()))
    out = np.zeros(9, np.float32)
    if dx or dy:
        ev = np.array([0, 0, 0, 1, int(dx), int(dy)], np.int32)
        _native.host().pth_trackball_script(eye.ctypes.data, look.ctypes.data, up.ctypes.data, C.c_float(cam.fovY()), C.c_float(aspect),
                                            1, C.c_float(10.0), 1, int(w), int(h), ev.ctypes.data, 2, out.ctypes.data)
    else:
        out[:] = np.concatenate([eye, look, up])
    moved = pt.Camera(tuple(out[0:3]), tuple(out[3:6]), tuple(out[6:9]), cam.fovY(), aspect)
    U, V, W = moved.UVWFrame()
    return out[0:3].copy(), U, V, W


def set_camera(params, eye, U, V, W):
    f = lambda v: pt.Float3(float(v[0]), float(v[1]), float(v[2]))
    params.cameraEye, params.cameraU, params.cameraV, params.cameraW = f(eye), f(U), f(V), f(W)
    return params


def camera_of(params):
    return tuple(np.array(v.tuple(), np.float32) for v in (params.cameraEye, params.cameraU, params.cameraV, params.cameraW))


def tri_bsdf(obj):
    """bsdfType per triangle in the index-buffer order (what the context builds on the first pt_temporal_blend)."""
    kinds = np.array([m.bsdfType & 3 for m in obj.getMaterials()], np.uint8)
    return kinds[np.asarray(obj.getMaterialIndices(), np.uint32)]


# ---- the blend -----------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def blend(accum, albedo, nd, camera, n_samples, bsdf, cap, prev=None, dtype=np.float32):
    """The output of pt_temporal_blend and where history was taken.

    accum, albedo, nd: [h, w, 4] of the current view; camera: (eye, U, V, W); n_samples: N; bsdf: uint8 per triangle; cap: the
    history cap; prev: None (no history) or (camera', history, albedo', nd') with [h', w', 4] images.  Returns (out [h, w, 4], took
    [h, w] bool: the pixel blended history in, i.e. it is not the pass-through)."""
    accum, albedo, nd = (np.ascontiguousarray(a, np.float32) for a in (accum, albedo, nd))
    h, w = accum.shape[:2]
    F = np.dtype(dtype).type
    prim = albedo[..., 3].view(np.uint32)
    accum, nd = accum.astype(dtype), nd.astype(dtype)
    N = F(n_samples)
    cap = F(np.float32(cap))
    out = accum.copy()
    out[..., 3] = N
    took = np.zeros((h, w), bool)
    if prev is None:
        return out, took
    (eye_p, U_p, V_p, W_p), hist, alb_p, nd_p = prev
    hist, alb_p, nd_p = (np.ascontiguousarray(a, np.float32) for a in (hist, alb_p, nd_p))
    prim_p = alb_p[..., 3].view(np.uint32)
    hist, nd_p = hist.astype(dtype), nd_p.astype(dtype)
    hp, wp = hist.shape[:2]
    eye, U, V, W = (np.asarray(v, np.float32).astype(dtype) for v in camera)
    eye_p, U_p, V_p, W_p = (np.asarray(v, np.float32).astype(dtype) for v in (eye_p, U_p, V_p, W_p))
    bsdf = np.asarray(bsdf, np.uint8)
    valid = (nd[..., 3] >= 0) & (prim < bsdf.size)
    valid[valid] = bsdf[prim[valid]] == BSDF_DIFFUSE
    valid &= np.isfinite(accum[..., :3]).all(axis=-1)              # a non-finite accumulation pixel: the pass-through
    with np.errstate(all="ignore"):
        d = dr.pixel_rays(w, h, eye, U, V, W, dtype)[:, 3:6].reshape(h, w, 3)
        v = (eye[None, None, :] + nd[..., 3:4] * d) - eye_p[None, None, :]
        s = _dot(v, W_p) / _dot(W_p, W_p)
        valid &= s > 0
        du = _dot(v, U_p) / (s * _dot(U_p, U_p))
        dv = _dot(v, V_p) / (s * _dot(V_p, V_p))
        fx = (du + F(1.0)) * F(0.5) * F(wp) - F(0.5)
        fy = (dv + F(1.0)) * F(0.5) * F(hp) - F(0.5)
        valid &= (fx >= F(-1.0)) & (fx < F(wp)) & (fy >= F(-1.0)) & (fy < F(hp))
        fx, fy = np.where(valid, fx, F(0.0)), np.where(valid, fy, F(0.0))
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        a = np.zeros((h, w), dtype); r = np.zeros((h, w, 3), dtype); m = np.zeros((h, w), dtype)
        for ty in range(2):
            yq = y0 + ty
            wy = ay if ty else F(1.0) - ay
            for tx in range(2):
                xq = x0 + tx
                inside = valid & (yq >= 0) & (yq < hp) & (xq >= 0) & (xq < wp)
                yc, xc = np.clip(yq, 0, hp - 1), np.clip(xq, 0, wp - 1)
                ok = inside & (prim_p[yc, xc] == prim)
                nq = nd_p[yc, xc]
                ok &= (nq[..., 0] * nd[..., 0] + nq[..., 1] * nd[..., 1] + nq[..., 2] * nd[..., 2]) > F(0.0)
                wq = (ax if tx else F(1.0) - ax) * wy
                hq = hist[yc, xc]
                ok &= np.isfinite(hq).all(axis=-1)                 # a poisoned tap is not accepted
                a = np.where(ok, a + wq, a)
                r = np.where(ok[..., None], r + wq[..., None] * hq[..., :3], r)
                m = np.where(ok, m + wq * hq[..., 3], m)
        n = np.where(m < cap, m, cap)
        took = valid & (a > 0) & (n > 0)
        den = n + N
        rgb = (n[..., None] * (r / a[..., None]) + N * accum[..., :3]) / den[..., None]
        took &= np.isfinite(rgb).all(axis=-1)                      # a blend that left the number format: the pass-through
    out[took, :3] = rgb[took]
    out[took, 3] = den[took]
    return out, took
