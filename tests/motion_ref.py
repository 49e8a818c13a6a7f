"""NumPy reference of pt_temporal_blend_motion (include/acgpt.h states the same definition), and the deformations its tests use.

It extends temporal_ref.blend by two steps and changes nothing else: the motion m of the hit point between the two vertex arrays
(Moller-Trumbore barycentrics on the current triangle, skipped where the triangle did not move) enters the reprojection, and the
history mean is clipped to mu +- gamma sigma of the current accumulation's 3 x 3 neighbourhood.  Everything is fp32 in the operation
order of csrc/temporal.hip, so that the GPU agrees with it as it does with temporal_ref.  Images are [h, w, 4] float32 with row 0 at
the bottom; vertex arrays are [n, 4] float32 (w ignored).

dtype=np.float64 evaluates the same formulas from the same fp32 inputs in double precision.  Invalid inputs follow include/acgpt.h:
temporal_ref's rules, and in the clip a neighbour whose rgb is not all finite is left out of the moments (k counts the rest) and a
sum c^2 / k - mu^2 that is not finite gives sigma = 0.  The clip's bounds are then never NaN, and its min and max are written np.fmin /
np.fmax, the device's fminf / fmaxf."""
import numpy as np

import denoise_ref as dr
import temporal_ref as tr

F = np.float32
SPHERE_MOVE = (-40.0, 0.0, 30.0)      # the calibration's move of the Cornell box's sphere: on the floor, clear of both blocks


# ---- deformations --------------------------------------------------------------------------------------------------------------
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
    return np.array(sorted(out), np.int64)


def translated(verts, which, d):
    """verts with the rows `which` moved by d, in fp32 (what acgpt_main --move adds)."""
    v = np.array(verts, np.float32).reshape(-1, 4)
    v[which, :3] += np.asarray(d, np.float32)
    return v


def rotated_about_y(verts, which, degrees):
    """verts with the rows `which` turned about the vertical axis through their centroid."""
    v = np.array(verts, np.float32).reshape(-1, 4)
    c = v[which, :3].astype(np.float64).mean(axis=0)
    a = np.radians(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    v[which, :3] = ((v[which, :3] - c) @ R.T + c).astype(np.float32)
    return v


def jittered(verts, seed, scale):
    v = np.array(verts, np.float32).reshape(-1, 4)
    v[:, :3] += np.random.default_rng(seed).normal(scale=scale, size=(v.shape[0], 3)).astype(np.float32)
    return v


# ---- the blend -----------------------------------------------------------------------------------------------------------------
_dot = tr._dot


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def clip_bounds(accum, gamma, dtype=np.float32):
    """(mu - gamma sigma, mu + gamma sigma) per pixel and channel, [h, w, 3]: the 3 x 3 neighbourhood of the accumulation, taps
    inside the image, dy outer, dx inner, sums left to right."""
    F = np.dtype(dtype).type
    c = np.ascontiguousarray(accum, np.float32)[..., :3].astype(dtype)
    h, w = c.shape[:2]
    s1 = np.zeros((h, w, 3), dtype); s2 = np.zeros((h, w, 3), dtype); k = np.zeros((h, w), dtype)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yq, xq = ys + dy, xs + dx
            inside = (yq >= 0) & (yq < h) & (xq >= 0) & (xq < w)
            cq = c[np.clip(yq, 0, h - 1), np.clip(xq, 0, w - 1)]
            inside = inside & np.isfinite(cq).all(axis=-1)         # a non-finite neighbour is left out
            with np.errstate(all="ignore"):
                s1 = np.where(inside[..., None], s1 + cq, s1)
                s2 = np.where(inside[..., None], s2 + cq * cq, s2)
            k = np.where(inside, k + F(1.0), k)
    with np.errstate(all="ignore"):
        mu = s1 / k[..., None]
        v = s2 / k[..., None] - mu * mu
        sigma = np.where(np.isfinite(v), np.sqrt(np.where(v > 0, v, F(0.0))), F(0.0))      # sqrtf(fmaxf(0, v)), 0 where v is not finite
        g = F(np.float32(gamma))
        return mu - g * sigma, mu + g * sigma


def blend(accum, albedo, nd, camera, n_samples, bsdf, cap, prev=None, idx=None, verts=None, prev_verts=None, gamma=0.0,
          return_history=False, dtype=np.float32):
    """The output of pt_temporal_blend_motion and where history was taken.

    The arguments of temporal_ref.blend, plus idx (the scene's index buffer), verts / prev_verts ([n, 4]: the positions the current
    and the previous view were traced with, both or neither) and gamma (the clip; 0: off).  Returns (out [h, w, 4], took [h, w]);
    with return_history also the history mean [h, w, 3] that entered the blend (after the clip; meaningful where took)."""
    assert (verts is None) == (prev_verts is None)
    accum, albedo, nd = (np.ascontiguousarray(a, np.float32) for a in (accum, albedo, nd))
    h, w = accum.shape[:2]
    F = np.dtype(dtype).type
    prim = albedo[..., 3].view(np.uint32)
    accum32 = accum
    accum, nd = accum.astype(dtype), nd.astype(dtype)
    N = F(n_samples)
    cap = F(np.float32(cap))
    out = accum.copy()
    out[..., 3] = N
    took = np.zeros((h, w), bool)
    hmean = np.zeros((h, w, 3), dtype)
    if prev is None:
        return (out, took, hmean) if return_history else (out, took)
    (eye_p, U_p, V_p, W_p), hist, alb_p, nd_p = prev
    hist, alb_p, nd_p = (np.ascontiguousarray(a, np.float32) for a in (hist, alb_p, nd_p))
    prim_p = alb_p[..., 3].view(np.uint32)
    hist, nd_p = hist.astype(dtype), nd_p.astype(dtype)
    hp, wp = hist.shape[:2]
    eye, U, V, W = (np.asarray(v, np.float32).astype(dtype) for v in camera)
    eye_p, U_p, V_p, W_p = (np.asarray(v, np.float32).astype(dtype) for v in (eye_p, U_p, V_p, W_p))
    bsdf = np.asarray(bsdf, np.uint8)
    valid = (nd[..., 3] >= 0) & (prim < bsdf.size)
    valid[valid] = bsdf[prim[valid]] == tr.BSDF_DIFFUSE
    valid &= np.isfinite(accum[..., :3]).all(axis=-1)              # a non-finite accumulation pixel: the pass-through
    with np.errstate(all="ignore"):
        d = dr.pixel_rays(w, h, eye, U, V, W, dtype)[:, 3:6].reshape(h, w, 3)
        P = eye[None, None, :] + nd[..., 3:4] * d
        if verts is not None:
            # motion: where the triangle moved, the hit point's barycentric displacement; elsewhere nothing is added
            vc = np.ascontiguousarray(verts, np.float32).reshape(-1, 4)[:, :3].astype(dtype)
            vq = np.ascontiguousarray(prev_verts, np.float32).reshape(-1, 4)[:, :3].astype(dtype)
            tri = np.asarray(idx, np.uint32).reshape(-1, 3)[np.where(valid, prim, 0)].astype(np.int64)
            v0, v1, v2 = vc[tri[..., 0]], vc[tri[..., 1]], vc[tri[..., 2]]
            D0, D1, D2 = vq[tri[..., 0]] - v0, vq[tri[..., 1]] - v1, vq[tri[..., 2]] - v2
            moved = valid & ((D0 != 0) | (D1 != 0) | (D2 != 0)).any(axis=-1)
            e1, e2 = v1 - v0, v2 - v0
            pv = _cross(d, e2)
            det = _dot(e1, pv)
            tv = eye[None, None, :] - v0
            b1 = _dot(tv, pv) / det
            qv = _cross(tv, e1)
            b2 = _dot(d, qv) / det
            m = (D0 + b1[..., None] * (D1 - D0)) + b2[..., None] * (D2 - D0)
            valid &= ~moved | np.isfinite(m).all(axis=-1)
            P = np.where(moved[..., None], P + m, P)
        v = P - eye_p[None, None, :]
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
        a = np.zeros((h, w), dtype); r = np.zeros((h, w, 3), dtype); mm = np.zeros((h, w), dtype)
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
                mm = np.where(ok, mm + wq * hq[..., 3], mm)
        n = np.where(mm < cap, mm, cap)
        took = valid & (a > 0) & (n > 0)
        hmean = r / a[..., None]
        if gamma > 0:
            lo, hi = clip_bounds(accum32, gamma, dtype)
            hmean = np.fmin(np.fmax(hmean, lo), hi)
        den = n + N
        rgb = (n[..., None] * hmean + N * accum[..., :3]) / den[..., None]
        took &= np.isfinite(rgb).all(axis=-1)                      # a blend that left the number format: the pass-through
    out[took, :3] = rgb[took]
    out[took, 3] = den[took]
    return (out, took, hmean) if return_history else (out, took)
