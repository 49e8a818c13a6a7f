"""NumPy statement of the padded scene box that pt_set_scene and pt_update_vertices(PT_UPDATE_REFIT) report in pt_get_bvh_info.scene_lo /
scene_hi (lbvh_build.hip record_aabb and build_impl; refit.hip rf_record_aabb and refit_lbvh), in fp32, operation for operation:

  pad_abs   max(1, largest finite |coordinate| over EVERY vertex, referenced or not) * 2^-19
  record    a, e1 = b - a, e2 = c - a; the box's corners are a, a + e1, a + e2 (the triangle the intersection test works on)
  pad       per axis max(1e-5 * max(1, |lo|, |hi|), pad_abs); the triangle's box is [lo - pad, hi + pad]
  scene     min / max of the triangles' boxes

Every step is a single correctly rounded fp32 operation (or a min / max), so the device's bits follow."""
import numpy as np

F = np.float32


def pad_abs(verts):
    """2^-19 of the largest finite |coordinate| of every vertex (xyz; at least 1 before the scaling)."""
    xyz = np.abs(np.asarray(verts, F).reshape(len(verts), -1)[:, :3]).reshape(-1)
    xyz = xyz[np.isfinite(xyz)]
    m = max(F(1.0), xyz.max()) if xyz.size else F(1.0)
    return F(m) * F(1.0 / 524288.0)


def triangle_boxes(verts, idx, pad=None):
    """(lo[T, 3], hi[T, 3]) fp32: each triangle's padded box from its record."""
    v = np.asarray(verts, F).reshape(len(verts), -1)[:, :3]
    i = np.asarray(idx, np.int64).reshape(-1, 3)
    pa = pad_abs(verts) if pad is None else F(pad)
    a, b, c = v[i[:, 0]], v[i[:, 1]], v[i[:, 2]]
    e1, e2 = (b - a).astype(F), (c - a).astype(F)
    pb, pc = (a + e1).astype(F), (a + e2).astype(F)
    lo = np.minimum(a, np.minimum(pb, pc))
    hi = np.maximum(a, np.maximum(pb, pc))
    rel = F(1e-5) * np.maximum(F(1.0), np.maximum(np.abs(lo), np.abs(hi)))
    pad_k = np.maximum(rel.astype(F), pa)
    return (lo - pad_k).astype(F), (hi + pad_k).astype(F)


def scene_box(verts, idx):
    """(scene_lo[3], scene_hi[3]) fp32, what pt_get_bvh_info reports for these vertices."""
    lo, hi = triangle_boxes(verts, idx)
    return lo.min(axis=0), hi.max(axis=0)
