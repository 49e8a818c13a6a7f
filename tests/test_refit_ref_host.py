"""tests/refit_ref.py without a GPU: the padded scene box it states contains every triangle (in float64), and equals values worked out by
hand on tiny scenes — the relative pad, the absolute pad that a far-away unreferenced vertex widens, and corners that are a + (b - a)
rather than b."""
import numpy as np

import refit_ref

F = np.float32


def _v(*xyz):
    return np.array([[x, y, z, 0.0] for x, y, z in xyz], F)


def test_box_contains_every_triangle():
    rng = np.random.default_rng(5)
    for scale, offset in ((1.0, 0.0), (1e-6, 0.0), (1e6, 0.0), (1.0, 1e7), (300.0, -40.0)):
        v = np.zeros((600, 4), F)
        v[:, :3] = (rng.uniform(-1, 1, size=(600, 3)) * scale + offset).astype(F)
        idx = rng.integers(0, 600, size=(400, 3)).astype(np.uint32)
        idx[:20, 1] = idx[:20, 0]                          # zero-area triangles
        lo, hi = refit_ref.scene_box(v, idx)
        tl, th = refit_ref.triangle_boxes(v, idx)
        p = v[idx.astype(np.int64), :3].astype(np.float64)      # [T, 3, 3]
        assert np.all(tl.astype(np.float64)[:, None, :] < p) and np.all(p < th.astype(np.float64)[:, None, :])
        assert np.array_equal(lo, tl.min(axis=0)) and np.array_equal(hi, th.max(axis=0))
        assert lo.dtype == F and hi.dtype == F


def test_unit_triangle():
    v = _v((0, 0, 0), (1, 0, 0), (0, 1, 0))
    assert refit_ref.pad_abs(v) == F(2.0 ** -19)
    lo, hi = refit_ref.scene_box(v, [[0, 1, 2]])
    p = F(1e-5)                                            # the relative pad beats 2^-19 = 1.9e-6
    assert lo.tolist() == [-p, -p, -p]
    assert hi.tolist() == [F(1) + p, F(1) + p, p]


def test_far_unreferenced_vertex_widens_the_pad():
    v = _v((0, 0, 0), (1, 0, 0), (0, 1, 0), (1e6, 0, 0))    # the fourth vertex belongs to no triangle
    pa = refit_ref.pad_abs(v)
    assert pa == F(15625.0 / 8192.0)                       # 1e6 * 2^-19, exact
    lo, hi = refit_ref.scene_box(v, [[0, 1, 2]])
    assert lo.tolist() == [-1.9073486328125] * 3
    assert hi.tolist() == [2.9073486328125, 2.9073486328125, 1.9073486328125]
    # without it, the unit triangle's box
    lo0, hi0 = refit_ref.scene_box(v[:3], [[0, 1, 2]])
    assert np.all(lo0 > lo) and np.all(hi0 < hi)
    # non-finite coordinates do not count
    w = v.copy()
    w[3, 0] = np.inf
    assert refit_ref.pad_abs(w) == F(2.0 ** -19)


def test_relative_pad_and_corners_from_the_record():
    # large coordinates: the relative pad 1e-5 * max(|lo|, |hi|) where it exceeds the absolute one
    v = _v((1000, -2000, 3), (1010, -2000, 3), (1000, -1990, 3))
    lo, hi = refit_ref.scene_box(v, [[0, 1, 2]])
    pa = F(2000.0) * F(2.0 ** -19)
    assert refit_ref.pad_abs(v) == pa
    assert lo[0] == F(1000) - F(1e-5) * F(1010) and hi[0] == F(1010) + F(1e-5) * F(1010)     # one pad per axis: max(|lo|, |hi|)
    assert lo[1] == F(-2000) - F(1e-5) * F(2000) and hi[1] == F(-1990) + F(1e-5) * F(2000)
    assert lo[2] == F(3) - pa and hi[2] == F(3) + pa                  # z: 3e-5 < 2000 * 2^-19, the absolute pad
    # a corner at a + (b - a), which fp32 rounds away from b
    a, b = F(30000.7), F(0.1)
    e1 = F(b - a)
    corner = F(a + e1)
    assert corner != b
    v = _v((30000.7, 0, 0), (0.1, 0, 0), (30000.7, 1, 0))
    lo, hi = refit_ref.scene_box(v, [[0, 1, 2]])
    assert lo[0] == corner - F(1e-5) * F(30000.7)                # not 0.1 - pad: the box is the record's triangle's

