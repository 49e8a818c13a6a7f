"""The case tables of tests/small_kernel_cases.py, held on the CPU to what their names claim: every camera's class by the share of
pixel centres whose ray hits the grown scene box (float64), every chunk_shift of launch_batch's rule reached by a sample shape, the
toggle table complete, the stack-depth scenes inside the reference limits of the small-scene path."""
import os

import numpy as np

import acgpathtracing_amd as pt
import small_kernel_cases as sk

SIZES = ((96, 64), (31, 33))


def test_the_scene_box_and_the_reference_camera_are_the_projects():
    v = np.array([[float(x) for x in line.split()[1:4]] for line in open(os.path.join(pt.SCENES, "cornell_box_diffuse.obj")) if line.startswith("v ")])
    assert tuple(v.min(axis=0)) == sk.SCENE_LO and tuple(v.max(axis=0)) == sk.SCENE_HI
    cam = pt.initCamera()
    assert (tuple(cam.eye()), tuple(cam.lookat()), tuple(cam.up()), cam.fovY()) == (sk.REF_EYE, sk.REF_LOOKAT, sk.REF_UP, sk.REF_FOVY)
    cam.setAspectRatio(np.float32(96) / np.float32(64))
    for got, want in zip(sk.camera("reference", 96, 64), (np.float32(cam.eye()),) + tuple(cam.UVWFrame())):
        assert np.allclose(got, want, rtol=1e-6, atol=1e-4), (got, want)
    lo, hi = sk.cull_box()
    ext = 559.2
    assert np.allclose(np.array(sk.SCENE_LO) - lo, ext / 1024 + 1e-6, rtol=1e-4) and np.allclose(hi - np.array(sk.SCENE_HI), ext / 1024 + 1e-6, rtol=1e-4)


def test_every_camera_is_of_its_class():
    assert set(sk.CAMERAS) == {"reference", "inside", "pulled_back", "off_axis", "grazing", "away"} and set(sk.PARTIAL_CAMERAS) < set(sk.CAMERAS)
    for w, h in SIZES:
        share = {}
        for name in sk.CAMERAS:
            cam = sk.camera(name, w, h)
            assert all(x.dtype == np.float32 and x.shape == (3,) for x in cam)
            r = sk.reach(cam, w, h)
            share[name] = r.mean()
            if name == "pulled_back":
                rows = r.sum(axis=1)
                assert (rows == 0).any() and (rows == w).any(), rows
                assert 0.0 < r.mean() < 0.25
            if name == "off_axis":       # cut by one vertical edge: one border column reaches, the other does not
                assert r[:, 0].any() != r[:, -1].any()
            if name == "grazing":
                cols = np.flatnonzero(r.any(axis=0))
                assert 1 <= len(cols) <= 2 and (cols.max() <= 1 or cols.min() >= w - 2), cols
        print(w, h, share)
        assert share["inside"] == 1.0 and share["away"] == 0.0
        for name in ("pulled_back", "off_axis", "grazing") + (("reference",) if (w, h) == (96, 64) else ()):
            assert 0.0 < share[name] < 1.0, (name, w, h, share[name])
    eye = sk.camera("inside", 96, 64)[0]
    assert (np.array(sk.SCENE_LO) < eye).all() and (eye < np.array(sk.SCENE_HI)).all()


def test_reach_is_the_slab_test():
    """the helper itself, on a view whose answer is known: straight at a unit box from 10 units away, four units of image plane"""
    cam = (np.float32([0.5, 0.5, -10.0]), np.float32([2.0, 0, 0]), np.float32([0, 2.0, 0]), np.float32([0, 0, 10.0]))
    r = sk.reach(cam, 40, 40, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0))
    # the front face spans a quarter of the image's width and height (grown by a thousandth): 10 x 10 pixel centres
    assert r.sum() == 100 and r[15:25, 15:25].all()


def test_sample_shapes_reach_every_shift():
    auto = {}
    for spp, chunks, frames in sk.SAMPLE_SHAPES:
        assert 1 <= spp <= 64 and frames >= 1 and chunks in (0, 1, 2, 4, 8, 16, 32)
        cs, ss = sk.shifts(spp, chunks, frames)
        assert (1 << cs) <= spp and ss >= cs and (1 << (ss - cs)) >= frames > (1 << (ss - cs)) // 2
        assert 96 * 64 << ss < 0x7FFFFFFF
        if chunks == 0:
            auto.setdefault(cs, []).append((spp, frames))
    assert sorted(auto) == [0, 1, 2, 3, 4], auto
    shapes = [(s, c, f) + sk.shifts(s, c, f) for s, c, f in sk.SAMPLE_SHAPES]
    assert any(s % 2 == 1 and s > 1 and c == 0 and cs == 0 for s, c, f, cs, ss in shapes)
    assert any(s == 1 for s, c, f, cs, ss in shapes)
    assert any(f << cs == 32 for s, c, f, cs, ss in shapes)
    assert any(cs == 5 for s, c, f, cs, ss in shapes)                # 32 runs: the last entry of the LCG skip table
    assert any(ss > cs for s, c, f, cs, ss in shapes)
    # the rule itself at the values launch_batch's comment names
    assert sk.shifts(16, 0, 1) == (2, 2) and sk.shifts(128, 0, 1) == (4, 4) and sk.shifts(128, 0, 1, pixels=1 << 20) == (3, 3)
    assert sk.shifts(16, 8, 3) == (3, 5) and sk.shifts(24, 0, 1) == (2, 2) and sk.shifts(12, 0, 2) == (1, 2)


def test_toggles_are_the_full_cross():
    assert len(sk.TOGGLES) == len(set(sk.TOGGLES)) == 12
    assert {(d, i) for d, i, _ in sk.TOGGLES} == {(False, False), (False, True), (True, False), (True, True)}
    assert {m for _, _, m in sk.TOGGLES} == {1, 4, 28}


def test_stack_depth_scenes():
    for v, idx, ids in (sk.lattice(28, 28), sk.tail(24, 700)):
        assert v.dtype == np.float32 and v.shape[1] == 4 and idx.dtype == np.uint32 and idx.shape == (len(ids), 3) and idx.max() == len(v) - 1
        assert 2 <= len(idx) <= 2049                                  # at most 2048 nodes
        assert (v[:, :3].min(axis=0) >= 0).all() and (v[:, :3].max(axis=0) <= np.array(sk.ROOM) + 1e-3).all()
    assert len(sk.lattice(28, 28)[1]) == 2 * 28 * 28
    v, idx, _ = sk.tail(24, 700)
    assert len(idx) == 10 + 24 + 700
    t = v[idx.ravel(), :3].reshape(-1, 3, 3)
    assert (t[-700:] == t[-701]).all()                                # coincident copies of the tail's last triangle
    size = np.ptp(t[10:34], axis=1).max(axis=1)
    assert (size[1:] <= size[:-1]).all() and size[-1] < size[0] / 100
    c = sk.tail_centres(24)
    assert (np.sort(c[:-1] / c[1:], axis=1) == [1.0, 1.0, 2.0]).all()     # one coordinate halves a step
    s = sk.spread(v)
    assert s.shape == v.shape and np.array_equal(s[:30], v[:30]) and not np.array_equal(s[30:], v[30:])
    ts = s[idx.ravel(), :3].reshape(-1, 3, 3)[10:]
    assert len(np.unique(ts.mean(axis=1).round(3), axis=0)) == len(ts)
