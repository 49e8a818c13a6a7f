"""The sweep, capsule, box and triangle casts and pt_query_poses_cast against tests/golden/cast_walk.npz, bit for bit: every record,
every any-hit byte and every visit pair of every mode of the pt_debug_*_visits hooks, on the four scenes and both node formats of
tests/cast_walk_cases.py.  The four families share csrc/cast_walk.h; the file was recorded from the commit before they did
(tests/golden/make_cast_walk_golden.py).  The visit counts are part of it: the boxes only prune, so a change to what the shared walk
admits leaves the records alone and moves the counts."""
import numpy as np
import pytest

import cast_walk_cases as cw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(cw.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def got():
    return cw.run_all()


def test_every_case_was_run_and_every_array_of_the_file_is_used(got, golden):
    assert sorted(got) == sorted(cw.all_keys())
    assert set(cw.pack(got)) == set(golden) - {"recorded_from"}


@pytest.mark.parametrize("scene", list(cw.SCENES))
def test_bits_equal_the_recorded_ones(got, golden, scene):
    keys = [k for k in cw.all_keys() if k.split("/")[1] == scene or (scene == "box" and k.startswith("poses_cast/"))]
    assert len(keys) >= 2 * (4 * 2 + 2 * 2 * 1 + 2 * 2 * 2)          # per format: four families' records and bytes, and a pair per hook mode
    for key in keys:
        want = cw.expected(golden, key)
        assert got[key].dtype == want.dtype and got[key].shape == want.shape, key
        bad = np.flatnonzero((got[key].reshape(want.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))
        assert bad.size == 0, (key, bad[:8], got[key][bad[:2]], want[bad[:2]])

