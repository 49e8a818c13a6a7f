"""The owner formula of render_megakernel.hip k_keep_owned, as tests/group_ref.py restates it, against the oracle's work distribution
(oracle.sample_pixel, StaticWorkDistribution::getSamplePixel): for every world from 1 to 16 and every shape below, the pixels the oracle
gives rank r are exactly those with owner == r, and the ranks' sets partition the image.  On the CPU; tests/test_gpu_group.py's restore
test ties the kernel to the same formula."""
import numpy as np
import pytest

import group_ref as gr
from test_shapes_host import rank_pixels

SHAPES = [(1, 1), (7, 3), (8, 4), (9, 5), (17, 13), (100, 52), (328, 204)]
WORLDS = list(range(1, 17))


@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_owner_is_the_inverse_of_sample_pixel(oracle, w, h):
    for world in WORLDS:
        own = gr.owner_image(w, h, world)
        assert own.shape == (h, w) and own.min() >= 0 and own.max() < world
        cover = np.zeros((h, w), np.int64)
        for rank in range(world):
            xy = rank_pixels(oracle, world, w, h, rank)
            xy = xy[(xy[:, 0] < w) & (xy[:, 1] < h)]              # the slots of partial tiles fall outside the image
            given = np.zeros((h, w), bool)
            given[xy[:, 1], xy[:, 0]] = True
            assert int(given.sum()) == len(xy), (world, rank)     # no pixel twice within a rank
            assert np.array_equal(given, own == rank), (world, rank)
            cover += given
        assert np.all(cover == 1), world


def test_owner_in_words():
    """Tiles are 8 x 4 pixels; along a strip row the tiles go to ranks 0, 1, ..., and every strip row down the deal rotates by one."""
    assert gr.owner(0, 0, 3) == 0 and gr.owner(7, 3, 3) == 0 and gr.owner(8, 0, 3) == 1 and gr.owner(16, 3, 3) == 2 and gr.owner(24, 0, 3) == 0
    assert gr.owner(0, 4, 3) == 2 and gr.owner(8, 4, 3) == 0 and gr.owner(0, 8, 3) == 1 and gr.owner(0, 12, 3) == 0
    assert np.all(gr.owner_image(40, 20, 1) == 0)
    # two ranks: minus and plus agree modulo 2, so a sign slip in the rotation shows from three ranks on
    assert np.array_equal(gr.owner_image(40, 20, 2), ((np.mgrid[0:20, 0:40][1] >> 3) + (np.mgrid[0:20, 0:40][0] >> 2)) % 2)
    assert not np.array_equal(gr.owner_image(40, 20, 3), ((np.mgrid[0:20, 0:40][1] >> 3) + (np.mgrid[0:20, 0:40][0] >> 2)) % 3)
