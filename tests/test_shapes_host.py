"""The image shapes and partitions that tests/test_gpu_shapes.py renders, and the oracle's work distribution at each of them: for every
(shape, world), oracle.sample_pixel over the num_samples slots of every rank covers each pixel exactly once, and the slots that land
outside the image (the padding of the last partial tile strips) number exactly world * num_samples - w * h.  The GPU file compares
each rank's pixel set with this fixture; here it is pinned on its own, on the CPU."""
import numpy as np
import pytest

# tiny and partial tiles, extreme extents, the pixel-class limit (capi.hip launch_batch: row spans for height <= 32767)
TINY_SHAPES = [(1, 1), (2, 1), (1, 2), (3, 5), (7, 3), (8, 4), (9, 5), (17, 13), (31, 33)]
EXTREME_SHAPES = [(65535, 1), (1, 65535), (65535, 3), (3, 65535)]
CLASS_LIMIT_SHAPES = [(2, 32767), (2, 32768), (2, 32769)]     # and the first image with a row y = 32768 (bit 15 of y set)
EXACT_SHAPES = TINY_SHAPES + EXTREME_SHAPES + CLASS_LIMIT_SHAPES
# (w, h, world) on both sides of 2^20 pixels per rank, where the automatic chunk rule switches from 16 runs to 8
AUTO_CHUNK_SHAPES = [(1024, 1023, 1), (1024, 1024, 1), (1025, 1024, 1), (2048, 1024, 2)]
PARTITION_WORLDS = [2, 3, 4, 5, 8]
PARTITION_SHAPES = [(5, 3), (9, 5), (17, 13), (100, 52)]


def expected_chunks(w, h, world, spp):
    """The automatic sample-chunk count (capi.hip launch_batch): 16 runs below 2^20 pixels per rank, 8 from there, fewer while spp is
    not a multiple of the count or a run would keep fewer than 4 samples."""
    want = 4 if (w * h) // world < (1 << 20) else 3
    while want > 0 and (spp % (1 << want) != 0 or (spp >> want) < 4):
        want -= 1
    return 1 << want


def rank_pixels(oracle, world, w, h, rank):
    """[n, 2] (x, y) of the slots of `rank`, in slot order, padding included."""
    n = oracle.num_samples(world, w, h)
    return np.array([oracle.sample_pixel(world, w, rank, si) for si in range(n)], np.int64).reshape(-1, 2)


def _strips(world, w, h):
    cols = -(-w // (8 * world))
    rows = -(-h // 4)
    return rows * cols * 32


CASES = sorted({(1, w, h) for w, h in EXACT_SHAPES} | {(world, w, h) for world in PARTITION_WORLDS for w, h in PARTITION_SHAPES}
               | {(world, w, h) for w, h, world in AUTO_CHUNK_SHAPES})


@pytest.mark.parametrize("world,w,h", CASES)
def test_sample_pixel_covers_every_pixel_once(oracle, world, w, h):
    n = oracle.num_samples(world, w, h)
    assert n == _strips(world, w, h)           # whole 8 * world x 4 tile strips, rounded up on both axes
    count = np.zeros((h, w), np.int64)
    pad = 0
    for rank in range(world):
        xy = rank_pixels(oracle, world, w, h, rank)
        assert (xy >= 0).all()
        inside = (xy[:, 0] < w) & (xy[:, 1] < h)
        np.add.at(count, (xy[inside, 1], xy[inside, 0]), 1)
        pad += int((~inside).sum())
    assert np.all(count == 1)
    assert pad == world * n - w * h


def test_chunk_rule():
    assert [expected_chunks(17, 13, 1, s) for s in (1, 2, 3, 4, 5, 7, 8, 12, 16, 64, 96)] == [1, 1, 1, 1, 1, 1, 2, 2, 4, 16, 16]
    assert expected_chunks(1024, 1023, 1, 64) == 16 and expected_chunks(1024, 1024, 1, 64) == 8
    assert expected_chunks(1025, 1024, 1, 64) == 8 and expected_chunks(2048, 1024, 2, 64) == 8
    assert expected_chunks(2047, 1024, 2, 64) == 16
    # at 32 spp the runs are capped at 8 by the 4-sample floor on both sides of the switch
    assert expected_chunks(1024, 1024, 1, 32) == 8 and expected_chunks(1024, 1023, 1, 32) == 8
