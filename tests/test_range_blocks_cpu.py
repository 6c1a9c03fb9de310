"""The block search of the ranged decode (csrc/lz4ada_range_blocks.h, through
lz4ada_range_blocks_host) against a brute-force definition: a block is touched
when it shares a byte with the range clipped to the frame.  Every start[] of 0
to 5 blocks of the sizes {0, 1, 2, 255, 256, 257}, every off in 0 .. size + 2,
every len in {0, 1, 2, size, size + 1}: the interval selected is the span of
the touched blocks, so it never begins or ends with a block of size 0, and it
is empty exactly when the clipped length is 0."""
import itertools

import numpy as np
import pytest

import lz4ada

SIZES = (0, 1, 2, 255, 256, 257)


def brute(sizes, offs, lens):
    """(first, count, want) per range as int64 arrays, from the definition."""
    start = np.concatenate(([0], np.cumsum(sizes, dtype=np.int64))).astype(np.int64)
    size = int(start[-1])
    want = np.maximum(np.minimum(offs + lens, size) - offs, 0)
    first = np.zeros(len(offs), dtype=np.int64)
    count = np.zeros(len(offs), dtype=np.int64)
    if len(sizes):
        lo, hi = start[:-1][None, :], start[1:][None, :]
        touched = (hi > lo) & (lo < (offs + want)[:, None]) & (hi > offs[:, None]) & (want[:, None] > 0)
        some = touched.any(axis=1)
        f = touched.argmax(axis=1)
        last = touched.shape[1] - 1 - touched[:, ::-1].argmax(axis=1)
        first = np.where(some, f, 0)
        count = np.where(some, last - f + 1, 0)
        assert (some == (want > 0)).all()  # a non-empty clipped range lies in some non-empty block
    return start, first, count, want


@pytest.mark.parametrize("nb", range(6))
def test_every_small_frame(nb):
    ranges = 0
    for sizes in itertools.product(SIZES, repeat=nb):
        size = sum(sizes)
        lens = np.array([0, 1, 2, size, size + 1], dtype=np.int64)
        offs = np.repeat(np.arange(size + 3, dtype=np.int64), len(lens))
        lens = np.tile(lens, size + 3)
        start, first, count, want = brute(sizes, offs, lens)
        f, c, w = lz4ada.range_blocks_host_many(start, offs, lens)
        f, c, w = (np.frombuffer(x, dtype=np.int64) for x in (f, c, w))
        assert (w == want).all(), sizes
        assert ((c == 0) == (want == 0)).all(), sizes
        assert (f == first).all() and (c == count).all(), sizes
        sz = np.asarray(sizes + (1,), dtype=np.int64)  # a sentinel so that index 0 exists when nb == 0
        hit = c > 0
        assert (sz[f[hit]] > 0).all() and (sz[(f + c - 1)[hit]] > 0).all(), sizes
        ranges += len(offs)
    assert ranges > 0


def test_one_range_and_misuse():
    assert lz4ada.range_blocks_host([0, 300, 300, 301], 299, 2) == (0, 3, 2)
    assert lz4ada.range_blocks_host([0, 300, 300, 301], 300, 5) == (2, 1, 1)
    assert lz4ada.range_blocks_host([0, 300, 300, 301], 301, 5) == (0, 0, 0)
    assert lz4ada.range_blocks_host([0], 0, 5) == (0, 0, 0)
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.range_blocks_host([0, 5], -1, 2)
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.range_blocks_host([0, 5], 1, -2)
