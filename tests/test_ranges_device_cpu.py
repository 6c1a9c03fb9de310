"""The argument checks of the seek index and the ranged decode run before any
device call, so they hold on a machine without a GPU: NULL arguments, a job
outside the index, negative or overflowing extents, a negative count and flags
in the build are API misuse; an empty index and an empty call work and launch
nothing."""
import ctypes

import pytest

import lz4ada

FAKE = 0x10000  # never dereferenced: the checks fail, or there is nothing to do
I64_MAX = (1 << 63) - 1


def stats():
    s = lz4ada.last_batch_stats()
    return (s.frames_batched, s.frames_single, s.passes, s.gpu_hashed, s.host_hashed)


@pytest.fixture()
def empty():
    with lz4ada.SeekIndex.build(FAKE, 1000, []) as idx:
        yield idx


def test_an_empty_index_needs_no_device(empty):
    assert empty._ptr and empty.njobs == 0 and empty.device_bytes == 0 and empty.in_len == 1000
    assert lz4ada.seek_index_debug(empty) == []
    n, ranges = lz4ada.decode_ranges_device(empty, FAKE, 1000, [], None, 0)
    assert n == 0 and stats() == (0,) * 5 and lz4ada.last_path() == 0
    assert ctypes.sizeof(lz4ada.FrameRange) == 48
    lz4ada._lib.lz4ada_seek_index_free(None)  # a no-op
    assert lz4ada._lib.lz4ada_seek_index_bytes(None) == 0
    empty.free()
    empty.free()  # the wrapper frees once
    assert empty._ptr is None


@pytest.mark.parametrize("ranges", [
    [(0, 0, 1)],             # no job 0 in an empty index
    [(-1, 0, 1)],
    [(0, -1, 1)],
    [(0, 0, -1)],
    [(0, I64_MAX, 1)],       # off + len overflows
    [(0, 2, I64_MAX - 1)],
])
def test_misuse_is_an_assertion_and_launches_nothing(empty, ranges):
    with pytest.raises(lz4ada.AssertionFailure) as ei:
        lz4ada.decode_ranges_device(empty, FAKE, 1000, ranges, FAKE, 1 << 20)
    assert ei.value.bound == 0 and ei.value.message.startswith("lz4ada_decode_ranges_device: ")
    assert stats() == (0,) * 5
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.ranges_select_debug(empty, ranges)


def test_another_in_len_is_an_assertion(empty):
    for in_len in (999, 1001, 0, -1):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.decode_ranges_device(empty, FAKE, in_len, [], FAKE, 0)
    assert stats() == (0,) * 5


def test_null_arguments(empty):
    lib = lz4ada._lib
    r = (lz4ada.FrameRange * 1)()
    n = ctypes.c_int64(-1)
    for args in ((None, FAKE, 1000, r, 0), (empty._ptr, None, 1000, r, 0), (empty._ptr, FAKE, 1000, None, 1),
                 (empty._ptr, FAKE, 1000, r, -1)):
        st = lib.lz4ada_decode_ranges_device(*args, FAKE, 1 << 20, ctypes.byref(n), None)
        assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and n.value == 0, args
    st = lib.lz4ada_decode_ranges_device(empty._ptr, FAKE, 1000, r, 0, FAKE, 0, None, None)
    assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure


def test_build_misuse():
    lib = lz4ada._lib
    jobs = (lz4ada.DeviceFrameJob * 1)()
    jobs[0].in_len = 10
    ptr = ctypes.c_void_p(FAKE)
    for flags in (lz4ada.FRAMES_LINKED, lz4ada.FRAMES_EXACT, 4):
        st = lib.lz4ada_seek_index_build(FAKE, 1000, jobs, 0, flags, ctypes.byref(ptr), None)
        assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and ptr.value is None
        assert lz4ada._thread_error() == "lz4ada_seek_index_build: flags must be 0"
    for args in ((FAKE, 1000, None, 1), (FAKE, 1000, jobs, -1), (None, 1000, jobs, 1), (FAKE, -1, jobs, 1)):
        ptr = ctypes.c_void_p(FAKE)
        st = lib.lz4ada_seek_index_build(*args, 0, ctypes.byref(ptr), None)
        assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and ptr.value is None, args
    st = lib.lz4ada_seek_index_build(FAKE, 1000, jobs, 0, 0, None, None)
    assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure
    for spans in ([(0, 1001)], [(0, 100), (50, 100)], [(-1, 10)]):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.SeekIndex.build(FAKE, 1000, spans)
    assert stats() == (0,) * 5
