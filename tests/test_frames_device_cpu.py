"""The argument checks of the device-to-device many-frame calls run before any
device call, so they hold on a machine without a GPU: ranges outside the
input and ranges that share bytes are API misuse, an empty job array is a
call that worked."""
import ctypes

import pytest

import lz4ada

FAKE = 0x10000  # never dereferenced: the checks fail, or there is no job


def stats():
    s = lz4ada.last_batch_stats()
    return (s.frames_batched, s.frames_single, s.passes, s.gpu_hashed, s.host_hashed)


@pytest.mark.parametrize("spans", [
    [(0, 100), (50, 100)],      # share bytes, neither runs to the end
    [(50, 100), (0, 100)],      # the same, given in falling order
    [(0, 1001)],                # past the end
    [(1001, 0)],                # starts past the end
    [(-1, 10)],
    [(0, -1)],
])
def test_misuse_is_an_assertion_and_launches_nothing(spans):
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.frames_device_bound(FAKE, 1000, spans)
    with pytest.raises(lz4ada.AssertionFailure) as ei:
        lz4ada.decode_frames_device(FAKE, 1000, spans, FAKE, 1 << 20)
    assert ei.value.bound == 0 and ei.value.message.startswith("lz4ada_decode_frames_device: ")
    assert stats() == (0,) * 5


def test_null_arguments():
    jobs = (lz4ada.DeviceFrameJob * 1)()
    n = ctypes.c_int64(-1)
    lib = lz4ada._lib
    for args in ((FAKE, 1000, None, 1), (FAKE, 1000, jobs, -1), (None, 1000, jobs, 1), (FAKE, -1, jobs, 1)):
        st = lib.lz4ada_decode_frames_device(*args, FAKE, 1 << 20, ctypes.byref(n), None)
        assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and n.value == 0
        st = lib.lz4ada_frames_device_bound(*args, ctypes.byref(n), None)
        assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and n.value == 0


def test_no_jobs_is_a_call_that_worked():
    assert lz4ada.frames_device_bound(FAKE, 1000, [])[0] == 0
    n, _ = lz4ada.decode_frames_device(FAKE, 1000, [], None, 0)
    assert n == 0 and stats() == (0,) * 5
    assert lz4ada.last_path() == 0
    assert (lz4ada.DEVFRAME_BLOCK, lz4ada.DEVFRAME_SIZE, lz4ada.DEVFRAME_CHECKSUM) == (5, 6, 7)
    assert ctypes.sizeof(lz4ada.DeviceFrameJob) == 48
