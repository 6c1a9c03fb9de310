"""Dictionary frames in the seek index (lz4ada_seek_index_build_dict, DESIGN.md
§19), the parts that need no device: the gap count of an interval on the host
(lz4ada_range_gaps_host, the statement the ranged decode's kernels and its host
sweep share) equals its brute-force definition, the new build's argument checks
run before any device call, and the Python keywords build the structure the
C-ABI takes."""
import ctypes

import pytest

import lz4ada

FAKE = 0x10000  # never dereferenced: the checks fail, or there is nothing to do
NONE, LINKED, INDEP = 0, 1, 2
CHECKPOINT_GAP = 65792


def stats():
    s = lz4ada.last_batch_stats()
    return (s.frames_batched, s.frames_single, s.passes, s.gpu_hashed, s.host_hashed)


def build_dict(args, opt, dd, ptr):
    return lz4ada._lib.lz4ada_seek_index_build_dict(*args, ctypes.byref(opt) if opt is not None else None,
                                                    ctypes.byref(dd) if dd is not None else None,
                                                    ctypes.byref(ptr) if ptr is not None else None, None)


# ---------------------------------------------------------------- the gap count

def brute(nb, K, kind, lo, hi):
    """By the definitions: a head is a block b > 0 with b % K == 0 of a frame in
    groups of K; the dictionary precedes every block of an independent modern
    frame and block 0 of a linked one."""
    heads = sum(1 for b in range(lo, hi) if K and b > 0 and b % K == 0)
    gaps = sum(1 for b in range(lo, hi) if kind == INDEP or (kind == LINKED and b == 0))
    return heads, gaps


@pytest.mark.parametrize("nb", range(1, 10))
def test_gap_count_is_the_brute_force_one(nb):
    for K in range(0, 5):
        for kind in (NONE, LINKED, INDEP):
            for lo in range(nb + 1):
                for hi in range(lo, nb + 1):
                    assert lz4ada.range_gaps_host(nb, K, kind, lo, hi) == brute(nb, K, kind, lo, hi), (K, kind, lo, hi)


def test_gap_count_edges():
    assert lz4ada.range_gaps_host(9, 2, LINKED, 0, 9) == (4, 1)
    assert lz4ada.range_gaps_host(9, 2, LINKED, 1, 9) == (4, 0)
    assert lz4ada.range_gaps_host(9, 0, INDEP, 3, 7) == (0, 4)
    assert lz4ada.range_gaps_host(9, 0, NONE, 0, 9) == (0, 0)
    assert lz4ada.range_gaps_host(0, 3, LINKED, 0, 0) == (0, 0)
    # a chain from block 0 and its heads: no block takes both gaps
    for K in range(1, 5):
        for hi in range(1, 10):
            heads, gaps = lz4ada.range_gaps_host(9, K, LINKED, 0, hi)
            assert heads + gaps == 1 + (hi - 1) // K
    for args in ((-1, 0, 0, 0, 0), (5, -1, 0, 0, 1), (5, 1, 3, 0, 1), (5, 1, -1, 0, 1), (5, 1, 1, -1, 1),
                 (5, 1, 1, 3, 2), (5, 1, 1, 0, 6)):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.range_gaps_host(*args)
    heads = ctypes.c_int64()
    assert lz4ada._ERRORS[lz4ada._lib.lz4ada_range_gaps_host(5, 1, 1, 0, 5, ctypes.byref(heads), None)] \
        is lz4ada.AssertionFailure
    assert lz4ada._ERRORS[lz4ada._lib.lz4ada_range_gaps_host(5, 1, 1, 0, 5, None, ctypes.byref(heads))] \
        is lz4ada.AssertionFailure


# ---------------------------------------------------------------------- misuse

BAD_DICTS = [(FAKE, -1, 0, 0), (None, 5, 0, 0), (FAKE, 100, 0, 2), (FAKE, 100, 0, lz4ada.DICT_CHECK_ID | 0x80000000),
             (FAKE, -(1 << 62), 7, lz4ada.DICT_CHECK_ID)]


def test_build_dict_misuse():
    jobs = (lz4ada.DeviceFrameJob * 1)()
    jobs[0].in_len = 10
    # the dictionary's own misuse, with no job (nothing else to do) and with one
    # (the check comes before the device is looked for)
    for args in ((FAKE, 1000, jobs, 0), (FAKE, 1000, jobs, 1)):
        for opt in (None, lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 0, 65536)):
            for bad in BAD_DICTS:
                ptr = ctypes.c_void_p(FAKE)
                st = build_dict(args, opt, lz4ada.DeviceDict(*bad), ptr)
                assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and ptr.value is None, (args[3], bad)
                assert "dict" in lz4ada._thread_error()
                assert stats() == (0,) * 5
    # what lz4ada_seek_index_build_opt rejects, with a dictionary and without
    good = (FAKE, 1000, jobs, 0)
    bad_opts = [lz4ada.SeekOptions(2, 0, 0), lz4ada.SeekOptions(lz4ada.SEEK_LINKED | 4, 0, 0),
                lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 1, 0), lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 0, -1)]
    for dd in (None, lz4ada.DeviceDict(None, 0, 0, 0), lz4ada.DeviceDict(FAKE, 100, 0, 0)):
        for opt in bad_opts:
            ptr = ctypes.c_void_p(FAKE)
            st = build_dict(good, opt, dd, ptr)
            assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and ptr.value is None, (opt.flags, opt.reserved)
        for args in ((FAKE, 1000, None, 1), (FAKE, 1000, jobs, -1), (None, 1000, jobs, 1), (FAKE, -1, jobs, 1)):
            ptr = ctypes.c_void_p(FAKE)
            st = build_dict(args, None, dd, ptr)
            assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and ptr.value is None, args
        assert lz4ada._ERRORS[build_dict(good, None, dd, None)] is lz4ada.AssertionFailure  # NULL idx
        assert stats() == (0,) * 5
    for spans in ([(0, 1001)], [(0, 100), (50, 100)], [(-1, 10)]):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.SeekIndex.build(FAKE, 1000, spans, dict=FAKE, dict_len=100)
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.SeekIndex.build(FAKE, 1000, [], dict=FAKE, dict_len=-3)
    assert stats() == (0,) * 5


@pytest.mark.parametrize("dd", [None, (None, 0, 0, 0), (FAKE, 100, 0, 0), (FAKE, 100000, 9, lz4ada.DICT_CHECK_ID)])
def test_an_empty_index_needs_no_device(dd):
    ptr = ctypes.c_void_p()
    dd = None if dd is None else lz4ada.DeviceDict(*dd)
    assert build_dict((FAKE, 1000, None, 0), lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 0, 0), dd, ptr) == 0 and ptr.value
    idx = lz4ada.SeekIndex(ptr.value, None, 0, 1000)
    assert idx.device_bytes == 0 and lz4ada.seek_index_debug(idx) == []
    n, _ = lz4ada.decode_ranges_device(idx, FAKE, 1000, [], None, 0)
    assert n == 0 and stats() == (0,) * 5 and lz4ada.last_path() == 0
    idx.free()


# ------------------------------------------------------------------ the keywords

def test_python_keywords_build_the_structure(monkeypatch):
    seen = []

    def fake(d_in, in_len, jobs, njobs, opt, dd, ptr, stream):
        o, d = opt._obj, dd._obj
        seen.append((d_in, in_len, njobs, o.flags, o.reserved, o.checkpoint_bytes, d.d_dict, d.dict_len, d.dict_id,
                     d.flags, stream))
        return 0

    def other(*a):
        raise AssertionError("a build with a dictionary goes through lz4ada_seek_index_build_dict")

    monkeypatch.setattr(lz4ada._lib, "lz4ada_seek_index_build_dict", fake, raising=False)
    monkeypatch.setattr(lz4ada._lib, "lz4ada_seek_index_build_opt", other, raising=False)
    monkeypatch.setattr(lz4ada._lib, "lz4ada_seek_index_build", other, raising=False)
    monkeypatch.setattr(lz4ada._lib, "lz4ada_seek_index_free", lambda p: None, raising=False)
    spans = [(0, 10), (16, 20)]
    lz4ada.SeekIndex.build(FAKE, 1000, spans, 5, dict=0x20000, dict_len=300)
    lz4ada.SeekIndex.build(FAKE, 1000, spans, 5, linked=True, checkpoint_bytes=4096, dict=0x20000, dict_len=70000,
                           dict_id=0xC0FFEE42)
    lz4ada.SeekIndex.build(FAKE, 1000, spans, dict=0x20000, dict_len=0, dict_id=7)  # no bytes: no pointer
    lz4ada.SeekIndex.build(FAKE, 1000, spans, dict=lz4ada.DeviceDict(0x30000, 12, 3, lz4ada.DICT_CHECK_ID))
    assert seen == [
        (FAKE, 1000, 2, 0, 0, 0, 0x20000, 300, 0, 0, 5),
        (FAKE, 1000, 2, lz4ada.SEEK_LINKED, 0, 4096, 0x20000, 70000, 0xC0FFEE42, lz4ada.DICT_CHECK_ID, 5),
        (FAKE, 1000, 2, 0, 0, 0, None, 0, 7, lz4ada.DICT_CHECK_ID, 0),
        (FAKE, 1000, 2, 0, 0, 0, 0x30000, 12, 3, lz4ada.DICT_CHECK_ID, 0),
    ]
    d = lz4ada._seek_dict(None, 0, None)
    assert (d.d_dict, d.dict_len, d.dict_id, d.flags) == (None, 0, 0, 0)


def test_no_dictionary_keeps_the_old_entries(monkeypatch):
    called = []
    monkeypatch.setattr(lz4ada._lib, "lz4ada_seek_index_build_dict",
                        lambda *a: called.append("dict") or 0, raising=False)
    with lz4ada.SeekIndex.build(FAKE, 1000, []) as a, lz4ada.SeekIndex.build(FAKE, 1000, [], linked=True) as b:
        assert a._ptr and b._ptr
    assert called == []
