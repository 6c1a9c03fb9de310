"""Linked frames in the seek index (lz4ada_seek_index_build_opt, DESIGN.md
§16), the parts that need no device: the new entry's argument checks run before
any device call, and the chain rule on the host (lz4ada_range_chains_host, the
statement the kernels and the host's sweep share) equals its brute-force
definition over every frame of 1 to 9 blocks, every group size 1 to 4 and every
set of up to three touched intervals."""
import ctypes
import itertools

import pytest

import lz4ada

FAKE = 0x10000  # never dereferenced: the checks fail, or there is nothing to do


def stats():
    s = lz4ada.last_batch_stats()
    return (s.frames_batched, s.frames_single, s.passes, s.gpu_hashed, s.host_hashed)


def build_opt(args, opt, ptr):
    return lz4ada._lib.lz4ada_seek_index_build_opt(*args, ctypes.byref(opt) if opt is not None else None,
                                                   ctypes.byref(ptr) if ptr is not None else None, None)


def test_build_opt_misuse():
    jobs = (lz4ada.DeviceFrameJob * 1)()
    jobs[0].in_len = 10
    good = (FAKE, 1000, jobs, 0)
    bad_opts = [lz4ada.SeekOptions(2, 0, 0), lz4ada.SeekOptions(lz4ada.SEEK_LINKED | 4, 0, 0),
                lz4ada.SeekOptions(0x80000000, 0, 0), lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 1, 0),
                lz4ada.SeekOptions(0, 7, 0), lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 0, -1),
                lz4ada.SeekOptions(0, 0, -(1 << 62))]
    for opt in bad_opts:
        ptr = ctypes.c_void_p(FAKE)
        st = build_opt(good, opt, ptr)
        assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and ptr.value is None, (opt.flags, opt.reserved)
        assert lz4ada._thread_error().startswith("lz4ada_seek_index_build_opt: ")
        assert stats() == (0,) * 5
    # what the plain build calls misuse, with and without the flag
    for opt in (None, lz4ada.SeekOptions(0, 0, 0), lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 0, 65536)):
        for args in ((FAKE, 1000, None, 1), (FAKE, 1000, jobs, -1), (None, 1000, jobs, 1), (FAKE, -1, jobs, 1)):
            ptr = ctypes.c_void_p(FAKE)
            st = build_opt(args, opt, ptr)
            assert lz4ada._ERRORS[st] is lz4ada.AssertionFailure and ptr.value is None, args
        assert lz4ada._ERRORS[build_opt(good, opt, None)] is lz4ada.AssertionFailure  # NULL idx
        assert stats() == (0,) * 5
    for spans in ([(0, 1001)], [(0, 100), (50, 100)], [(-1, 10)]):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.SeekIndex.build(FAKE, 1000, spans, linked=True)
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.SeekIndex.build(FAKE, 1000, [], linked=True, checkpoint_bytes=-5)
    assert stats() == (0,) * 5


@pytest.mark.parametrize("opt", [None, lz4ada.SeekOptions(0, 0, 0), lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 0, 0),
                                 lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 0, 1 << 40)])
def test_an_empty_index_needs_no_device(opt):
    ptr = ctypes.c_void_p()
    assert build_opt((FAKE, 1000, None, 0), opt, ptr) == 0 and ptr.value
    idx = lz4ada.SeekIndex(ptr.value, None, 0, 1000)
    assert idx.device_bytes == 0 and lz4ada.seek_index_debug(idx) == []
    n, _ = lz4ada.decode_ranges_device(idx, FAKE, 1000, [], None, 0)
    assert n == 0 and stats() == (0,) * 5 and lz4ada.last_path() == 0
    idx.free()
    with lz4ada.SeekIndex.build(FAKE, 1000, [], linked=True, checkpoint_bytes=65536) as idx:
        assert idx._ptr and idx.device_bytes == 0


# ------------------------------------------------------------- the chain rule

def model(nb, K, touched):
    """The definition: a range touching [a, z] marks floor(a / K) * K .. z; a
    marked block b > 0 with b % K == 0 is a head; the chains are the maximal
    runs of marked blocks, cut in front of every head."""
    marked = set()
    for a, n in touched:
        if n:
            marked |= set(range(a // K * K, a + n))
    heads = {b for b in marked if b > 0 and b % K == 0}
    chains = []
    for b in sorted(marked):
        if b in heads or b - 1 not in marked:
            chains.append([b, 1])
        else:
            chains[-1][1] += 1
    return sorted(marked), sorted(heads), [tuple(c) for c in chains]


def intervals(nb):
    return [(a, z - a + 1) for a in range(nb) for z in range(a, nb)]


@pytest.mark.parametrize("nb", range(1, 10))
def test_chain_rule_is_the_brute_force_one(nb):
    ivs = intervals(nb)
    sets = [c for r in range(4) for c in itertools.combinations(ivs, r)]
    for K in range(1, 5):
        for touched in sets:
            got = lz4ada.range_chains_host(nb, K, list(touched))
            assert got == model(nb, K, touched), (nb, K, touched)
            # a chain never begins inside a group: its start is a group start
            assert all(f % K == 0 for f, _ in got[2]), (nb, K, touched)


def test_chain_rule_edges():
    assert lz4ada.range_chains_host(9, 2, [(5, 1)]) == ([4, 5], [4], [(4, 2)])
    assert lz4ada.range_chains_host(9, 2, [(1, 6)]) == ([0, 1, 2, 3, 4, 5, 6], [2, 4, 6], [(0, 2), (2, 2), (4, 2), (6, 1)])
    assert lz4ada.range_chains_host(9, 2, [(3, 0), (8, 1), (8, 1)]) == ([8], [8], [(8, 1)])
    assert lz4ada.range_chains_host(5, 16, [(4, 1)]) == ([0, 1, 2, 3, 4], [], [(0, 5)])
    # group 0: independent blocks, every touched block on its own
    assert lz4ada.range_chains_host(4, 0, [(1, 2)]) == ([1, 2], [], [(1, 1), (2, 1)])
    assert lz4ada.range_chains_host(0, 3, []) == ([], [], [])
    for args in ((3, 2, [(3, 1)]), (3, 2, [(-1, 1)]), (3, -1, [(0, 1)]), (-1, 1, [])):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.range_chains_host(*args)
