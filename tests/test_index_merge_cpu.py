"""The merge rule of lz4ada_seek_index_concat on the host (no
GPU needed): lz4ada_index_merge_plan_host -- the validation, the five
exclusive prefixes and the part of every merged element -- against
numpy.cumsum and a linear scan, over part lists in which prefixes repeat
(parts without frames, parts with frames and no block); then every misuse of
the call itself and its empty cases, over empty indexes, which need no device."""
import ctypes

import numpy as np
import pytest

import lz4ada

ASSERTION, CONSTRAINT = 6, 7


def part_list(rng, nparts, empty_runs=True):
    """(jobs, blocks, checkpoints, input length, nominal slots) per part."""
    parts = []
    for p in range(nparts):
        roll = rng.integers(0, 10)
        if empty_runs and (roll < 3 or (nparts > 8 and (p < 3 or p >= nparts - 2 or nparts // 2 <= p < nparts // 2 + 3))):
            parts.append((0, 0, 0, int(rng.integers(0, 50)), 0))  # no job (runs at the front, middle and end)
            continue
        n = int(rng.integers(1, 9))
        if roll < 5:
            parts.append((n, 0, 0, 15 * n, 0))  # records of 0 bytes: frames without a block
            continue
        nb = int(rng.integers(1, 40))
        nck = int(rng.integers(0, nb)) if roll >= 7 else 0
        parts.append((n, nb, nck, int(rng.integers(20 * n, 1 << 20)), 256 * int(rng.integers(nb, 300 * nb))))
    return parts


def bases_for(rng, parts):
    bases, at = [], 0
    for p in parts:
        at += int(rng.integers(0, 3)) * int(rng.integers(0, 5000))  # touching, or a gap
        bases.append(at)
        at += p[3]
    return bases, at + int(rng.integers(0, 100))


def linear_part_of(prefix, i):
    """The definition: the one part p with prefix[p] <= i < prefix[p + 1]."""
    hits = [p for p in range(len(prefix) - 1) if prefix[p] <= i < prefix[p + 1]]
    assert len(hits) == 1
    return hits[0]


def check_plan(parts, bases, in_len):
    cols = np.array(parts, dtype=np.int64).reshape(len(parts), 5)
    n, nb, nck, slots = cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 4]
    want = [np.concatenate(([0], np.cumsum(c))).tolist() for c in (n, nb, nb + n, nck, slots)]
    queries = [(k, i) for k in range(4) for i in range(want[k][-1])]
    # nominal slots are bytes: their first, last and every part's boundary elements
    queries += [(4, i) for i in sorted({j for v in want[4] for j in (v - 1, v, v + 1) if 0 <= j < want[4][-1]})]
    prefix, part_of = lz4ada.index_merge_plan_host(parts, bases, in_len, queries)
    assert prefix == want
    for (k, i), p in zip(queries, part_of):
        assert p == linear_part_of(want[k], i), (k, i, p)
    return len(queries)


@pytest.mark.parametrize("nparts", [1, 2, 3, 7, 31, 300])
def test_prefixes_and_parts_against_cumsum_and_a_linear_scan(nparts):
    rng = np.random.default_rng(1000 + nparts)
    asked = 0
    for _ in range(2 if nparts == 300 else 8):
        parts = part_list(rng, nparts, empty_runs=nparts > 1)
        bases, in_len = bases_for(rng, parts)
        asked += check_plan(parts, bases, in_len)
    assert asked > 0


def test_repeated_prefixes_by_hand():
    """Empty parts at the front, in the middle and at the end; parts with
    frames and no block between parts with blocks."""
    e, z = (0, 0, 0, 7, 0), (2, 0, 0, 30, 0)
    a, b = (3, 5, 2, 1000, 5 * 65536), (1, 4, 3, 900, 4 * 65536)
    parts = [e, e, z, a, e, e, e, z, z, b, a, e, z, e, e]
    bases, at = [], 3
    for p in parts:
        bases.append(at)
        at += p[3]
    prefix, part_of = lz4ada.index_merge_plan_host(parts, bases, at, [(0, 0), (0, 1), (0, 2), (1, 0), (1, 4), (1, 5),
                                                                       (3, 0), (3, 2), (3, 4), (3, 5), (2, 0), (2, 2)])
    assert prefix[0][:5] == [0, 0, 0, 2, 5] and prefix[1][:5] == [0, 0, 0, 0, 5]
    assert part_of == [2, 2, 3, 3, 3, 9, 3, 9, 9, 10, 2, 3]
    check_plan(parts, bases, at)
    check_plan([], [], 0)
    check_plan([e, e], [0, 7], 14)
    check_plan([z], [5], 35)


def test_rule_misuse():
    a = (3, 5, 2, 1000, 5 * 65536)
    plan = lz4ada.index_merge_plan_host
    plan([a, a], [0, 1000], 2000)  # touching parts are fine
    plan([a, a], [10, 1500], 2500)  # and so are gaps
    for parts, bases, in_len in (([a, a], [0, 999], 2000), ([a, a], [1000, 0], 2000), ([a], [-1], 2000),
                                 ([a], [1], 1000), ([a, a], [0, 1000], 1999), ([a], [0], -1),
                                 ([(0, 0, 0, 10, 0), a], [5, 14], 2000), ([(-1, 0, 0, 10, 0)], [0], 10)):
        with pytest.raises(lz4ada.AssertionFailure):
            plan(parts, bases, in_len)
    with pytest.raises(lz4ada.AssertionFailure):
        plan([a], [0], 1000, [(1, 5)])  # a query past the total
    big = ((1 << 30), 1, 0, 16 << 30, 256)
    plan([big], [0], 16 << 30)
    with pytest.raises(lz4ada.ConstraintError):
        plan([big, big], [0, 16 << 30], 32 << 30)
    many = (1, (1 << 30) + 5, 0, 1 << 40, 256)
    with pytest.raises(lz4ada.ConstraintError):
        plan([many, many], [0, 1 << 40], 1 << 41)


# --------------------------------------------------- the call, over empty indexes

def empty_index(in_len):
    """An index over no job: the build makes no device call, and reads nothing
    at d_in (any address that is not NULL)."""
    return lz4ada.SeekIndex.build(4096, in_len, [])


def raw_concat(parts, bases, nparts, in_len, want_idx=True, null_parts=False, null_bases=False):
    arr = (ctypes.c_void_p * max(len(parts), 1))(*parts)
    base = (ctypes.c_int64 * max(len(bases), 1))(*bases)
    ptr = ctypes.c_void_p(0xDEAD)
    st = lz4ada._lib.lz4ada_seek_index_concat(None if null_parts else arr, None if null_bases else base, nparts,
                                              in_len, ctypes.byref(ptr) if want_idx else None, None)
    return st, ptr.value


def test_concat_misuse():
    with empty_index(100) as a, empty_index(50) as b:
        pa, pb = a._ptr, b._ptr
        assert raw_concat([pa, pb], [0, 100], 2, 150, want_idx=False)[0] == ASSERTION  # NULL idx
        for kw in (dict(null_parts=True), dict(null_bases=True)):
            assert raw_concat([pa, pb], [0, 100], 2, 150, **kw) == (ASSERTION, None)
        for parts, bases, nparts, in_len in (
                ([pa, None], [0, 100], 2, 150),  # a NULL part
                ([pa], [0], -1, 150),  # nparts < 0
                ([pa], [0], 1, -1),  # in_len < 0
                ([pa, pb], [-1, 100], 2, 150),  # a negative base
                ([pa, pb], [0, 99], 2, 150),  # inside the part before
                ([pb, pa], [100, 0], 2, 150),  # not rising
                ([pa, pb], [0, 100], 2, 149),  # the last part ends past in_len
                ([pa, pa], [0, 99], 2, 300)):  # the same part twice, overlapping itself
            assert raw_concat(parts, bases, nparts, in_len) == (ASSERTION, None), (bases, nparts, in_len)
        assert "in_len" in lz4ada._thread_error() or "part" in lz4ada._thread_error()
        # equal is fine, gaps are fine, and so is the same part twice over disjoint places
        for parts, bases, in_len in (([pa, pb], [0, 100], 150), ([pa, pb], [7, 200], 250), ([pa, pa], [0, 100], 200)):
            st, ptr = raw_concat(parts, bases, 2, in_len)
            assert st == 0 and ptr
            lz4ada._lib.lz4ada_seek_index_free(ptr)
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.SeekIndex.concat([a, b], [0, 99], 150)


def test_concat_of_empty_parts_is_an_empty_index():
    with empty_index(100) as a, empty_index(0) as b:
        for parts, bases in (([], []), ([a], [5]), ([a, b, a], [0, 100, 100])):
            with lz4ada.SeekIndex.concat(parts, bases, 300) as x:
                assert x.njobs == 0 and x.in_len == 300 and x.device_bytes == 0
                st = lz4ada.last_batch_stats()
                assert all(getattr(st, f) == 0 for f, _ in st._fields_)
                # nranges == 0: a call that worked and launches nothing (d_in is never read: any address)
                got, arr = lz4ada.decode_ranges_device(x, 4096, 300, [], None, 0)
                assert got == 0
                with pytest.raises(lz4ada.AssertionFailure):  # the old in_len
                    lz4ada.decode_ranges_device(x, 4096, 100, [], None, 0)
                arrays = lz4ada.seek_index_arrays_debug(x)
                assert arrays["nframes"] == 0 and arrays["desc"] == [] and arrays["first"] is None
                with lz4ada.SeekIndex.concat([x, a], [0, 300], 400) as y:  # a result is a part like any other
                    assert y.njobs == 0 and y.in_len == 400 and y.device_bytes == 0
    assert lz4ada._lib.lz4ada_abi_version() == 1
