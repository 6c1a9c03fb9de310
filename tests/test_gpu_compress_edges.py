"""The compressor's in-block edge cases on the GPU: the records
of tests/_compress_edge_cases.py, which tests/test_compress_edges_cpu.py proves
to sit where they claim, through k_compress_blocks, k_compress_blocks_dict and
k_compress_blocks_linked -- the three builds of lz4ada_compress_block.inc -- and
the scan and emit kernels.  As in tests/test_gpu_compress.py the yardstick is
the serial statement, byte for byte, with that file's contract around it: dense
frames in job order, out_off / out_len / status, stored_blocks, the guard region
behind *out_len.  Every test is one or two calls of many jobs."""
import pytest
import torch

import lz4ada
from _compress_cases import KiB
from _compress_dict_cases import dict_frame_blocks
from _compress_edge_cases import (EDGE_DICT, alignment_ladder, continuation_cases, far_repeats, in_block_cases,
                                  laid_out, near_bound, small_alphabets)

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4 * KiB
ALL = dict(block_checksum=True, content_checksum=True, content_size=True)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.delenv("LZ4ADA_BATCH_BYTES", raising=False)
    monkeypatch.delenv("LZ4ADA_BATCH_HASH_MAX", raising=False)
    monkeypatch.delenv("LZ4ADA_BATCH_LINKED_MAX", raising=False)


def to_device(data, at=0):
    """The bytes in device memory, `at` bytes into their allocation."""
    t = torch.empty(at + max(len(data), 1), dtype=torch.uint8, device="cuda")
    t[at:at + len(data)] = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8)[:len(data)]
    return t[at:at + len(data)]


def to_host(t):
    return t.cpu().numpy().tobytes()


_WANT = {}


def statement(plain, d, linked, kw):
    """The serial statement's frame, computed once per record and options."""
    key = (plain, d, linked, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = lz4ada.compress_frame_host(plain, dict=d or b"", linked=linked, **kw)
    return _WANT[key]


def jobs_of(cases, pad=3, shuffle=True):
    """(name, record) laid out at odd places of one input, the jobs in an order
    of their own -> (input, spans, names in job order, plaintexts in job order)."""
    data, spans, order = laid_out([rec for _, rec in cases], pad, shuffle)
    return data, spans, [cases[i][0] for i in order], [cases[i][1] for i in order]


def compress(data, spans, d=None, linked=False, **kw):
    """One call into a canary-filled buffer of bound + GUARD bytes with out_cap
    = bound -> (the whole buffer's bytes, bytes written, jobs, bound).  d: the
    dictionary's bytes, laid one byte into its allocation."""
    dt = to_device(d, 1) if d is not None else None
    dd = (dt.data_ptr(), len(d)) if d is not None else None
    bound = lz4ada.compress_frames_bound([n for _, n in spans], dict=dd, **kw)
    t = to_device(data)
    out = torch.full((bound + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    n, jobs = lz4ada.compress_frames_device(t.data_ptr(), len(data), spans, out.data_ptr(), bound,
                                            torch.cuda.current_stream().cuda_stream, dict=dd, linked=linked, **kw)
    return to_host(out), n, jobs, bound


def check_call(raw, n, jobs, bound, names, plains, d=None, linked=False, **kw):
    """tests/test_gpu_compress.py's check_call, the failing record named with
    the first byte at which it differs from the serial statement."""
    at = 0
    for i, (name, plain) in enumerate(zip(names, plains)):
        want = statement(plain, d, linked, kw)
        assert (jobs[i].out_off, jobs[i].out_len, jobs[i].status) == (at, len(want), 0), name
        got = raw[at:at + len(want)]
        if got != want:
            k = next(j for j in range(len(want)) if got[j] != want[j])
            pytest.fail(f"{name} ({len(plain)} bytes) differs from the serial statement at byte {k} of its frame: "
                        f"{got[k:k + 8].hex()} for {want[k:k + 8].hex()}")
        assert jobs[i].stored_blocks == sum(b[0] for b in dict_frame_blocks(want)[4]), name
        at += len(want)
    assert n == at <= bound
    assert raw[n:] == bytes([CANARY]) * (bound + GUARD - n), "bytes at or beyond *out_len were written"


def run(cases, d=None, linked=False, pad=3, shuffle=True, **kw):
    data, spans, names, plains = jobs_of(cases, pad, shuffle)
    raw, n, jobs, bound = compress(data, spans, d, linked, **kw)
    check_call(raw, n, jobs, bound, names, plains, d, linked, **kw)
    return names, jobs


def check_near_bound(names, jobs):
    """stored_blocks case by case, from the statement's block function: 1
    exactly where the block does not come out shorter than it went in."""
    stored = {name: len(lz4ada.compress_block_host(rec, len(rec) + 1024)) > len(rec) - 1
              for name, rec, _ in near_bound()}
    assert 6 <= sum(stored.values()) <= len(stored) - 6
    seen = 0
    for i, name in enumerate(names):
        if name in stored:
            assert jobs[i].stored_blocks == int(stored[name]), name
            seen += 1
    assert seen == len(stored)


def test_in_block_edges_plain():
    """k_compress_blocks over the extension grid, the length edges, the blocks
    around the stored threshold, the window tails and the far repeats cut into
    blocks of 64 KiB; without a flag and with all three."""
    cases = in_block_cases()
    assert len(cases) > 500
    for kw in (dict(), ALL):
        names, jobs = run(cases, **kw)
        check_near_bound(names, jobs)


def test_far_repeats_id5():
    """The offset limit past position 2^17 of one 256 KiB block."""
    run([(name, rec) for name, rec, _ in far_repeats()], block=256 * KiB)


def test_small_alphabets():
    cases = [(name, rec) for name, rec, _ in small_alphabets()]
    run(cases)


def test_alignment_ladder():
    """Every destination alignment against every payload length mod 4, stored
    and compressed, and every source alignment of a stored block."""
    cases = [(name, rec) for name, rec, _ in alignment_ladder()]
    run(cases, pad=4, shuffle=False)
    run(cases, pad=4, shuffle=False, block_checksum=True)


def test_edges_with_a_dictionary():
    """k_compress_blocks_dict's copy of the body: the same records against a
    dictionary that seeds the table and matches nothing they plan."""
    names, jobs = run(in_block_cases(), EDGE_DICT)
    check_near_bound(names, jobs)  # the planned sequences, and so the sizes, are unchanged under it


def test_edges_in_a_continuation_block():
    """k_compress_blocks_linked with `cont` set: each record is 64 KiB of noise
    and an edge case as block 1, every table entry seeded from block 0."""
    cases = [(name, rec) for name, rec, _ in continuation_cases()]
    names, jobs = run(cases, linked=True)
    # block 0 is stored; block 1 is compressed, but for the one case a byte over
    assert [jobs[i].stored_blocks for i in range(len(names))] == [2 if name == "ext_end_ml7" else 1 for name in names]


def test_edges_decode_on_the_device():
    """The decoder's kernels on what the edge cases produce: match lengths and
    literal runs at the extension thresholds, stored blocks beside compressed
    ones, and the small alphabets' offsets of 1..8."""
    cases = in_block_cases() + [(name, rec) for name, rec, _ in small_alphabets()]
    data, spans, names, plains = jobs_of(cases)
    frames, where = lz4ada.compress_frames_tensor(to_device(data), spans)
    raw = to_host(frames)
    for name, plain, (off, n) in zip(names, plains, where):
        assert raw[off:off + n] == statement(plain, None, False, {}), name
    got, jobs = lz4ada.decode_frames_tensor(frames, where)
    got = to_host(got)
    for i, (name, plain) in enumerate(zip(names, plains)):
        assert (jobs[i].status, jobs[i].consumed) == (0, where[i][1]), (name, jobs[i].reason)
        assert got[jobs[i].out_off:jobs[i].out_off + jobs[i].out_len] == plain, name
