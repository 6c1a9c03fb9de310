"""Records compressed against a shared dictionary on the GPU
(lz4ada_compress_frames_device_dict).  The yardstick is the
serial statement, byte for byte (lz4ada_compress_frame_dict_host, which
tests/test_compress_dict_host_cpu.py pins to the format and to three
decoders), so no decoder stands between the kernel and the check; then the
call's contract -- order, density, the guard region, the bound, the id -- and
the frames back through lz4ada_decode_frames_device_dict."""
import ctypes
import hashlib

import pytest
import torch

import lz4ada
from _compress_cases import KiB, LEN_ID5, pseudo_text, record
from _compress_dict_cases import (RECORDED, crafted, dict_frame_blocks, mixed_jobs, parse_block_dict,
                                  reads_dictionary, second_block_from_dictionary, text_dict)

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4 * KiB
ALL = dict(block_checksum=True, content_checksum=True, content_size=True)
MIXED = mixed_jobs()


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.delenv("LZ4ADA_BATCH_BYTES", raising=False)
    monkeypatch.delenv("LZ4ADA_BATCH_HASH_MAX", raising=False)


def to_device(data, at=0):
    """The bytes in device memory, `at` bytes into their allocation."""
    t = torch.empty(at + max(len(data), 1), dtype=torch.uint8, device="cuda")
    t[at:at + len(data)] = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8)[:len(data)]
    return t[at:at + len(data)]


def to_host(t):
    return t.cpu().numpy().tobytes()


def compress(data, spans, d, dict_id=None, slack=0, at=1, **kw):
    """One call into a canary-filled buffer of bound + slack + GUARD bytes with
    out_cap = bound + slack -> (the whole buffer's bytes, bytes written, jobs,
    bound).  d: the dictionary's bytes (None: no dictionary structure at all),
    laid `at` bytes into its allocation."""
    dt = to_device(d, at) if d is not None else None
    dd = (dt.data_ptr() if len(d) else None, len(d)) if d is not None else None
    bound = lz4ada.compress_frames_bound([n for _, n in spans], dict=dd, dict_id=dict_id, **kw)
    t = to_device(data)
    out = torch.full((bound + slack + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    n, jobs = lz4ada.compress_frames_device(t.data_ptr() if len(data) else None, len(data), spans, out.data_ptr(),
                                            bound + slack, torch.cuda.current_stream().cuda_stream, dict=dd,
                                            dict_id=dict_id, **kw)
    return to_host(out), n, jobs, bound


def check_call(raw, n, jobs, bound, plains, d, dict_id=None, slack=0, **kw):
    """Dense frames in job order that equal the serial statement's, and nothing
    written at or beyond the call's length."""
    at = 0
    for i, plain in enumerate(plains):
        want = lz4ada.compress_frame_host(plain, dict=d or b"", dict_id=dict_id, **kw)
        assert (jobs[i].out_off, jobs[i].out_len, jobs[i].status) == (at, len(want), 0), i
        assert raw[at:at + len(want)] == want, f"job {i} ({len(plain)} bytes) differs from the serial statement"
        assert jobs[i].stored_blocks == sum(b[0] for b in dict_frame_blocks(want)[4]), i
        at += len(want)
    assert n == at <= bound
    assert raw[n:] == bytes([CANARY]) * (bound + slack + GUARD - n), "bytes at or beyond *out_len were written"


@pytest.mark.parametrize("dl", [4, 65, 1000, 65535, 65536, 100000])
def test_mixed_jobs_equal_the_serial_statement(dl):
    data, spans, plains = MIXED
    d = text_dict(dl)
    raw, n, jobs, bound = compress(data, spans, d, slack=1000, at=dl % 4)
    check_call(raw, n, jobs, bound, plains, d, slack=1000)


def test_mixed_jobs_with_every_checksum():
    data, spans, plains = MIXED
    d = text_dict(65536)
    raw, n, jobs, bound = compress(data, spans, d, **ALL)
    check_call(raw, n, jobs, bound, plains, d, **ALL)
    raw2, n2, _, _ = compress(data, spans, d, at=2, **ALL)
    assert (raw2, n2) == (raw, n), "two calls differ"


def test_crafted_edges():
    """Every crafted record of the CPU file, one call per dictionary."""
    by_dict = {}
    for _, d, plain, _ in crafted():
        by_dict.setdefault(d, []).append(plain)
    d2, plain2 = second_block_from_dictionary()
    by_dict.setdefault(d2, []).extend([plain2, record(65537)])
    assert len(by_dict) >= 15
    for d, plains in by_dict.items():
        data, spans = b"", []
        for i, p in enumerate(plains):
            data += b"\x55" * (1 + i % 3)
            spans.append((len(data), len(p)))
            data += p
        raw, n, jobs, bound = compress(data, spans, d, at=3)
        check_call(raw, n, jobs, bound, plains, d)


def test_write_id():
    data, spans, plains = MIXED
    d = text_dict(65536)
    lens = [n for _, n in spans]
    for kw in ({}, ALL):
        raw, n, jobs, bound = compress(data, spans, d, dict_id=0xC0FFEE42, **kw)
        assert bound == lz4ada.compress_frames_bound(lens, **kw) + 4 * len(spans)
        check_call(raw, n, jobs, bound, plains, d, dict_id=0xC0FFEE42, **kw)
    # the id without a dictionary: the plain kernel's payloads behind the longer header
    raw, n, jobs, bound = compress(data, spans, b"", dict_id=7)
    check_call(raw, n, jobs, bound, plains, b"", dict_id=7)
    assert bound == lz4ada.compress_frames_bound(lens) + 4 * len(spans)


def test_capacity_one_below_the_bound():
    data, spans, _ = MIXED
    dt = to_device(text_dict(1000))
    dd = (dt.data_ptr(), dt.numel())
    bound = lz4ada.compress_frames_bound([n for _, n in spans], dict=dd, dict_id=3)
    t = to_device(data)
    out = torch.full((bound + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(lz4ada.TooLittleMemory) as e:
        lz4ada.compress_frames_device(t.data_ptr(), len(data), spans, out.data_ptr(), bound - 1,
                                      torch.cuda.current_stream().cuda_stream, dict=dd, dict_id=3)
    assert e.value.bound == bound
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "d_out was touched"


def test_no_dictionary_is_the_plain_call():
    data, spans, plains = MIXED
    want = compress(data, spans, None, **ALL)
    check_call(*want, plains, None, **ALL)
    raw, n, jobs, bound = compress(data, spans, b"", **ALL)  # a structure with dict_len 0 and no id
    assert (raw, n, bound) == want[:2] + want[3:]
    assert [(j.out_off, j.out_len, j.stored_blocks) for j in jobs[:len(spans)]] == \
           [(j.out_off, j.out_len, j.stored_blocks) for j in want[2][:len(spans)]]
    frames, where = lz4ada.compress_frames_tensor(to_device(data), spans, **ALL)  # the keywords' defaults
    assert to_host(frames) == raw[:n]


def test_misuse_launches_nothing():
    data = record(300)
    t, dt = to_device(data), to_device(text_dict(100))
    out = torch.full((1000 + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for cd in (lz4ada.CompressDict(dt.data_ptr(), -1, 0, 0), lz4ada.CompressDict(None, 100, 0, 0),
               lz4ada.CompressDict(dt.data_ptr(), 100, 0, 2), lz4ada.CompressDict(dt.data_ptr(), 100, 0, 0x80000001)):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.compress_frames_device(t.data_ptr(), 300, [(0, 300)], out.data_ptr(), 1000, stream, dict=cd)
    for bad in (dict(block=3), dict(block=8)):  # the options stay closed
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.compress_frames_device(t.data_ptr(), 300, [(0, 300)], out.data_ptr(), 1000, stream,
                                          dict=(dt.data_ptr(), 100), **bad)
    opt, n = lz4ada.CompressOptions(4, 8), ctypes.c_int64()
    cd = lz4ada.CompressDict(dt.data_ptr(), 100, 0, 0)
    st = lz4ada._lib.lz4ada_compress_frames_device_dict(t.data_ptr(), 300, lz4ada._compress_jobs([(0, 300)]), 1,
                                                        ctypes.byref(opt), ctypes.byref(cd), out.data_ptr(), 1000,
                                                        ctypes.byref(n), stream)
    assert st == 6  # LZ4ADA_ASSERTION_ERROR
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "d_out was touched"


def test_round_trip_on_the_device():
    """The frames through decode_frames_device with the dictionary, with the
    written id checked and without; another id is EXACT_PATH / DEVFRAME_DICT;
    without the dictionary a frame that reads it does not come back."""
    data, spans, plains = MIXED
    d = text_dict(65536)
    dt = to_device(d)
    frames, where = lz4ada.compress_frames_tensor(to_device(data), spans, dict=dt, dict_id=77, content_checksum=True)
    for check in (77, None):
        got, jobs = lz4ada.decode_frames_tensor(frames, where, dict=dt, dict_id=check)
        got = to_host(got)
        for i, plain in enumerate(plains):
            assert (jobs[i].status, jobs[i].consumed) == (0, where[i][1]), (i, jobs[i].reason)
            assert got[jobs[i].out_off:jobs[i].out_off + jobs[i].out_len] == plain, i
    _, jobs = lz4ada.decode_frames_tensor(frames, where, dict=dt, dict_id=78)
    assert all((jobs[i].status, jobs[i].reason) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_DICT)
               for i in range(len(plains)))
    # frames without an id, decoded without the dictionary
    k = next(i for i, p in enumerate(plains) if len(p) == 65535)
    frame = lz4ada.compress_frame_host(plains[k], dict=d)
    assert reads_dictionary(parse_block_dict(dict_frame_blocks(frame)[4][0][1], plains[k], d))
    frames, where = lz4ada.compress_frames_tensor(to_device(data), spans, dict=dt)
    assert to_host(frames[where[k][0]:where[k][0] + where[k][1]]) == frame
    got, jobs = lz4ada.decode_frames_tensor(frames, where)
    got = to_host(got)
    assert jobs[k].status != 0 or got[jobs[k].out_off:jobs[k].out_off + jobs[k].out_len] != plains[k]
    got, jobs = lz4ada.decode_frames_tensor(frames, where, dict=dt)
    assert jobs[k].status == 0 and to_host(got)[jobs[k].out_off:jobs[k].out_off + jobs[k].out_len] == plains[k]


def test_split_passes(monkeypatch):
    """LZ4ADA_BATCH_BYTES below the jobs' slots: more than three passes share
    the table of one call, the same bytes."""
    data, spans, plains = MIXED
    d = text_dict(65536)
    want = compress(data, spans, d, dict_id=5, **ALL)
    budget = 200 * KiB
    assert sum(-(-len(p) // 256) * 256 for p in plains) > 3 * budget
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(budget))
    raw, n, jobs, bound = compress(data, spans, d, dict_id=5, **ALL)
    assert (raw, n, bound) == want[:2] + want[3:]
    check_call(raw, n, jobs, bound, plains, d, dict_id=5, **ALL)


def test_id5_record():
    """One record of 300,000 bytes in blocks of 256 KiB: biased positions pass 2^18."""
    plain = record(LEN_ID5)
    d = text_dict(65536)
    raw, n, jobs, bound = compress(b"\x00" * 5 + plain, [(5, LEN_ID5)], d, block=256 * KiB)
    check_call(raw, n, jobs, bound, [plain], d, block=256 * KiB)
    assert jobs[0].stored_blocks == 0
    raw, n, jobs, bound = compress(plain[:100], [], d)
    assert (n, bound) == (0, 0) and raw == bytes([CANARY]) * GUARD
    raw, n, jobs, bound = compress(b"", [(0, 0), (0, 0)], d, dict_id=1, **ALL)
    check_call(raw, n, jobs, bound, [b"", b""], d, dict_id=1, **ALL)


def test_many_small_blocks():
    """2,048 records of 1 KiB, more blocks than resident waves, against the
    65,536-byte dictionary, compared with the serial statement by digest; the
    first 64 are the ratio test's and total what it recorded."""
    text = pseudo_text(65536 + 64 * KiB, 7)
    d, recs = text[:65536], text[65536:]
    spans = [(i * KiB, KiB) for i in range(64)]
    spans += [((i * 977) % (64 * KiB - KiB), KiB) for i in range(2048 - 64)]
    frames, where = lz4ada.compress_frames_tensor(to_device(recs), spans, dict=to_device(d))
    want, lens = hashlib.sha256(), []
    for o, n in spans:
        f = lz4ada.compress_frame_host(recs[o:o + n], dict=d)
        want.update(f)
        lens.append(len(f))
    assert [w[1] for w in where] == lens
    assert hashlib.sha256(to_host(frames)).hexdigest() == want.hexdigest()
    assert sum(lens[:64]) == RECORDED[1] + 64 * (7 + 4 + 4)
