"""Records compressed into frames of linked blocks on the GPU
(lz4ada_compress_frames_device_linked).  The yardstick is the
serial statement, byte for byte (lz4ada_compress_frame_linked_host, which
tests/test_compress_linked_host_cpu.py pins to the format and to two decoders),
so no decoder stands between the kernel and the check; then the call's contract
-- order, density, the guard region, the bound, misuse -- and the frames back
through the device's decoders of linked frames: decode_frames_device(linked=True),
its dictionary form and a linked SeekIndex.  Never through the oracle or a
reference-twin path: a linked frame may carry the offsets of quirk D1."""
import ctypes
import hashlib

import pytest
import torch

import lz4ada
from _compress_cases import KiB, id4_records, pseudo_text, record
from _compress_dict_cases import dict_frame_blocks, text_dict
from _compress_linked_cases import B, LENGTHS, dict_only_record, mixed_jobs, parse_block_linked

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4 * KiB
ALL = dict(block_checksum=True, content_checksum=True, content_size=True)
MIXED = mixed_jobs()
D64K = text_dict(65536)


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


@pytest.fixture(scope="module")
def mixed_on_device():
    return to_device(MIXED[0])


_WANT = {}


def statement(plain, d, dict_id, linked, kw):
    """The serial statement's frame, computed once per record and options."""
    key = (plain, d, dict_id, linked, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = lz4ada.compress_frame_host(plain, dict=d or b"", dict_id=dict_id, linked=linked, **kw)
    return _WANT[key]


def compress(data, spans, d=None, dict_id=None, slack=0, at=1, linked=True, t=None, **kw):
    """One call into a canary-filled buffer of bound + slack + GUARD bytes with
    out_cap = bound + slack -> (the whole buffer's bytes, bytes written, jobs,
    bound).  d: the dictionary's bytes (None: no dictionary structure at all),
    laid `at` bytes into its allocation."""
    dt = to_device(d, at) if d is not None else None
    dd = (dt.data_ptr() if len(d) else None, len(d)) if d is not None else None
    bound = lz4ada.compress_frames_bound([n for _, n in spans], dict=dd, dict_id=dict_id, **kw)
    t = to_device(data) if t is None else t
    out = torch.full((bound + slack + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    n, jobs = lz4ada.compress_frames_device(t.data_ptr() if len(data) else None, len(data), spans, out.data_ptr(),
                                            bound + slack, torch.cuda.current_stream().cuda_stream, dict=dd,
                                            dict_id=dict_id, linked=linked, **kw)
    return to_host(out), n, jobs, bound


def check_call(raw, n, jobs, bound, plains, d=None, dict_id=None, slack=0, linked=True, **kw):
    """Dense frames in job order that equal the serial statement's, and nothing
    written at or beyond the call's length."""
    at = 0
    for i, plain in enumerate(plains):
        want = statement(plain, d, dict_id, linked, kw)
        assert (jobs[i].out_off, jobs[i].out_len, jobs[i].status) == (at, len(want), 0), i
        assert raw[at:at + len(want)] == want, f"job {i} ({len(plain)} bytes) differs from the serial statement"
        assert jobs[i].stored_blocks == sum(b[0] for b in dict_frame_blocks(want)[4]), i
        at += len(want)
    assert n == at <= bound
    assert raw[n:] == bytes([CANARY]) * (bound + slack + GUARD - n), "bytes at or beyond *out_len were written"


# ------------------------------------------------- device equals the statement

def test_mixed_jobs_equal_the_serial_statement(mixed_on_device):
    """Mixed, overlapping, out-of-order jobs with the crafted records among
    them, no dictionary: the guard region behind *out_len stays canary."""
    data, spans, plains = MIXED
    assert sum(len(p) > B for p in plains) >= 50 and sum(len(p) <= B for p in plains) >= 10
    raw, n, jobs, bound = compress(data, spans, slack=1000, t=mixed_on_device)
    check_call(raw, n, jobs, bound, plains, slack=1000)


@pytest.mark.parametrize("dl", [4, 65536, 100000])
def test_mixed_jobs_with_a_dictionary(dl, mixed_on_device):
    data, spans, plains = MIXED
    d = text_dict(dl)
    raw, n, jobs, bound = compress(data, spans, d, at=dl % 3, t=mixed_on_device)
    check_call(raw, n, jobs, bound, plains, d)


def test_mixed_jobs_with_every_checksum(mixed_on_device):
    data, spans, plains = MIXED
    raw, n, jobs, bound = compress(data, spans, D64K, dict_id=0xC0FFEE42, t=mixed_on_device, **ALL)
    assert bound == lz4ada.compress_frames_bound([n for _, n in spans], **ALL) + 4 * len(spans)
    check_call(raw, n, jobs, bound, plains, D64K, dict_id=0xC0FFEE42, **ALL)
    raw2, n2, _, _ = compress(data, spans, D64K, dict_id=0xC0FFEE42, at=2, t=mixed_on_device, **ALL)
    assert (raw2, n2) == (raw, n), "two calls differ"
    raw, n, jobs, bound = compress(data, spans, t=mixed_on_device, **ALL)
    check_call(raw, n, jobs, bound, plains, **ALL)


def test_capacity_one_below_the_bound(mixed_on_device):
    data, spans, _ = MIXED
    dt = to_device(text_dict(1000))
    for kw in (dict(), dict(dict=(dt.data_ptr(), dt.numel()), dict_id=3)):
        bound = lz4ada.compress_frames_bound([n for _, n in spans], **kw)
        out = torch.full((bound + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        with pytest.raises(lz4ada.TooLittleMemory) as e:
            lz4ada.compress_frames_device(mixed_on_device.data_ptr(), len(data), spans, out.data_ptr(), bound - 1,
                                          torch.cuda.current_stream().cuda_stream, linked=True, **kw)
        assert e.value.bound == bound
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()), "d_out was touched"


def test_misuse_launches_nothing():
    data = record(300)
    t, dt = to_device(data), to_device(text_dict(100))
    out = torch.full((1000 + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for cd in (lz4ada.CompressDict(dt.data_ptr(), -1, 0, 0), lz4ada.CompressDict(None, 100, 0, 0),
               lz4ada.CompressDict(dt.data_ptr(), 100, 0, 2), lz4ada.CompressDict(dt.data_ptr(), 100, 0, 0x80000001)):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.compress_frames_device(t.data_ptr(), 300, [(0, 300)], out.data_ptr(), 1000, stream, dict=cd,
                                          linked=True)
    for bad in (dict(block=3), dict(block=8)):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.compress_frames_device(t.data_ptr(), 300, [(0, 300)], out.data_ptr(), 1000, stream, linked=True,
                                          **bad)
    for span in ((1, 300), (-1, 10), (0, -1)):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.compress_frames_device(t.data_ptr(), 300, [span], out.data_ptr(), 1000, stream, linked=True)
    n = ctypes.c_int64()
    for flags in (8, 0x20):  # the options stay closed: linking is the entry
        opt = lz4ada.CompressOptions(4, flags)
        st = lz4ada._lib.lz4ada_compress_frames_device_linked(t.data_ptr(), 300, lz4ada._compress_jobs([(0, 300)]), 1,
                                                              ctypes.byref(opt), None, out.data_ptr(), 1000,
                                                              ctypes.byref(n), stream)
        assert st == 6  # LZ4ADA_ASSERTION_ERROR
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "d_out was touched"


def test_no_continuation_block_is_the_unlinked_call():
    """Records that all fit one block: the unlinked call's bytes apart from FLG
    and HC of every header, with and without a dictionary."""
    recs = [p for _, p in id4_records() if len(p) <= B]
    assert any(len(p) == B for p in recs)
    data, spans = b"", []
    for i, p in enumerate(recs):
        data += b"\x55" * (1 + i % 3)
        spans.append((len(data), len(p)))
        data += p
    for d in (None, D64K):
        raw, n, jobs, bound = compress(data, spans, d, **ALL)
        check_call(raw, n, jobs, bound, recs, d, **ALL)
        twin, tn, tjobs, tbound = compress(data, spans, d, linked=False, **ALL)
        assert (n, bound) == (tn, tbound)
        got = bytearray(raw)
        for i in range(len(spans)):
            assert (jobs[i].out_off, jobs[i].out_len) == (tjobs[i].out_off, tjobs[i].out_len)
            at = jobs[i].out_off
            hlen = dict_frame_blocks(raw[at:at + jobs[i].out_len])[6]
            assert got[at + 4] == twin[at + 4] ^ 0x20
            got[at + 4], got[at + hlen - 1] = twin[at + 4], twin[at + hlen - 1]
        assert bytes(got) == twin


def test_split_passes(monkeypatch, mixed_on_device):
    """LZ4ADA_BATCH_BYTES below the jobs' slots: the passes are cut between
    records, some hold a continuation block and some none, the same bytes."""
    data, spans, plains = MIXED
    want = compress(data, spans, D64K, dict_id=5, t=mixed_on_device, **ALL)
    budget = 200 * KiB
    assert sum(-(-len(p) // 256) * 256 for p in plains) > 3 * budget
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(budget))
    raw, n, jobs, bound = compress(data, spans, D64K, dict_id=5, t=mixed_on_device, **ALL)
    assert (raw, n, bound) == want[:2] + want[3:]
    check_call(raw, n, jobs, bound, plains, D64K, dict_id=5, **ALL)
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", "1")  # one record per pass
    few = [s for s in spans if s[1] in LENGTHS or s[1] < 100]
    raw, n, jobs, bound = compress(data, few, t=mixed_on_device)
    check_call(raw, n, jobs, bound, [data[o:o + k] for o, k in few])


def test_larger_blocks():
    """Blocks of 256 KiB: one record of 300,000 bytes, whose second block reads
    the last 64 KiB of the first, and two of one block."""
    plain = record(300000)
    data = b"\x00" * 5 + plain
    spans = [(5, 300000), (5, 4 * B), (7, 1000)]
    plains = [data[o:o + n] for o, n in spans]
    for d in (None, D64K):
        raw, n, jobs, bound = compress(data, spans, d, block=256 * KiB, **ALL)
        check_call(raw, n, jobs, bound, plains, d, block=256 * KiB, **ALL)
        assert jobs[0].stored_blocks == 0
    raw, n, jobs, bound = compress(plain[:100], [])
    assert (n, bound) == (0, 0) and raw == bytes([CANARY]) * GUARD
    raw, n, jobs, bound = compress(b"", [(0, 0), (0, 0)], **ALL)
    check_call(raw, n, jobs, bound, [b"", b""], **ALL)


# --------------------------------------------------------------- round trips

def d1_risk(plain, frame, d=b""):
    """Whether a block after the first holds a match that reaches 65,529 or more
    back, before its block: the shape the passes without a dictionary decline
    (quirk D1's round state) instead of decoding."""
    for i, (stored, payload, _) in enumerate(dict_frame_blocks(frame)[4]):
        at = 0
        for lit, off, ml in ([] if stored or i == 0 else parse_block_linked(payload, plain, i, B, d)):
            at += lit
            if off >= 65529 and off > at:
                return True
            at += ml
    return False


def round_trip_jobs():
    """The mixed jobs whose frames fit lz4ada_batch_linked_max()."""
    data, spans, plains = MIXED
    cap = lz4ada.batch_linked_max()
    keep = [i for i, p in enumerate(plains) if -(-len(p) // 256) * 256 + 256 <= cap]
    assert any(len(plains[i]) > 2 * B for i in keep)
    return data, [spans[i] for i in keep], [plains[i] for i in keep]


def test_round_trip_through_the_linked_pass(mixed_on_device):
    """decode_frames_device(linked=True): every frame comes back as its record,
    or, where a match has quirk D1's shape, is declined -- never other bytes."""
    data, spans, plains = round_trip_jobs()
    frames, where = lz4ada.compress_frames_tensor(mixed_on_device, spans, linked=True, content_checksum=True)
    got, jobs = lz4ada.decode_frames_tensor(frames, where, linked=True)
    got, raw = to_host(got), to_host(frames)
    declined = 0
    for i, plain in enumerate(plains):
        if jobs[i].status == lz4ada.EXACT_PATH:
            assert d1_risk(plain, raw[where[i][0]:where[i][0] + where[i][1]]), (i, jobs[i].reason)
            declined += 1
            continue
        assert (jobs[i].status, jobs[i].consumed) == (0, where[i][1]), (i, jobs[i].reason)
        assert got[jobs[i].out_off:jobs[i].out_off + jobs[i].out_len] == plain, i
    assert declined < len(plains) // 4


def test_round_trip_with_the_dictionary(mixed_on_device):
    """The dictionary pass has the specification's semantics: text records come
    back whole; a frame it declines (a stored 64 KiB block) gives no bytes."""
    data, spans, plains = round_trip_jobs()
    extra = dict_only_record(D64K)
    t = to_device(data + extra)
    spans, plains = spans + [(len(data), len(extra))], plains + [extra]
    dt = to_device(D64K)
    frames, where = lz4ada.compress_frames_tensor(t, spans, dict=dt, dict_id=77, linked=True, content_checksum=True)
    got, jobs = lz4ada.decode_frames_tensor(frames, where, linked=True, dict=dt, dict_id=77)
    got = to_host(got)
    good = 0
    for i, plain in enumerate(plains):
        if jobs[i].status == lz4ada.EXACT_PATH:
            continue
        assert (jobs[i].status, jobs[i].consumed) == (0, where[i][1]), (i, jobs[i].reason)
        assert got[jobs[i].out_off:jobs[i].out_off + jobs[i].out_len] == plain, i
        good += 1
    assert jobs[len(plains) - 1].status == 0, "the record whose block 0 reads the dictionary"
    assert good >= len(plains) * 3 // 4
    _, jobs = lz4ada.decode_frames_tensor(frames, where, linked=True, dict=dt, dict_id=78)
    assert all(jobs[i].status == lz4ada.EXACT_PATH for i in range(len(plains)))


def test_round_trip_through_a_linked_seek_index():
    """Ranges that straddle block boundaries, out of frames of 2 to 5 blocks."""
    recs = [pseudo_text(n, n + 3) for n in (2 * B + 1, B + 1024, 4 * B + 777, 3 * B)]
    data, spans = b"", []
    for p in recs:
        spans.append((len(data), len(p)))
        data += p
    frames, where = lz4ada.compress_frames_tensor(to_device(data), spans, linked=True, block_checksum=True)
    ranges = []
    for j, p in enumerate(recs):
        ranges += [(j, B - 5, 10), (j, B - 1, 2), (j, 0, len(p)), (j, B + 1, len(p) - B - 1), (j, len(p) - 3, 100)]
        if len(p) > 2 * B:
            ranges += [(j, B - 100, B + 200), (j, 2 * B - 1, 1), (j, 2 * B, 1)]
    with lz4ada.SeekIndex.build_tensor(frames, where, linked=True, checkpoint_bytes=2 * B) as idx:
        assert all(idx.jobs[j].status == 0 and idx.jobs[j].out_len == len(p) for j, p in enumerate(recs))
        got, arr = lz4ada.decode_ranges_tensor(idx, frames, ranges)
        got = to_host(got)
        for k, (j, off, n) in enumerate(ranges):
            want = recs[j][off:off + n]
            assert (arr[k].status, arr[k].out_len) == (0, len(want)), (k, arr[k].reason)
            assert got[arr[k].out_off:arr[k].out_off + arr[k].out_len] == want, k


def test_many_two_block_records():
    """256 records of 65,536 + 1,024 bytes, 512 blocks, more than the resident
    waves of some CUs: compared with the serial statement by digest."""
    n = B + KiB
    text = pseudo_text(n + 255 * 1531, 17)
    spans = [(i * 1531, n) for i in range(256)]
    frames, where = lz4ada.compress_frames_tensor(to_device(text), spans, linked=True)
    want, lens = hashlib.sha256(), []
    for o, k in spans:
        f = lz4ada.compress_frame_host(text[o:o + k], linked=True)
        want.update(f)
        lens.append(len(f))
    assert [w[1] for w in where] == lens
    assert hashlib.sha256(to_host(frames)).hexdigest() == want.hexdigest()
