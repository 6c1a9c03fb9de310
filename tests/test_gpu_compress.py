"""Records compressed into LZ4 frames on the GPU (lz4ada_compress_frames_device,
DESIGN.md §17).  The yardstick is the serial statement, byte for byte
(lz4ada_compress_frame_host, which tests/test_compress_host_cpu.py pins to the
format and to three decoders), so no decoder stands between the kernel and the
check; then the call's contract -- order, density, the guard region, the bound
-- and the frames back through this library's device calls without any flag."""
import hashlib

import pytest
import torch

import _oracle as O
import lz4ada
from _compress_cases import KiB, LEN_ID5, MiB, frame_blocks, id4_records, pseudo_text, record

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


def to_device(data):
    t = torch.empty(max(len(data), 1), dtype=torch.uint8, device="cuda")
    t[:len(data)] = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8)[:len(data)]
    return t[:len(data)]


def to_host(t):
    return t.cpu().numpy().tobytes()


def compress(data, spans, slack=0, **kw):
    """One call into a canary-filled buffer of bound + slack + GUARD bytes with
    out_cap = bound + slack -> (the whole buffer's bytes, bytes written, jobs, bound)."""
    bound = lz4ada.compress_frames_bound([n for _, n in spans], **kw)
    t = to_device(data)
    out = torch.full((bound + slack + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    n, jobs = lz4ada.compress_frames_device(t.data_ptr() if len(data) else None, len(data), spans, out.data_ptr(),
                                            bound + slack, torch.cuda.current_stream().cuda_stream, **kw)
    return to_host(out), n, jobs, bound


def check_call(raw, n, jobs, bound, plains, slack=0, **kw):
    """Dense frames in job order that equal the serial statement's, and nothing
    written at or beyond the call's length."""
    at = 0
    for i, plain in enumerate(plains):
        want = lz4ada.compress_frame_host(plain, **kw)
        assert (jobs[i].out_off, jobs[i].out_len, jobs[i].status) == (at, len(want), 0), i
        assert raw[at:at + len(want)] == want, f"job {i} ({len(plain)} bytes) differs from the serial statement"
        assert jobs[i].stored_blocks == sum(b[0] for b in frame_blocks(want)[3]), i
        at += len(want)
    assert n == at <= bound
    assert raw[n:] == bytes([CANARY]) * (bound + slack + GUARD - n), "bytes at or beyond *out_len were written"


def mixed_jobs():
    """Every record of the CPU lists laid out at odd places of one input, the
    jobs in an order of their own, with jobs that overlap others -> (input,
    spans, the plaintext of every job)."""
    recs = [r for _, r in id4_records()]
    data, where = b"", []
    for i, r in enumerate(recs):
        data += b"\x55" * (1 + i % 3)  # no record starts aligned by accident
        where.append((len(data), len(r)))
        data += r
    order = list(range(len(recs)))[::-1]
    order = order[1::2] + order[0::2]  # out of order in in_off
    spans = [where[i] for i in order]
    big = max(where, key=lambda w: w[1])
    spans += [(big[0] + 100, 70000), (big[0] + 3, 13), (big[0], big[1]), (big[0] + 65536 - 7, 65537)]
    return data, spans, [data[o:o + n] for o, n in spans]


def test_bytes_equal_the_serial_statement():
    data, spans, plains = mixed_jobs()
    raw, n, jobs, bound = compress(data, spans, slack=1000)
    check_call(raw, n, jobs, bound, plains, slack=1000)
    raw2, n2, _, _ = compress(data, spans, slack=1000)
    assert (raw2, n2) == (raw, n), "two calls differ"


def test_id5_record_and_no_jobs():
    plain = record(LEN_ID5)
    raw, n, jobs, bound = compress(b"\x00" * 5 + plain, [(5, LEN_ID5)], block=256 * KiB)
    check_call(raw, n, jobs, bound, [plain], block=256 * KiB)
    raw, n, jobs, bound = compress(plain[:100], [])
    assert (n, bound) == (0, 0) and raw == bytes([CANARY]) * GUARD
    raw, n, jobs, bound = compress(b"", [(0, 0), (0, 0)], **ALL)
    check_call(raw, n, jobs, bound, [b"", b""], **ALL)


def test_capacity_one_below_the_bound():
    data, spans, _ = mixed_jobs()
    bound = lz4ada.compress_frames_bound([n for _, n in spans])
    t = to_device(data)
    out = torch.full((bound + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(lz4ada.TooLittleMemory) as e:
        lz4ada.compress_frames_device(t.data_ptr(), len(data), spans, out.data_ptr(), bound - 1,
                                      torch.cuda.current_stream().cuda_stream)
    assert e.value.bound == bound
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "d_out was touched"


def test_round_trip_on_the_device():
    """decode_frames_device without flags returns the records, frames_device_sizes
    their lengths, and a SeekIndex serves a range from the middle of a
    multi-block record (64 KiB blocks)."""
    data, spans, plains = mixed_jobs()
    frames, where = lz4ada.compress_frames_tensor(to_device(data), spans)
    got, jobs = lz4ada.decode_frames_tensor(frames, where)
    got = to_host(got)
    for i, plain in enumerate(plains):
        assert (jobs[i].status, jobs[i].consumed) == (0, where[i][1]), (i, jobs[i].reason)
        assert got[jobs[i].out_off:jobs[i].out_off + jobs[i].out_len] == plain, i
    total, sized = lz4ada.frames_device_sizes(frames.data_ptr(), frames.numel(), where,
                                              torch.cuda.current_stream().cuda_stream)
    assert [sized[i].out_len for i in range(len(plains))] == [len(p) for p in plains]
    assert total == sum(len(p) for p in plains)
    k = max(range(len(plains)), key=lambda i: len(plains[i]))
    assert len(plains[k]) > 2 * 64 * KiB
    with lz4ada.SeekIndex.build_tensor(frames, where) as idx:
        part, ranges = lz4ada.decode_ranges_tensor(idx, frames, [(k, 60000, 12000), (k, 131000, 73)])
        assert [r.status for r in ranges[:2]] == [0, 0]
        assert to_host(part) == plains[k][60000:72000] + plains[k][131000:131073]


def test_checksums_and_the_host_chain(monkeypatch):
    """All three flags: the oracle accepts every frame, so the header, block
    and content checksums are right -- also for the record over
    lz4ada_batch_hash_max(), whose content checksum the host chain supplies."""
    monkeypatch.setenv("LZ4ADA_BATCH_HASH_MAX", "100000")
    assert lz4ada.batch_hash_max() == 100000
    data, spans, plains = mixed_jobs()
    assert max(len(p) for p in plains) > 100000 > min(len(p) for p in plains if len(p) > 65536)
    raw, n, jobs, bound = compress(data, spans, **ALL)
    check_call(raw, n, jobs, bound, plains, **ALL)
    for i, plain in enumerate(plains):
        frame = raw[jobs[i].out_off:jobs[i].out_off + jobs[i].out_len]
        st, out, _, msg = O.decode_stream(frame, out_cap=len(plain) + 64)
        assert st == O.OK and out == plain, (i, msg)


def test_split_passes(monkeypatch):
    """LZ4ADA_BATCH_BYTES below the jobs' slots: several passes, the same bytes."""
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(200 * KiB))
    data, spans, plains = mixed_jobs()
    raw, n, jobs, bound = compress(data, spans, **ALL)
    check_call(raw, n, jobs, bound, plains, **ALL)


def test_large_block():
    """One id-7 record of 4 MiB + 5 bytes of text: a 4 MiB block is one wave's work."""
    plain = (pseudo_text(MiB, 9) * 5)[:4 * MiB + 5]
    raw, n, jobs, bound = compress(plain, [(0, len(plain))], block=4 * MiB, content_size=True)
    check_call(raw, n, jobs, bound, [plain], block=4 * MiB, content_size=True)
    assert jobs[0].stored_blocks == 1  # the five bytes
    out, used = lz4ada.decode_frame(raw[:n])
    assert (bytes(out), used) == (plain, n)


def test_many_blocks():
    """2,048 records of 64 KiB, more blocks than resident waves, as overlapping
    jobs of one MiB of text; compared with the serial statement by digest."""
    text = pseudo_text(MiB, 5)
    spans = [((i * 977) % (MiB - 64 * KiB), 64 * KiB) for i in range(2048)]
    frames, where = lz4ada.compress_frames_tensor(to_device(text), spans)
    want, lens = hashlib.sha256(), []
    for o, n in spans:
        f = lz4ada.compress_frame_host(text[o:o + n])
        want.update(f)
        lens.append(len(f))
    assert [w[1] for w in where] == lens
    assert hashlib.sha256(to_host(frames)).hexdigest() == want.hexdigest()
