"""Many frames in one device pass (lz4ada_decode_frames and the routing of
decode_stream): every frame's bytes, extent and verdict against the
generator's plaintext and the oracle; one bad frame among ~300 costs only
itself and is reported with the reference's text; the pass splits by the
byte budget; content checksums above G go to the host chain; the device scan
behind the layout crosses its tiles and its second level."""
import ctypes
import random
import struct

import pytest
import xxhash

import _lz4build as B
import _oracle as O
import lz4ada
import lz4frame
from conftest import error_vectors, read_eds, read_vector

pytestmark = pytest.mark.gpu

# every compacted start alignment mod 4 and every XXH32 tail length occurs
SIZES = [0, 1, 2, 3, 15, 16, 17, 4095, 65536, 65537, 3 * 65536 + 1000]
MANY_AT = 150   # the frame of 40 blocks
MIDDLE = 137    # where the bad-frame cases put their frame


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


def block_of(rng, kind, n, seed):
    """(payload, decoded, stored) of about n bytes: gen_block kinds 0-4, a
    random-sequence block (5), a stored block (6)."""
    if kind == 6:
        raw = rng.randbytes(n)
        return raw, raw, True
    if kind == 5 and n >= 4096:
        seqs = B.sparse_seqs(rng, n - 3400)  # the last sequence adds at most 800 + 2500
        comp, raw = B.encode(seqs, final_lits=rng.randbytes(5))
        assert len(raw) <= 65536
        return comp, raw, False
    if kind >= 4 and n < 64:
        kind = 1
    comp, raw = lz4ada.gen_block(kind % 5, seed, n)
    return comp, raw, False


def make_frame(i, sizes=None):
    rng = random.Random(9000 + i)
    n = SIZES[i % len(SIZES)]
    pieces = sizes if sizes is not None else [min(65536, n - at) for at in range(0, n, 65536)]
    blocks = [block_of(rng, (i + k) % 7, m, 100 * i + k) for k, m in enumerate(pieces)]
    return lz4frame.build_frame(blocks, (4 << 20) if i & 8 else (64 << 10), block_cksum=bool(i & 1),
                                content_cksum=bool(i & 2), with_content_size=bool(i & 4))


@pytest.fixture(scope="module")
def batch():
    """[(frame, plaintext, has content checksum)] * 300; never modified."""
    out = []
    for i in range(300):
        f, raw = make_frame(i, [65536] * 39 + [777] if i == MANY_AT else None)
        out.append((f, raw, bool(i & 2)))
    return tuple(out)


def stats():
    s = lz4ada.last_batch_stats()
    return dict(batched=s.frames_batched, single=s.frames_single, passes=s.passes,
                gpu=s.gpu_hashed, host=s.host_hashed)


def check_jobs(out, jobs, items, skip=()):
    at = 0
    for i, (f, raw, _) in enumerate(items):
        j = jobs[i]
        assert j.out_off == at, i
        at += j.out_len
        if i in skip:
            continue
        assert (j.status, j.consumed, j.out_len) == (0, len(f), len(raw)), i
        assert out[j.out_off:j.out_off + j.out_len] == raw, i
    assert at == len(out)


def test_parity_and_layout(batch):
    frames = [f for f, _, _ in batch]
    assert max(len(raw) for _, raw, _ in batch) <= lz4ada.batch_hash_max()  # all under G
    assert {sum(len(r) for _, r, _ in batch[:i]) & 3 for i in range(300)} == {0, 1, 2, 3}
    out, jobs = lz4ada.decode_frames_jobs(frames)
    check_jobs(out, jobs, batch)
    assert all(jobs[i].path == lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT for i in range(300))
    assert lz4ada.last_path() == lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT
    assert stats() == dict(batched=300, single=0, passes=1, host=0,
                           gpu=sum(1 for _, _, ck in batch if ck))
    res = lz4ada.decode_frames(frames)
    assert [(r[0], r[1], r[2]) for r in res] == [(raw, len(f), None) for f, raw, _ in batch]


def oracle_alone(frames: bytes) -> bytes:
    st, out, _, msg = O.decode_stream(frames, out_cap=4 << 20)
    assert st == O.OK, msg
    return out


@pytest.fixture(scope="module")
def mixed_stream(batch):
    """The batch as one stream with a skippable + modern pair, a legacy frame
    and one linked frame in the middle -> (stream, expected bytes, frames
    built as non-batchable).  Expected: the generator's plaintext, and the
    oracle on each inserted piece alone -- one oracle context cannot take the
    whole stream (it keeps the first frame's block maximum), and the CLI
    loop's 4 KiB reads fail a header that straddles a read."""
    blocks = [(c, r, False) for c, r in lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, 77, 65536, 3)]
    linked, linked_raw = lz4frame.build_frame(blocks, 64 << 10, indep=False, content_cksum=True)
    assert oracle_alone(linked) == linked_raw
    parts = [(f, raw) for f, raw, _ in batch]
    parts[200:200] = [(linked, linked_raw)]
    for at, name in ((100, "z100legacy"), (50, "skipz100")):
        v = read_vector(name, "lz4")
        parts[at:at] = [(v, oracle_alone(v))]
    return b"".join(f for f, _ in parts), b"".join(r for _, r in parts), 1


def test_stream_equals_oracle(mixed_stream):
    data, want, non_batchable = mixed_stream
    assert lz4ada.decode_stream(data) == want
    assert lz4ada.last_path() & (lz4ada.PATH_BATCH | lz4ada.PATH_LINKED) == \
        lz4ada.PATH_BATCH | lz4ada.PATH_LINKED
    s = stats()
    assert s["single"] == non_batchable
    assert s["batched"] == 300 + 3  # skippable, z100, z100legacy
    entries = lz4ada.stream_index(data)
    assert sum(1 for e in entries if e.batchable != lz4ada.BATCH_OK) == non_batchable
    # the fixed-buffer call: the same bytes and their count
    buf = ctypes.create_string_buffer(len(want) + 1)
    n = ctypes.c_int64(-1)
    assert lz4ada._lib.lz4ada_decode_stream(data, len(data), buf, len(buf), ctypes.byref(n)) == 0
    assert n.value == len(want) and buf.raw[:n.value] == want


def test_no_batch_switch(mixed_stream, monkeypatch):
    data, want, _ = mixed_stream
    monkeypatch.setenv("LZ4ADA_NO_BATCH", "1")
    assert lz4ada.decode_stream(data) == want
    assert not lz4ada.last_path() & lz4ada.PATH_BATCH
    assert stats()["batched"] == 0 and stats()["passes"] == 0


# ------------------------------------------------------- one bad frame

def three_blocks(**kw):
    blocks = [(*lz4ada.gen_block(1, 500 + k, n), False) for k, n in enumerate([65536, 65536, 1000])]
    return lz4frame.build_frame(blocks, 64 << 10, **kw)


def resized(delta):
    blocks = [(*lz4ada.gen_block(1, 600 + k, n), False) for k, n in enumerate([65536, 1000])]
    raw = b"".join(b[1] for b in blocks)
    return lz4frame.header(64 << 10, content_cksum=True, content_size=len(raw) + delta) + \
        b"".join(lz4frame.block_record(b[0]) for b in blocks) + lz4frame.trailer(raw, True)


def bad_frame(kind):
    if kind == "block_checksum":
        f, _ = three_blocks(block_cksum=True, content_cksum=True)
        _, descs = lz4ada.frame_index(f)
        b = bytearray(f)
        b[descs[1].in_off + descs[1].in_len] ^= 0x10  # the second block's checksum
        return bytes(b)
    if kind == "content_checksum":
        f, _ = three_blocks(content_cksum=True)
        return f[:-1] + bytes([f[-1] ^ 0x01])
    if kind == "size_long":
        return resized(+5)
    if kind == "size_short":
        return resized(-5)
    return read_vector(kind, "err")


BAD_KINDS = ["block_checksum", "content_checksum", "size_long", "size_short"] + error_vectors()


@pytest.mark.parametrize("kind", BAD_KINDS)
def test_one_bad_frame_does_not_cost_the_others(batch, kind):
    bad = bad_frame(kind)
    ref_out, ref_cons, ref_exc = lz4ada.decode_frame_partial(bad)
    ost, oracle_out, omsg = O.unlz4ada(bad)
    items = list(batch)
    items[MIDDLE] = (bad, ref_out, False)
    out, jobs = lz4ada.decode_frames_jobs([f for f, _, _ in items])
    check_jobs(out, jobs, items, skip={MIDDLE})
    j = jobs[MIDDLE]
    got = out[j.out_off:j.out_off + j.out_len]
    msg = lz4ada._lib.lz4ada_frames_error(MIDDLE).decode()
    if ref_exc is None:  # trailingbytes: a good frame, then bytes its caller gets back
        assert kind == "trailingbytes"
        assert (j.status, j.consumed, got, msg) == (0, ref_cons, ref_out, "")
    else:
        exc = lz4ada._ERRORS[j.status](msg)
        assert (type(exc), exc.message) == (type(ref_exc), ref_exc.message)
        if kind in error_vectors():
            assert str(exc) == read_eds(kind)
        assert got == ref_out  # what the reference output before raising
        if str(exc) == O.exception_information(ost, omsg):  # its CLI loop raises the same
            assert got == oracle_out
        assert j.consumed == 0
    # the same inputs as one stream: the oracle's exception after the frames before
    data = b"".join(f for f, _, _ in items)
    st, _, smsg = O.unlz4ada(data, out_cap=len(out) + (64 << 20))
    assert st != O.OK
    with pytest.raises(lz4ada.LZ4AdaError) as ei:
        lz4ada.decode_stream(data)
    assert str(ei.value) == O.exception_information(st, smsg)
    cap = len(out) + (1 << 20)
    buf = ctypes.create_string_buffer(cap)
    n = ctypes.c_int64(-1)
    cst = lz4ada._lib.lz4ada_decode_stream(data, len(data), buf, cap, ctypes.byref(n))
    assert cst != 0 and lz4ada._thread_error() == smsg
    before = sum(len(raw) for _, raw, _ in items[:MIDDLE])
    # trailingbytes fails only at the bytes after its own, whole, frame
    assert n.value == before + (len(ref_out) if ref_exc is None else 0)
    assert buf.raw[:before] == out[:before]


# ------------------------------------------------------------ pass splitting

def test_pass_splitting(monkeypatch):
    items = []
    for i in range(64):
        comp, raw = lz4ada.gen_block(1, 3000 + i, 65536)
        f, _ = lz4frame.build_frame([(comp, raw, False)], 64 << 10, content_cksum=True)
        items.append((f, raw, True))
    whole, _ = lz4ada.decode_frames_jobs([f for f, _, _ in items])
    assert stats()["passes"] == 1
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(1 << 20))
    out, jobs = lz4ada.decode_frames_jobs([f for f, _, _ in items])
    check_jobs(out, jobs, items)
    assert out == whole
    s = stats()
    assert s["passes"] == 4 and s["batched"] == 64 and s["single"] == 0  # 16 slots of 64 KiB each
    # a frame larger than the budget goes on its own and is still right
    big = make_frame(MANY_AT, [65536] * 39 + [777])
    items.insert(20, (big[0], big[1], True))
    out, jobs = lz4ada.decode_frames_jobs([f for f, _, _ in items])
    check_jobs(out, jobs, items)
    s = stats()
    assert s["single"] == 1 and s["batched"] == 64 and s["passes"] > 1
    assert not jobs[20].path & lz4ada.PATH_BATCH


# ---------------------------------------------------------- host-hash branch

def test_host_hash_branch(batch, monkeypatch):
    monkeypatch.setenv("LZ4ADA_BATCH_HASH_MAX", "4096")
    assert lz4ada.batch_hash_max() == 4096
    out, jobs = lz4ada.decode_frames_jobs([f for f, _, _ in batch])
    check_jobs(out, jobs, batch)
    s = stats()
    assert s["host"] == sum(1 for _, raw, ck in batch if ck and len(raw) > 4096) > 0
    assert s["gpu"] == sum(1 for _, raw, ck in batch if ck and len(raw) <= 4096) > 0
    assert s["batched"] == 300 and s["single"] == 0
    # a flipped content checksum on a host-hashed frame: the reference's text
    bad = bad_frame("content_checksum")
    ref_out, _, ref_exc = lz4ada.decode_frame_partial(bad)
    assert isinstance(ref_exc, lz4ada.ChecksumError) and len(ref_out) > 4096
    items = list(batch)
    items[MIDDLE] = (bad, ref_out, True)
    out, jobs = lz4ada.decode_frames_jobs([f for f, _, _ in items])
    check_jobs(out, jobs, items, skip={MIDDLE})
    j = jobs[MIDDLE]
    assert lz4ada._ERRORS[j.status] is lz4ada.ChecksumError
    assert lz4ada._lib.lz4ada_frames_error(MIDDLE).decode() == ref_exc.message
    assert out[j.out_off:j.out_off + j.out_len] == ref_out
    assert stats()["single"] == 1


# ------------------------------------------------- the scan and the span hash

def tiny_blocks_frame(rng, nblocks):
    """One frame of nblocks stored blocks of 1-3 bytes."""
    raw = rng.randbytes(3 * nblocks)
    recs, plain, at = [], [], 0
    for k in range(nblocks):
        n = 1 + (k % 3)
        recs.append(struct.pack("<I", 0x80000000 | n) + raw[at:at + n])
        plain.append(raw[at:at + n])
        at += n
    plain = b"".join(plain)
    return lz4frame.header(64 << 10, content_cksum=True) + b"".join(recs) + \
        lz4frame.trailer(plain, True), plain


def test_scan_crosses_tiles_and_levels():
    """280,001 blocks: 274 tiles of the first level, so the second level's one
    workgroup takes two rounds with a carry; frames start inside tiles."""
    rng = random.Random(4)
    items = [(*tiny_blocks_frame(rng, n), True) for n in (1, 139_000, 1_000, 140_000)]
    out, jobs = lz4ada.decode_frames_jobs([f for f, _, _ in items])
    check_jobs(out, jobs, items)
    assert stats() == dict(batched=4, single=0, passes=1, gpu=4, host=0)


def test_xxh32_spans_kernel_alone():
    import torch
    rng = random.Random(11)
    buf = rng.randbytes(300_000)
    spans = [(a, n) for a in (0, 1, 2, 3, 4097) for n in (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64,
                                                            65, 1000, 4096, 65536, 200_001)]
    spans.append((len(buf) - 19, 19))  # ends with the buffer
    d_buf = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    got, ms = lz4ada.xxh32_spans_device(d_buf.data_ptr(), spans)
    assert got == [xxhash.xxh32(buf[a:a + n]).intdigest() for a, n in spans]
    assert ms >= 0
