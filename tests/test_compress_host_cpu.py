"""The compressor's serial statement: lz4ada_compress_block_host
and lz4ada_compress_frame_host, which the device call is tested against byte
for byte (tests/test_gpu_compress.py).  Round trips through the oracle, this
library's host decoder and, where the system has it, liblz4; a strict sequence
parser over every compressed block; crafted inputs at the token and extension
edges, the offset limit and the end-of-block rules; the ratio against liblz4's
recorded sizes (tests/golden/compress_sizes.json).  No GPU."""
import ctypes
import ctypes.util
import itertools
import json
import os

import pytest

import _oracle as O
import lz4ada
from _compress_cases import (BLOCK_LEN, KiB, LEN_ID5, frame_blocks, frame_bound, id4_records, noise, parse_block,
                             pseudo_text, record)
from _compress_edge_cases import A, far_repeat, planted
from conftest import GOLDEN

FLAG_SETS = [dict(zip(("block_checksum", "content_checksum", "content_size"), bits))
             for bits in itertools.product((False, True), repeat=3)]
ID4 = id4_records()


def oracle_decode(frame, n):
    st, out, _, msg = O.decode_stream(frame, out_cap=n + 64)
    assert st == O.OK, msg
    return out


def check_frame(frame, plain, block_id=4, block_checksum=False, content_checksum=False, content_size=False):
    """Everything a frame must be: the layout, the walk's verdict, every
    block's sequences, and the record back from two decoders."""
    n, blen = len(plain), BLOCK_LEN[block_id]
    assert len(frame) <= frame_bound(n, block_id, block_checksum, content_checksum, content_size)
    flg, bd, size, blocks, cck = frame_blocks(frame)
    assert flg == 0x60 | (0x10 if block_checksum else 0) | (8 if content_size else 0) | (4 if content_checksum else 0)
    assert bd == block_id << 4
    assert size == (n if content_size else None)
    assert len(blocks) == -(-n // blen)
    for i, (stored, payload, ck) in enumerate(blocks):
        part = plain[i * blen:(i + 1) * blen]
        if stored:
            assert payload == part
            assert len(lz4ada.compress_block_host(part, len(part) - 1)) == 0, "stored, yet it would have shrunk"
        else:
            assert len(payload) < len(part), "a block is stored whenever its compressed form is not shorter"
            parse_block(payload, part)
            assert payload == lz4ada.compress_block_host(part)
        assert ck == (O.xxh32(payload) if block_checksum else None)
    assert cck == (O.xxh32(plain) if content_checksum else None)
    v, info, descs = lz4ada.frame_walk_host(frame)
    assert v == lz4ada.BATCH_OK
    assert (info.nblocks, info.independent, info.frame_len, info.block_max) == (len(blocks), 1, len(frame), blen)
    assert (info.has_content_size, info.content_size) == (1, n) if content_size else info.has_content_size == 0
    assert [bool(descs[i].flags & lz4ada.BLOCK_STORED) for i in range(len(blocks))] == [b[0] for b in blocks]
    assert oracle_decode(frame, n) == plain
    out, used = lz4ada.decode_frame_dict_host(frame, out_cap=n)
    assert (out, used) == (plain, len(frame))
    return blocks


@pytest.mark.parametrize("name,plain", ID4, ids=[r[0] for r in ID4])
def test_round_trip_id4(name, plain):
    check_frame(lz4ada.compress_frame_host(plain), plain)


def test_round_trip_id5():
    plain = record(LEN_ID5)
    blocks = check_frame(lz4ada.compress_frame_host(plain, block=256 * KiB), plain, block_id=5)
    assert [len(b[1]) < 256 * KiB for b in blocks] == [True, True]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "".join("1" if v else "0" for v in f.values()))
@pytest.mark.parametrize("n", [14, 131073])
def test_every_flag_combination(n, flags):
    plain = record(n)
    check_frame(lz4ada.compress_frame_host(plain, **flags), plain, **flags)
    # a stored block carries its checksum too
    plain = noise(n, 5)
    check_frame(lz4ada.compress_frame_host(plain, **flags), plain, **flags)


def test_block_id_0_means_4():
    plain = record(65537)
    assert lz4ada.compress_frame_host(plain, block=0) == lz4ada.compress_frame_host(plain, block=4)


# ----------------------------------------------------------------- liblz4

def lz4f_decompress(frame, n):
    name = ctypes.util.find_library("lz4")
    if not name:
        pytest.skip("no liblz4 on this system")
    lz4 = ctypes.CDLL(name)
    lz4.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lz4.LZ4F_createDecompressionContext.restype = ctypes.c_size_t
    lz4.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t),
                                    ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    lz4.LZ4F_decompress.restype = ctypes.c_size_t
    lz4.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    lz4.LZ4F_isError.argtypes = [ctypes.c_size_t]
    ctx = ctypes.c_void_p()
    assert not lz4.LZ4F_isError(lz4.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    try:
        dst = ctypes.create_string_buffer(n + 1)
        src = ctypes.create_string_buffer(frame, len(frame))
        got, used, hint = 0, 0, 1
        while used < len(frame):
            dn, sn = ctypes.c_size_t(n + 1 - got), ctypes.c_size_t(len(frame) - used)
            hint = lz4.LZ4F_decompress(ctx, ctypes.byref(dst, got), ctypes.byref(dn), ctypes.byref(src, used),
                                       ctypes.byref(sn), None)
            assert not lz4.LZ4F_isError(hint), "LZ4F_decompress rejects the frame"
            assert dn.value or sn.value, "LZ4F_decompress makes no progress"
            got, used = got + dn.value, used + sn.value
        assert hint == 0, "LZ4F_decompress expects more input"
        return dst.raw[:got]
    finally:
        lz4.LZ4F_freeDecompressionContext(ctx)


def test_liblz4_reads_the_frames():
    all_flags = FLAG_SETS[-1]
    for name, plain in ID4:
        assert lz4f_decompress(lz4ada.compress_frame_host(plain), len(plain)) == plain, name
        assert lz4f_decompress(lz4ada.compress_frame_host(plain, **all_flags), len(plain)) == plain, name
    plain = record(LEN_ID5)
    assert lz4f_decompress(lz4ada.compress_frame_host(plain, block=256 * KiB, **all_flags), LEN_ID5) == plain


# ---------------------------------------------------------------- crafted

@pytest.mark.parametrize("lit", [14, 15, 16, 269, 270, 271])
def test_literal_run_edges(lit):
    data, want = planted(lit, 40)
    comp = lz4ada.compress_block_host(data)
    assert parse_block(comp, data) == want
    # the token's nibble and the 255-extension, byte for byte
    p = 1 + (len(A) - 15) // 255 + 1 + len(A) + 2 + 1  # past the first sequence (match length 32: one extension byte)
    assert comp[p] >> 4 == min(lit, 15)
    ext = {14: b"", 15: b"\x00", 16: b"\x01", 269: b"\xfe", 270: b"\xff\x00", 271: b"\xff\x01"}[lit]
    assert comp[p + 1:p + 1 + len(ext)] == ext
    assert comp[p + 1 + len(ext):p + 1 + len(ext) + lit] == data[len(A) + 32:len(A) + 32 + lit]


@pytest.mark.parametrize("ml", [18, 19, 20, 273, 274])
def test_match_length_edges(ml):
    data, want = planted(20, ml)
    comp = lz4ada.compress_block_host(data)
    assert parse_block(comp, data) == want
    p = 1 + (len(A) - 15) // 255 + 1 + len(A) + 2 + 1
    assert comp[p] == (15 << 4) | min(ml - 4, 15)  # 20 literals
    q = p + 2 + 20 + 2  # past the token, the literal extension, the literals and the offset
    ext = {18: b"", 19: b"\x00", 20: b"\x01", 273: b"\xfe", 274: b"\xff\x00"}[ml]
    assert comp[q:q + len(ext)] == ext
    assert comp[q + len(ext)] >> 4 == 15  # the last token: 20 literals


def test_offset_65535_is_matched_and_65536_is_not():
    data, at = far_repeat(65535)
    assert at > 1 << 17 and len(data) < 256 * KiB
    seqs = parse_block(lz4ada.compress_block_host(data), data)
    assert (0, 65535, 32) in seqs, seqs
    data, at = far_repeat(65536)
    seqs = parse_block(lz4ada.compress_block_host(data), data)
    assert all(off < 65535 and ml != 32 for _, off, ml in seqs), seqs
    assert seqs[-1][0] == 32 + 20  # the copy stays literal
    for d in (65535, 65536):  # and as a record of 256 KiB blocks
        data, _ = far_repeat(d)
        check_frame(lz4ada.compress_frame_host(data, block=256 * KiB), data, block_id=5)


def test_repeat_inside_the_last_12_bytes_stays_literal():
    data = A + A[:11]  # begins at n - 11
    assert parse_block(lz4ada.compress_block_host(data), data) == [(len(data), 0, 0)]
    data = A + A[:12]  # begins at n - 12, the last place: 7 bytes, then the last 5 as literals
    assert parse_block(lz4ada.compress_block_host(data), data) == [(len(A), len(A), 7), (5, 0, 0)]


def test_zeros_extend_past_the_window():
    """64 KiB of zeros: 64 literals and one match to the end.  A matcher that
    caps a match at its window comes out near 3 KiB."""
    plain = bytes(64 * KiB)
    comp = lz4ada.compress_block_host(plain)
    assert len(comp) <= 512
    assert parse_block(comp, plain) == [(64, 1, 64 * KiB - 5 - 64), (5, 0, 0)]
    blocks = check_frame(lz4ada.compress_frame_host(plain), plain)
    assert len(blocks[0][1]) <= 512


@pytest.mark.parametrize("n,block_id", [(65536, 4), (200000, 4), (300000, 5), (100, 4), (13, 4)])
def test_noise_is_stored_at_exactly_the_bound(n, block_id):
    plain = noise(n, n)
    for flags in (FLAG_SETS[0], FLAG_SETS[-1]):
        frame = lz4ada.compress_frame_host(plain, block=BLOCK_LEN[block_id], **flags)
        blocks = check_frame(frame, plain, block_id=block_id, **flags)
        assert all(b[0] for b in blocks)  # stored_blocks == the block count
        assert len(frame) == frame_bound(n, block_id, *flags.values())
        assert len(frame) == lz4ada.compress_frames_bound([n], BLOCK_LEN[block_id], **flags)


# ------------------------------------------------------------------ ratio

def test_ratio_against_liblz4():
    """Frames of 16 x 64 KiB, 64 x 4 KiB and 64 x 1 KiB text records total at
    most 1.10 times liblz4's recorded block sizes plus the frame overhead (15
    bytes per one-block frame).  Measured with the rule of DESIGN.md §17 on this
    text: 1.07, 1.02 and 1.00."""
    with open(os.path.join(GOLDEN, "compress_sizes.json")) as fh:
        gold = json.load(fh)
    text = pseudo_text(16 * 64 * KiB, gold["seed"])
    for block, count in ((64 * KiB, 16), (4 * KiB, 64), (KiB, 64)):
        want = gold["sizes"][str(block)]
        assert len(want) == count
        total = sum(len(lz4ada.compress_frame_host(text[i * block:(i + 1) * block])) for i in range(count))
        overhead = count * (7 + 4 + 4)
        print(f"{count} x {block}: {total} bytes, liblz4 {sum(want)}: {(total - overhead) / sum(want):.4f}")
        assert total <= 1.10 * sum(want) + overhead


# ------------------------------------------------- misuse and capacity

def raw_frame(plain, opt, cap, guard=64):
    buf = ctypes.create_string_buffer(b"\xa5" * (cap + guard), cap + guard)
    n = lz4ada._lib.lz4ada_compress_frame_host(plain if plain else None, len(plain), ctypes.byref(opt), buf, cap)
    return n, buf.raw


@pytest.mark.parametrize("n", [0, 13, 300])
def test_every_capacity_below_the_bound(n):
    plain = record(n)
    for flags in (0, 7):
        opt = lz4ada.CompressOptions(4, flags)
        bound = frame_bound(n, 4, *(bool(flags),) * 3)
        assert lz4ada.compress_frames_bound([n], 65536, *(bool(flags),) * 3) == bound
        for cap in range(bound):
            got, raw = raw_frame(plain, opt, cap)
            assert got == -5 and raw == b"\xa5" * (cap + 64), cap  # LZ4ADA_TOO_LITTLE_MEMORY, dst untouched
        got, raw = raw_frame(plain, opt, bound)
        assert 0 < got <= bound and raw[bound:] == b"\xa5" * 64
        assert raw[:got] == lz4ada.compress_frame_host(plain, block_checksum=bool(flags),
                                                       content_checksum=bool(flags), content_size=bool(flags))


def test_capacity_of_a_multi_block_record():
    plain = record(131073)
    opt = lz4ada.CompressOptions(4, 7)
    bound = frame_bound(131073, 4, True, True, True)
    for cap in (0, 1, 7, 65536, bound - 1):
        got, raw = raw_frame(plain, opt, cap)
        assert got == -5 and raw == b"\xa5" * (cap + 64)
    with pytest.raises(lz4ada.TooLittleMemory):
        lz4ada.compress_frame_host(plain, cap=bound - 1, **FLAG_SETS[-1])


@pytest.mark.parametrize("name", ["text300", "zeros300", "planted"])
def test_block_capacities(name):
    """Every capacity below a block's length gives 0, and nothing behind dst + cap is written."""
    plain = {"text300": pseudo_text(300, 3), "zeros300": bytes(300), "planted": planted(270, 274)[0]}[name]
    comp = lz4ada.compress_block_host(plain)
    for cap in range(len(comp) + 2):
        buf = ctypes.create_string_buffer(b"\xa5" * (cap + 64), cap + 64)
        got = lz4ada._lib.lz4ada_compress_block_host(plain, len(plain), buf, cap)
        assert got == (len(comp) if cap >= len(comp) else 0), cap
        assert buf.raw[cap:] == b"\xa5" * 64, cap
        if got:
            assert buf.raw[:got] == comp


def test_misuse():
    for block, flags in ((3, 0), (8, 0), (1, 0), (4, 8), (0, 0x80000000)):
        opt = lz4ada.CompressOptions(block, flags)
        buf = ctypes.create_string_buffer(256)
        assert lz4ada._lib.lz4ada_compress_frame_host(b"abc", 3, ctypes.byref(opt), buf, 256) == -6
        jobs = lz4ada._compress_jobs([(0, 3)])
        assert lz4ada._lib.lz4ada_compress_frames_bound(jobs, 1, ctypes.byref(opt)) == -1
        with pytest.raises(lz4ada.AssertionFailure):  # before any launch: no GPU needed
            _device_call(opt)
    assert lz4ada._lib.lz4ada_compress_frame_host(None, 3, None, ctypes.create_string_buffer(64), 64) == -6
    assert lz4ada._lib.lz4ada_compress_block_host(None, 3, ctypes.create_string_buffer(64), 64) == -1
    assert lz4ada._lib.lz4ada_compress_block_host(b"abc", -1, ctypes.create_string_buffer(64), 64) == -1
    assert lz4ada._lib.lz4ada_compress_frames_bound(lz4ada._compress_jobs([(0, -1)]), 1, None) == -1
    for span in ((-1, 2), (0, 4), (2, 2), (4, 0)):  # a range outside [0, in_len)
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.compress_frames_device(0x1000, 3, [(0, 3), span], 0x2000, 1 << 20)


def _device_call(opt):
    jobs = lz4ada._compress_jobs([(0, 3)])
    n = ctypes.c_int64()
    st = lz4ada._lib.lz4ada_compress_frames_device(0x1000, 3, jobs, 1, ctypes.byref(opt), 0x2000, 256,
                                                   ctypes.byref(n), None)
    lz4ada._check(st, lz4ada._thread_error())


def test_device_call_reports_the_bound_without_a_launch():
    lens = [0, 5, 70000]
    bound = lz4ada.compress_frames_bound(lens, content_checksum=True)
    assert bound == sum(frame_bound(n, 4, cck=True) for n in lens)
    with pytest.raises(lz4ada.TooLittleMemory) as e:
        lz4ada.compress_frames_device(0x1000, 70005, [(0, 0), (0, 5), (5, 70000)], 0x2000, bound - 1,
                                      content_checksum=True)
    assert e.value.bound == bound


def test_device_call_without_gpu_fails_loudly():
    if lz4ada.device_available():
        pytest.skip("a GPU is present")
    with pytest.raises(lz4ada.DeviceError):
        lz4ada.compress_frames_device(0x1000, 3, [(0, 3)], 0x2000, 256)
