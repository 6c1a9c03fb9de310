"""The compressor's serial statement with a dictionary:
lz4ada_compress_block_dict_host and lz4ada_compress_frame_dict_host, which the
device call is tested against byte for byte (tests/test_gpu_compress_dict.py).
Round trips through this library's host decoder, liblz4's frame decoder and its
block decoder; a strict sequence parser that knows the dictionary over every
compressed block; the dictionary lengths around 4 and 65,536; crafted records
at the boundary between dictionary and block; the id in the header; the ratio
against liblz4's recorded sizes (tests/golden/compress_dict_sizes.json).  No
GPU."""
import ctypes
import ctypes.util
import json
import os

import pytest

import _oracle as O
import lz4ada
from _compress_cases import BLOCK_LEN, KiB, LEN_ID5, frame_bound, id4_records, pseudo_text, record
from _compress_dict_cases import (DICT_LENGTHS, RECORDED, crafted, dict_frame_blocks, parse_block_dict,
                                  reads_dictionary, second_block_from_dictionary, text_dict)
from conftest import GOLDEN

ID4 = id4_records()
D64K = text_dict(65536)
CRAFTED = crafted()
ALL = dict(block_checksum=True, content_checksum=True, content_size=True)


def liblz4():
    name = ctypes.util.find_library("lz4")
    return ctypes.CDLL(name) if name else None


def lz4_block_using_dict(lz4, payload, n, d):
    lz4.LZ4_decompress_safe_usingDict.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_char_p, ctypes.c_int]
    dst = ctypes.create_string_buffer(max(n, 1))
    got = lz4.LZ4_decompress_safe_usingDict(payload, dst, len(payload), n, d, len(d))
    assert got == n, "LZ4_decompress_safe_usingDict rejects the block"
    return dst.raw[:n]


def lz4f_using_dict(lz4, frame, n, d):
    size_t = ctypes.c_size_t
    lz4.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lz4.LZ4F_createDecompressionContext.restype = size_t
    lz4.LZ4F_decompress_usingDict.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(size_t),
                                              ctypes.c_void_p, ctypes.POINTER(size_t), ctypes.c_char_p, size_t,
                                              ctypes.c_void_p]
    lz4.LZ4F_decompress_usingDict.restype = size_t
    lz4.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    lz4.LZ4F_isError.argtypes = [size_t]
    ctx = ctypes.c_void_p()
    assert not lz4.LZ4F_isError(lz4.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    try:
        dst = ctypes.create_string_buffer(n + 1)
        src = ctypes.create_string_buffer(frame, len(frame))
        got, used, hint = 0, 0, 1
        while used < len(frame):
            dn, sn = size_t(n + 1 - got), size_t(len(frame) - used)
            hint = lz4.LZ4F_decompress_usingDict(ctx, ctypes.byref(dst, got), ctypes.byref(dn),
                                                 ctypes.byref(src, used), ctypes.byref(sn), d, len(d), None)
            assert not lz4.LZ4F_isError(hint), "LZ4F_decompress_usingDict rejects the frame"
            assert dn.value or sn.value, "LZ4F_decompress_usingDict makes no progress"
            got, used = got + dn.value, used + sn.value
        assert hint == 0, "LZ4F_decompress_usingDict expects more input"
        return dst.raw[:got]
    finally:
        lz4.LZ4F_freeDecompressionContext(ctx)


def check_frame(frame, plain, d, block_id=4, dict_id=None, block_checksum=False, content_checksum=False,
                content_size=False):
    """The layout, every block's sequences under the dictionary, and the record
    back from this library's host decoder -> [(stored, payload, sequences or None)]."""
    n, blen = len(plain), BLOCK_LEN[block_id]
    extra = 4 if dict_id is not None else 0
    assert len(frame) <= frame_bound(n, block_id, block_checksum, content_checksum, content_size) + extra
    flg, bd, size, did, blocks, cck, _ = dict_frame_blocks(frame)
    assert flg == (0x60 | (0x10 if block_checksum else 0) | (8 if content_size else 0) | (4 if content_checksum else 0)
                   | (1 if dict_id is not None else 0))
    assert (bd, size, did) == (block_id << 4, n if content_size else None, dict_id)
    assert len(blocks) == -(-n // blen)
    res = []
    for i, (stored, payload, ck) in enumerate(blocks):
        part = plain[i * blen:(i + 1) * blen]
        seqs = None
        if stored:
            assert payload == part
            assert len(lz4ada.compress_block_host(part, len(part) - 1, dict=d)) == 0, "stored, yet it would have shrunk"
        else:
            assert len(payload) < len(part), "a block is stored whenever its compressed form is not shorter"
            seqs = parse_block_dict(payload, part, d)
            assert payload == lz4ada.compress_block_host(part, dict=d)
        assert ck == (O.xxh32(payload) if block_checksum else None)
        res.append((stored, payload, seqs))
    assert cck == (O.xxh32(plain) if content_checksum else None)
    out, used = lz4ada.decode_frame_dict_host(frame, d, out_cap=n)
    assert (out, used) == (plain, len(frame))
    return res


# --------------------------------------------------------------- round trips

@pytest.mark.parametrize("name,plain", ID4, ids=[r[0] for r in ID4])
def test_round_trip_id4(name, plain):
    check_frame(lz4ada.compress_frame_host(plain, dict=D64K), plain, D64K)
    check_frame(lz4ada.compress_frame_host(plain, dict=D64K, dict_id=77, **ALL), plain, D64K, dict_id=77, **ALL)


def test_round_trip_id5():
    plain = record(LEN_ID5)
    blocks = check_frame(lz4ada.compress_frame_host(plain, block=256 * KiB, dict=D64K), plain, D64K, block_id=5)
    assert [b[0] for b in blocks] == [False, False]
    assert all(reads_dictionary(b[2]) for b in blocks), "the dictionary lies in front of every block"


def test_liblz4_reads_the_frames_and_the_blocks():
    lz4 = liblz4()
    if lz4 is None:
        pytest.skip("no liblz4 on this system")
    frames = [(plain, lz4ada.compress_frame_host(plain, dict=D64K), 4) for _, plain in ID4]
    frames += [(plain, lz4ada.compress_frame_host(plain, dict=D64K, dict_id=9, **ALL), 4) for _, plain in ID4]
    plain = record(LEN_ID5)
    frames.append((plain, lz4ada.compress_frame_host(plain, block=256 * KiB, dict=D64K, **ALL), 5))
    for plain, frame, block_id in frames:
        blen = BLOCK_LEN[block_id]
        for i, (stored, payload, _) in enumerate(dict_frame_blocks(frame)[4]):
            if not stored:
                part = plain[i * blen:(i + 1) * blen]
                assert lz4_block_using_dict(lz4, payload, len(part), D64K) == part
        if hasattr(lz4, "LZ4F_decompress_usingDict"):
            assert lz4f_using_dict(lz4, frame, len(plain), D64K) == plain


def test_no_dictionary_is_the_plain_statement():
    for _, plain in ID4:
        assert lz4ada.compress_block_host(plain, dict=b"") == lz4ada.compress_block_host(plain)
        for kw in ({}, ALL):
            want = lz4ada.compress_frame_host(plain, **kw)
            assert lz4ada.compress_frame_host(plain, dict=b"", **kw) == want
            cap = lz4ada.compress_frames_bound([len(plain)], **kw)
            buf = ctypes.create_string_buffer(cap)
            opt = lz4ada._compress_options(65536, *(bool(kw),) * 3)
            n = lz4ada._lib.lz4ada_compress_frame_dict_host(plain if plain else None, len(plain), ctypes.byref(opt),
                                                            None, 0, 123, 0, buf, cap)
            assert buf.raw[:n] == want, "dict_len 0 without WRITE_ID: the id is ignored"


# --------------------------------------------------------- dictionary lengths

@pytest.mark.parametrize("dl", DICT_LENGTHS)
def test_dictionary_lengths(dl):
    d = text_dict(dl)
    sizes = []
    for seed in (1, 2, 3):
        plain = pseudo_text(KiB, 100 + seed)
        frame = lz4ada.compress_frame_host(plain, dict=d)
        check_frame(frame, plain, d)
        sizes.append(len(frame))
        if dl <= 3:  # nothing is seeded
            assert frame == lz4ada.compress_frame_host(plain)
        if dl > 65536:  # only the last 65,536 bytes are used
            other = bytes([d[0] ^ 0xFF]) + bytes(x ^ 0x55 for x in d[1:dl - 65536]) + d[dl - 65536:]
            assert len(other) == dl and lz4ada.compress_frame_host(plain, dict=other) == frame
            assert lz4ada.compress_frame_host(plain, dict=d[dl - 65536:]) == frame
    if dl >= 1000:
        assert sum(sizes) < sum(len(lz4ada.compress_frame_host(pseudo_text(KiB, 100 + s))) for s in (1, 2, 3))


# ------------------------------------------------------------------- crafted

@pytest.mark.parametrize("name,d,plain,want", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_crafted(name, d, plain, want):
    comp = lz4ada.compress_block_host(plain, dict=d)
    assert parse_block_dict(comp, plain, d) == want
    frame = lz4ada.compress_frame_host(plain, dict=d)
    blocks = check_frame(frame, plain, d)
    if len(comp) < len(plain):
        assert blocks[0][1] == comp
    else:
        assert blocks[0][0], "not shorter than the record: stored"


def test_offset_bytes_at_the_limit():
    """Byte for byte: token 0x04 (no literal, match length 8), offset ff ff."""
    _, d, plain, _ = next(c for c in CRAFTED if c[0] == "distance65535")
    comp = lz4ada.compress_block_host(plain, dict=d)
    assert comp[:3] == b"\x04\xff\xff" and comp[3] == 0xF0 and comp[4] == 20 - 15 and comp[5:] == plain[8:]
    _, d, plain, _ = next(c for c in CRAFTED if c[0] == "distance65536")
    assert lz4ada.compress_block_host(plain, dict=d) == b"\xf0" + bytes([28 - 15]) + plain


def test_the_dictionary_reaches_every_block():
    plain = record(65537)
    blocks = check_frame(lz4ada.compress_frame_host(plain, dict=D64K), plain, D64K)
    assert [b[0] for b in blocks] == [False, True] and blocks[1][1] == plain[65536:]  # one byte: stored
    d, plain = second_block_from_dictionary()
    assert len(plain) == 131073
    blocks = check_frame(lz4ada.compress_frame_host(plain, dict=d), plain, d)
    assert [b[0] for b in blocks] == [False, False, True]
    lit, off, ml = blocks[1][2][0]
    assert lit == 0 and off > 0 and ml >= 50, "the second block begins with a match into the dictionary"
    assert reads_dictionary(blocks[0][2])


# ------------------------------------------------------------------ WRITE_ID

def raw_frame(plain, opt, d, dict_id, dflags, cap, guard=64):
    buf = ctypes.create_string_buffer(b"\xa5" * (cap + guard), cap + guard)
    n = lz4ada._lib.lz4ada_compress_frame_dict_host(plain if plain else None, len(plain), ctypes.byref(opt),
                                                    d if d else None, len(d), dict_id, dflags, buf, cap)
    return n, buf.raw


@pytest.mark.parametrize("size", [False, True])
def test_write_id_header(size):
    plain = record(300)
    plainf = lz4ada.compress_frame_host(plain, dict=D64K, content_size=size)
    frame = lz4ada.compress_frame_host(plain, dict=D64K, dict_id=0xC0FFEE42, content_size=size)
    flg, _, csize, did, blocks, _, hlen = dict_frame_blocks(frame)
    assert flg & 1 and did == 0xC0FFEE42 and csize == (300 if size else None)
    assert hlen == (19 if size else 11) and len(frame) == len(plainf) + 4
    at = 14 if size else 6
    assert frame[at:at + 4] == b"\x42\xee\xff\xc0"  # after the content size, before HC
    assert frame[hlen:] == plainf[hlen - 4:], "everything behind the header is the frame without an id"
    out, used = lz4ada.decode_frame_dict_host(frame, D64K, out_cap=300)
    assert (out, used) == (plain, len(frame))
    bad = bytearray(frame)
    bad[at] ^= 1  # HC covers the id
    with pytest.raises(lz4ada.LZ4AdaError):
        lz4ada.decode_frame_dict_host(bytes(bad), D64K, out_cap=300)


def test_write_id_bound_and_capacities():
    lens = [0, 13, 300, 70000]
    for kw in ({}, ALL):
        plain_bound = lz4ada.compress_frames_bound(lens, **kw)
        assert lz4ada.compress_frames_bound(lens, dict_id=5, **kw) == plain_bound + 4 * len(lens)
        assert lz4ada.compress_frames_bound(lens, dict=(0x1000, 70000), **kw) == plain_bound
        assert lz4ada.compress_frames_bound(lens, dict=(None, 70000), dict_id=0, **kw) == plain_bound + 4 * len(lens)
    d = text_dict(1000)
    for n in (0, 13, 300):
        plain = record(n)
        for flags in (0, 7):
            opt = lz4ada.CompressOptions(4, flags)
            bound = frame_bound(n, 4, *(bool(flags),) * 3) + 4
            for cap in range(bound):
                got, raw = raw_frame(plain, opt, d, 5, lz4ada.COMP_DICT_WRITE_ID, cap)
                assert got == -5 and raw == b"\xa5" * (cap + 64), cap  # LZ4ADA_TOO_LITTLE_MEMORY, dst untouched
            got, raw = raw_frame(plain, opt, d, 5, lz4ada.COMP_DICT_WRITE_ID, bound)
            assert 0 < got <= bound and raw[bound:] == b"\xa5" * 64
            assert raw[:got] == lz4ada.compress_frame_host(plain, dict=d, dict_id=5, block_checksum=bool(flags),
                                                           content_checksum=bool(flags), content_size=bool(flags))
    with pytest.raises(lz4ada.TooLittleMemory):
        lz4ada.compress_frame_host(record(300), dict=d, dict_id=5,
                                   cap=lz4ada.compress_frames_bound([300], dict_id=5) - 1)


def _device_call(opt, cd, cap=256):
    jobs = lz4ada._compress_jobs([(0, 3)])
    n = ctypes.c_int64()
    st = lz4ada._lib.lz4ada_compress_frames_device_dict(0x1000, 3, jobs, 1, ctypes.byref(opt), ctypes.byref(cd), 0x2000,
                                                        cap, ctypes.byref(n), None)
    lz4ada._check(st, lz4ada._thread_error())


def test_misuse():
    opt = lz4ada.CompressOptions(4, 0)
    buf = ctypes.create_string_buffer(256)
    call = lz4ada._lib.lz4ada_compress_frame_dict_host
    assert call(b"abc", 3, ctypes.byref(opt), b"abcd", -1, 0, 0, buf, 256) == -6
    assert call(b"abc", 3, ctypes.byref(opt), None, 4, 0, 0, buf, 256) == -6
    assert call(b"abc", 3, ctypes.byref(opt), b"abcd", 4, 0, 2, buf, 256) == -6  # an unknown dictionary flag
    assert call(b"abc", 3, ctypes.byref(opt), b"abcd", 4, 0, 0, buf, 256) > 0
    block = lz4ada._lib.lz4ada_compress_block_dict_host
    assert block(b"abc", 3, b"abcd", -1, buf, 256) == -1
    assert block(b"abc", 3, None, 4, buf, 256) == -1
    assert block(b"abc", 3, None, 0, buf, 256) == 4
    jobs = lz4ada._compress_jobs([(0, 3)])
    bad = lz4ada.CompressDict(None, 0, 0, 2)
    assert lz4ada._lib.lz4ada_compress_frames_bound_dict(jobs, 1, ctypes.byref(opt), ctypes.byref(bad)) == -1
    # the options stay closed: the id travels in the dictionary's structure, FLG bit 0 is no option
    for flags in (8, 0x80000000):
        closed = lz4ada.CompressOptions(4, flags)
        ok = lz4ada.CompressDict(0x3000, 4, 0, 0)
        assert lz4ada._lib.lz4ada_compress_frames_bound_dict(jobs, 1, ctypes.byref(closed), ctypes.byref(ok)) == -1
        with pytest.raises(lz4ada.AssertionFailure):
            _device_call(closed, ok)
    # before any launch: no GPU needed
    for cd in (lz4ada.CompressDict(0x3000, -1, 0, 0), lz4ada.CompressDict(None, 4, 0, 0),
               lz4ada.CompressDict(0x3000, 4, 0, 2), lz4ada.CompressDict(0x3000, 4, 0, 0x80000000)):
        with pytest.raises(lz4ada.AssertionFailure):
            _device_call(opt, cd)
    with pytest.raises(lz4ada.TooLittleMemory) as e:  # the bound with the id, without a launch
        lz4ada.compress_frames_device(0x1000, 70005, [(0, 0), (0, 5), (5, 70000)], 0x2000, 10,
                                      dict=(0x3000, 100), dict_id=1)
    assert e.value.bound == sum(frame_bound(n) + 4 for n in (0, 5, 70000))


# --------------------------------------------------------------------- ratio

def ratio_rows():
    """Per row of the recorded sizes: (dictionary, record, count, our payload
    bytes with the dictionary, without, liblz4's with)."""
    with open(os.path.join(GOLDEN, "compress_dict_sizes.json")) as fh:
        gold = json.load(fh)
    rows = []
    for row in gold["rows"]:
        dl, rl, cnt = row["dict"], row["record"], row["count"]
        assert len(row["sizes"]) == cnt
        text = pseudo_text(65536 + rl * cnt, gold["seed"])
        d = text[:65536][-dl:]
        ours = plain = 0
        for i in range(cnt):
            rec = text[65536 + i * rl:65536 + (i + 1) * rl]
            ours += sum(len(b[1]) for b in dict_frame_blocks(lz4ada.compress_frame_host(rec, dict=d))[4])
            plain += sum(len(b[1]) for b in dict_frame_blocks(lz4ada.compress_frame_host(rec))[4])
        rows.append((dl, rl, cnt, ours, plain, sum(row["sizes"])))
    return rows


def test_ratio_against_liblz4():
    """Payload bytes against liblz4's LZ4_loadDict + LZ4_compress_fast_continue:
    at most 1.15 per row, and 64 x 1 KiB with the 65,536-byte dictionary at
    most 0.70 of the same records without it.  The rule of DESIGN.md §18 gives
    1.106, 1.102, 1.081, 1.012, 0.995 and 0.978, and 0.579."""
    rows = ratio_rows()
    for dl, rl, cnt, ours, plain, lib in rows:
        print(f"dict {dl}, {cnt} x {rl}: {ours} bytes, without {plain}, liblz4 {lib}: "
              f"{ours / lib:.3f}, {ours / plain:.3f}")
    for dl, rl, cnt, ours, plain, lib in rows:
        assert ours <= 1.15 * lib, (dl, rl)
    dl, rl, cnt, ours, plain, _ = rows[1]
    assert (dl, rl, cnt) == (65536, 1024, 64) and ours <= 0.70 * plain
    assert [r[3] for r in rows] == RECORDED, "the statement is deterministic: it has departed from the rule"
