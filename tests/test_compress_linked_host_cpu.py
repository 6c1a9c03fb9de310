"""The serial statement of a frame of linked blocks:
lz4ada_compress_frame_linked_host, which the device call is tested against byte
for byte (tests/test_gpu_compress_linked.py).  Block 0 against the unlinked
frame's; a strict sequence parser over every block with the frame's earlier
output as the decoded prefix; crafted records at the boundary between a block
and the record in front of it; the dictionary in front of block 0 alone; every
capacity below the bound; the sizes against liblz4's recorded ones
(tests/golden/compress_linked_sizes.json).  The record comes back only through
decoders with the specification's semantics: lz4ada_decode_frame_dict_host and,
where present, liblz4 -- never the oracle (quirk D1).  No GPU."""
import ctypes
import ctypes.util
import itertools
import json
import os

import pytest

import _oracle as O
import lz4ada
from _compress_cases import BLOCK_LEN, KiB, frame_bound, id4_records, noise, pseudo_text, record
from _compress_dict_cases import dict_frame_blocks, reads_dictionary, text_dict
from _compress_linked_cases import (B, LENGTHS, RECORDED, block_history, crafted, dict_only_record,
                                    parse_block_linked, size_rows, stored_then_compressible)
from conftest import GOLDEN

D64K = text_dict(65536)
CRAFTED = crafted()
ALL = dict(block_checksum=True, content_checksum=True, content_size=True)


def liblz4():
    name = ctypes.util.find_library("lz4")
    return ctypes.CDLL(name) if name else None


def lz4f_decode(lz4, frame, n, d=b""):
    """The frame through liblz4's frame decoder, with the dictionary where it has the call."""
    size_t = ctypes.c_size_t
    lz4.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lz4.LZ4F_createDecompressionContext.restype = size_t
    lz4.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    lz4.LZ4F_isError.argtypes = [size_t]
    if d:
        call = lz4.LZ4F_decompress_usingDict
        call.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(size_t), ctypes.c_void_p,
                         ctypes.POINTER(size_t), ctypes.c_char_p, size_t, ctypes.c_void_p]
        extra = (d, len(d), None)
    else:
        call = lz4.LZ4F_decompress
        call.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(size_t), ctypes.c_void_p,
                         ctypes.POINTER(size_t), ctypes.c_void_p]
        extra = (None,)
    call.restype = size_t
    ctx = ctypes.c_void_p()
    assert not lz4.LZ4F_isError(lz4.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    try:
        dst = ctypes.create_string_buffer(n + 1)
        src = ctypes.create_string_buffer(frame, len(frame))
        got, used, hint = 0, 0, 1
        while used < len(frame):
            dn, sn = size_t(n + 1 - got), size_t(len(frame) - used)
            hint = call(ctx, ctypes.byref(dst, got), ctypes.byref(dn), ctypes.byref(src, used), ctypes.byref(sn),
                        *extra)
            assert not lz4.LZ4F_isError(hint), "liblz4 rejects the frame"
            assert dn.value or sn.value, "liblz4 makes no progress"
            got, used = got + dn.value, used + sn.value
        assert hint == 0, "liblz4 expects more input"
        return dst.raw[:got]
    finally:
        lz4.LZ4F_freeDecompressionContext(ctx)


def check_frame(frame, plain, d=b"", block_id=4, dict_id=None, block_checksum=False, content_checksum=False,
                content_size=False):
    """The layout with B.Indep clear, every block's sequences with the frame's
    earlier output in front of it, every block's bytes as the block statement
    gives them for that history, and the record back from the host decoder ->
    [(stored, payload, sequences or None)]."""
    n, blen = len(plain), BLOCK_LEN[block_id]
    extra = 4 if dict_id is not None else 0
    assert len(frame) <= frame_bound(n, block_id, block_checksum, content_checksum, content_size) + extra
    flg, bd, size, did, blocks, cck, _ = dict_frame_blocks(frame)
    assert flg == (0x40 | (0x10 if block_checksum else 0) | (8 if content_size else 0) | (4 if content_checksum else 0)
                   | (1 if dict_id is not None else 0)), "version 01, B.Indep clear"
    assert (bd, size, did) == (block_id << 4, n if content_size else None, dict_id)
    assert len(blocks) == -(-n // blen)
    res = []
    for i, (stored, payload, ck) in enumerate(blocks):
        part, hist = plain[i * blen:(i + 1) * blen], block_history(plain, i, blen, d)
        seqs = None
        if stored:
            assert payload == part
            assert len(lz4ada.compress_block_host(part, len(part) - 1, dict=hist)) == 0, "stored, yet it would shrink"
        else:
            assert len(payload) < len(part), "a block is stored whenever its compressed form is not shorter"
            seqs = parse_block_linked(payload, plain, i, blen, d)
            assert payload == lz4ada.compress_block_host(part, dict=hist), "the existing function with another D"
        assert ck == (O.xxh32(payload) if block_checksum else None)
        res.append((stored, payload, seqs))
    assert cck == (O.xxh32(plain) if content_checksum else None)
    out, used = lz4ada.decode_frame_dict_host(frame, d, out_cap=n)
    assert (out, used) == (plain, len(frame))
    return res


def unlinked_twin(frame, kw, plain, d=b"", dict_id=None):
    """The unlinked frame of the same record and options, and both frames' headers' lengths."""
    twin = lz4ada.compress_frame_host(plain, dict=d, dict_id=dict_id, **kw)
    return twin, dict_frame_blocks(frame)[6], dict_frame_blocks(twin)[6]


# ------------------------------------------------------------------- block 0

@pytest.mark.parametrize("n", LENGTHS)
def test_block0_is_the_unlinked_frames(n):
    """With and without a dictionary: block 0 byte for byte, and the header but for FLG and HC."""
    plain = pseudo_text(n, n + 1)
    for d, dict_id in ((b"", None), (D64K, None), (D64K, 9)):
        frame = lz4ada.compress_frame_host(plain, dict=d, dict_id=dict_id, linked=True)
        twin, hlen, tlen = unlinked_twin(frame, {}, plain, d, dict_id)
        assert hlen == tlen and frame[4] == twin[4] ^ 0x20
        assert frame[:4] == twin[:4] and frame[5:hlen - 1] == twin[5:hlen - 1]
        b0, t0 = dict_frame_blocks(frame)[4][0], dict_frame_blocks(twin)[4][0]
        assert b0 == t0
        size = 4 + len(b0[1])
        assert frame[hlen:hlen + size] == twin[hlen:hlen + size]
        assert len(frame) <= len(twin)
        check_frame(frame, plain, d, dict_id=dict_id)


def test_one_block_is_the_unlinked_frame_but_for_the_bit():
    for _, plain in id4_records():
        if len(plain) > B:
            continue
        for d, kw in ((b"", {}), (b"", ALL), (D64K, ALL)):
            frame = lz4ada.compress_frame_host(plain, dict=d, linked=True, **kw)
            twin, hlen, _ = unlinked_twin(frame, kw, plain, d)
            assert frame[4] == twin[4] ^ 0x20 and frame[:4] == twin[:4]
            assert frame[5:hlen - 1] == twin[5:hlen - 1] and frame[hlen:] == twin[hlen:]
            check_frame(frame, plain, d, **kw)


# ----------------------------------------------------------- flags and parser

FLAG_SETS = [dict(zip(("block_checksum", "content_checksum", "content_size"), bits))
             for bits in itertools.product((False, True), repeat=3)]


@pytest.mark.parametrize("kw", FLAG_SETS, ids=["".join("bcs"[i] if v else "-" for i, v in enumerate(k.values()))
                                               for k in FLAG_SETS])
def test_every_flag_combination(kw):
    plain = pseudo_text(2 * B + 1, 21)
    blocks = check_frame(lz4ada.compress_frame_host(plain, linked=True, **kw), plain, **kw)
    assert [b[0] for b in blocks] == [False, False, True]
    assert reads_dictionary(blocks[1][2]), "block 1 reads the record in front of it"
    check_frame(lz4ada.compress_frame_host(plain, dict=D64K, dict_id=77, linked=True, **kw), plain, D64K, dict_id=77,
                **kw)


@pytest.mark.parametrize("n", LENGTHS)
def test_record_lengths(n):
    plain = pseudo_text(n, n + 1)
    blocks = check_frame(lz4ada.compress_frame_host(plain, linked=True), plain)
    last = n - B * (len(blocks) - 1)
    assert blocks[-1][0] == (last < 13), "a last block under 13 bytes is a literal run, and stored"
    plain = record(n, "zeros")
    check_frame(lz4ada.compress_frame_host(plain, linked=True, **ALL), plain, **ALL)


# ------------------------------------------------------------------- crafted

@pytest.mark.parametrize("name,plain,want", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_crafted(name, plain, want):
    comp = lz4ada.compress_block_host(plain[B:], dict=plain[:B])
    assert parse_block_linked(comp, plain, 1, B) == want
    blocks = check_frame(lz4ada.compress_frame_host(plain, linked=True), plain)
    assert len(blocks) == 2
    if len(comp) < len(plain) - B:
        assert blocks[1][1] == comp
    else:
        assert blocks[1][0], "not shorter than the block: stored"


def test_offset_bytes_at_the_limit():
    """Byte for byte: token 0x04 (no literal, match length 8), offset ff ff."""
    plain = next(c[1] for c in CRAFTED if c[0] == "distance65535")
    comp = dict_frame_blocks(lz4ada.compress_frame_host(plain, linked=True))[4][1][1]
    assert comp[:3] == b"\x04\xff\xff" and comp[3] == 0xF0 and comp[4] == 20 - 15 and comp[5:] == plain[B + 8:]
    plain = next(c[1] for c in CRAFTED if c[0] == "distance65536")
    stored, payload, _ = dict_frame_blocks(lz4ada.compress_frame_host(plain, linked=True))[4][1]
    assert stored and payload == plain[B:], "one literal run of 28 bytes is not shorter: stored"


def test_a_stored_block_is_history_too():
    plain = stored_then_compressible()
    blocks = check_frame(lz4ada.compress_frame_host(plain, linked=True, **ALL), plain, **ALL)
    assert [b[0] for b in blocks] == [False, True, False]
    lit, off, ml = blocks[2][2][0]
    assert lit < 64 and off == 1000 and lit + ml == 1000, "block 2 begins with the noise of the stored block"
    twin = dict_frame_blocks(lz4ada.compress_frame_host(plain, **ALL))[4]
    assert len(blocks[2][1]) + 900 < len(twin[2][1])


def test_larger_blocks():
    """Block id 5: 262,144 + 37,856 bytes, the second block's window the last 64 KiB of the first."""
    plain = record(300000)
    blocks = check_frame(lz4ada.compress_frame_host(plain, block=256 * KiB, linked=True, **ALL), plain, block_id=5,
                         **ALL)
    assert [b[0] for b in blocks] == [False, False] and reads_dictionary(blocks[1][2])
    twin = dict_frame_blocks(lz4ada.compress_frame_host(plain, block=256 * KiB, **ALL))[4]
    assert blocks[0][1] == twin[0][1] and len(blocks[1][1]) < len(twin[1][1])
    # a repeat 65,535 back in block 1 across the 256 KiB boundary, and one 65,536 back
    S = bytes(x or 1 for x in noise(8, 71))
    for dist, found in ((65535, True), (65536, False)):
        b0 = bytearray(4 * B)
        b0[4 * B - dist:4 * B - dist + 8] = S
        plain = bytes(b0) + S + bytes(x or 1 for x in noise(20, 72))
        blocks = check_frame(lz4ada.compress_frame_host(plain, block=256 * KiB, linked=True), plain, block_id=5)
        assert blocks[1][0] != found and (not found or blocks[1][2] == [(0, 65535, 8), (20, 0, 0)])


# ---------------------------------------------------------------- dictionary

def test_the_dictionary_lies_in_front_of_block_0_alone():
    plain = dict_only_record(D64K)
    frame = lz4ada.compress_frame_host(plain, dict=D64K, linked=True)
    blocks = check_frame(frame, plain, D64K)
    assert [b[0] for b in blocks] == [False, False, True]
    assert reads_dictionary(blocks[0][2]), "block 0 reads the dictionary"
    # the unlinked frame begins block 1 with a match into the dictionary ...
    twin = dict_frame_blocks(lz4ada.compress_frame_host(plain, dict=D64K))[4]
    assert blocks[0][1] == twin[0][1]
    # ... the linked one leaves those 100 bytes to what the record offers: block 1
    # parses against the record alone (check_frame), and few of them are matched
    at = matched = 0
    for lit, off, ml in blocks[1][2]:
        at += lit
        if at < 100:
            matched += min(ml, 100 - at)
        at += ml
    assert matched < 50
    # without the dictionary the frame does not come back
    try:
        out, _ = lz4ada.decode_frame_dict_host(frame, b"", out_cap=len(plain))
    except lz4ada.LZ4AdaError:
        out = None
    assert out != plain
    # a dictionary longer than the window: only its last 65,536 bytes are read
    long = text_dict(100000)
    assert lz4ada.compress_frame_host(plain, dict=long, linked=True) == \
           lz4ada.compress_frame_host(plain, dict=long[-65536:], linked=True)


def test_liblz4_reads_the_frames():
    lz4 = liblz4()
    if lz4 is None:
        pytest.skip("no liblz4 on this system")
    cases = [(plain, b"", 65536) for _, plain, _ in CRAFTED]
    cases += [(pseudo_text(n, n + 1), b"", 65536) for n in LENGTHS]
    cases += [(stored_then_compressible(), b"", 65536), (record(300000), b"", 256 * KiB)]
    if hasattr(lz4, "LZ4F_decompress_usingDict"):
        cases += [(dict_only_record(D64K), D64K, 65536), (record(300000), D64K, 256 * KiB)]
    for plain, d, block in cases:
        frame = lz4ada.compress_frame_host(plain, block=block, dict=d, linked=True, **ALL)
        assert lz4f_decode(lz4, frame, len(plain), d) == plain


# ------------------------------------------------------------------ capacity

def raw_frame(plain, opt, d, dict_id, dflags, cap, guard=64):
    buf = ctypes.create_string_buffer(b"\xa5" * (cap + guard), cap + guard)
    n = lz4ada._lib.lz4ada_compress_frame_linked_host(plain if plain else None, len(plain), ctypes.byref(opt),
                                                      d if d else None, len(d), dict_id, dflags, buf, cap)
    return n, buf.raw


def test_every_capacity_below_the_bound():
    for n in (0, 13, 300):
        plain = record(n)
        for flags, d, dflags in ((0, b"", 0), (7, b"", 0), (7, text_dict(1000), lz4ada.COMP_DICT_WRITE_ID)):
            opt = lz4ada.CompressOptions(4, flags)
            bound = frame_bound(n, 4, *(bool(flags),) * 3) + (4 if dflags else 0)
            for cap in range(bound):
                got, raw = raw_frame(plain, opt, d, 5, dflags, cap)
                assert got == -5 and raw == b"\xa5" * (cap + 64), cap  # LZ4ADA_TOO_LITTLE_MEMORY, dst untouched
            got, raw = raw_frame(plain, opt, d, 5, dflags, bound)
            assert 0 < got <= bound and raw[bound:] == b"\xa5" * 64
    # two blocks: every capacity, the destination one buffer that stays canary
    plain = pseudo_text(B + 13, 31)
    opt = lz4ada.CompressOptions(4, 7)
    bound = frame_bound(B + 13, 4, True, True, True)
    assert lz4ada.compress_frames_bound([B + 13], **ALL) == bound
    canary = b"\xa5" * (bound + 64)
    buf = ctypes.create_string_buffer(canary, bound + 64)
    call = lz4ada._lib.lz4ada_compress_frame_linked_host
    for cap in range(bound):
        assert call(plain, len(plain), ctypes.byref(opt), None, 0, 0, 0, buf, cap) == -5, cap
    assert buf.raw == canary
    got = call(plain, len(plain), ctypes.byref(opt), None, 0, 0, 0, buf, bound)
    assert 0 < got < bound and buf.raw[bound:] == canary[bound:]
    assert buf.raw[:got] == lz4ada.compress_frame_host(plain, linked=True, **ALL)
    with pytest.raises(lz4ada.TooLittleMemory):
        lz4ada.compress_frame_host(plain, linked=True, cap=lz4ada.compress_frames_bound([B + 13]) - 1)


def test_misuse():
    opt = lz4ada.CompressOptions(4, 0)
    buf = ctypes.create_string_buffer(256)
    call = lz4ada._lib.lz4ada_compress_frame_linked_host
    assert call(b"abc", 3, ctypes.byref(opt), b"abcd", -1, 0, 0, buf, 256) == -6
    assert call(b"abc", 3, ctypes.byref(opt), None, 4, 0, 0, buf, 256) == -6
    assert call(b"abc", 3, ctypes.byref(opt), b"abcd", 4, 0, 2, buf, 256) == -6  # an unknown dictionary flag
    assert call(None, 3, ctypes.byref(opt), None, 0, 0, 0, buf, 256) == -6
    assert call(b"abc", 3, ctypes.byref(opt), None, 0, 0, 0, buf, 256) > 0
    assert call(b"abc", 3, None, None, 0, 0, 0, buf, 256) > 0
    # the options stay closed: linking is an entry, not a flag
    for flags in (8, 0x20, 0x80000000):
        closed = lz4ada.CompressOptions(4, flags)
        assert call(b"abc", 3, ctypes.byref(closed), None, 0, 0, 0, buf, 256) == -6
    assert lz4ada._lib.lz4ada_abi_version() == 1


def _device_call(opt, cd, cap=256, d_in=0x1000, d_out=0x2000, span=(0, 3)):
    jobs = lz4ada._compress_jobs([span])
    n = ctypes.c_int64()
    st = lz4ada._lib.lz4ada_compress_frames_device_linked(d_in, 3, jobs, 1, ctypes.byref(opt),
                                                          ctypes.byref(cd) if cd is not None else None, d_out, cap,
                                                          ctypes.byref(n), None)
    lz4ada._check(st, lz4ada._thread_error())


def test_device_misuse_needs_no_gpu():
    """LZ4ADA_ASSERTION_ERROR and the bound come before any launch."""
    opt = lz4ada.CompressOptions(4, 0)
    for flags in (8, 0x20, 0x80000000):
        with pytest.raises(lz4ada.AssertionFailure):
            _device_call(lz4ada.CompressOptions(4, flags), None)
    for block_id in (3, 8):
        with pytest.raises(lz4ada.AssertionFailure):
            _device_call(lz4ada.CompressOptions(block_id, 0), None)
    for cd in (lz4ada.CompressDict(0x3000, -1, 0, 0), lz4ada.CompressDict(None, 4, 0, 0),
               lz4ada.CompressDict(0x3000, 4, 0, 2), lz4ada.CompressDict(0x3000, 4, 0, 0x80000000)):
        with pytest.raises(lz4ada.AssertionFailure):
            _device_call(opt, cd)
    with pytest.raises(lz4ada.AssertionFailure):
        _device_call(opt, None, span=(1, 3))  # outside the input
    with pytest.raises(lz4ada.AssertionFailure):
        _device_call(opt, None, d_in=None)
    with pytest.raises(lz4ada.AssertionFailure):
        _device_call(opt, None, d_out=None)
    for kw, extra in ((dict(), 0), (dict(dict=(0x3000, 100), dict_id=1), 4)):
        with pytest.raises(lz4ada.TooLittleMemory) as e:
            lz4ada.compress_frames_device(0x1000, 200005, [(0, 0), (0, 5), (5, 200000)], 0x2000, 10, linked=True, **kw)
        assert e.value.bound == sum(frame_bound(n) + extra for n in (0, 5, 200000))


# --------------------------------------------------------------------- sizes

def size_figures():
    with open(os.path.join(GOLDEN, "compress_linked_sizes.json")) as fh:
        gold = json.load(fh)
    rows = []
    for (name, rec, blen), row in zip(size_rows(), gold["rows"]):
        assert (row["name"], row["record"], row["block"]) == (name, len(rec), blen)
        assert len(row["liblz4_linked"]) == -(-len(rec) // blen)
        ours = sum(len(b[1]) for b in dict_frame_blocks(lz4ada.compress_frame_host(rec, block=blen, linked=True))[4])
        plain = sum(len(b[1]) for b in dict_frame_blocks(lz4ada.compress_frame_host(rec, block=blen))[4])
        rows.append((name, ours, plain, sum(row["liblz4_linked"]), row))
    assert len(rows) == len(gold["rows"]) == 5
    return rows


def test_sizes_against_liblz4():
    """Payload bytes, linked: the statement's recorded figures exactly, never
    more than the same record in independent blocks, and at most 1.10 of
    liblz4's LZ4_compress_fast_continue over the same blocks (DESIGN.md §17's
    cap).  The rule gives 1.009, 1.010, 1.012, 1.004 and 0.789."""
    rows = size_figures()
    for name, ours, plain, lib, _ in rows:
        print(f"{name}: linked {ours}, independent {plain}, liblz4 linked {lib}: {ours / plain:.3f}, {ours / lib:.3f}")
    for name, ours, plain, lib, row in rows:
        assert (ours, plain) == (row["linked"], row["independent"]), name
        assert ours <= plain, name
        assert ours <= 1.10 * lib, name
    assert [r[1] for r in rows] == RECORDED, "the statement is deterministic: it has departed from the rule"
