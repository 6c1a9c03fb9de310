"""lz4ada_decode_frame_dict_host: one modern frame decoded
against a dictionary on the host, the LZ4 specification's semantics.  Checked
against the committed liblz4 fixtures (tests/golden/lz4f_dict, written by
make_lz4_dict_fixtures.py: frames from LZ4F_compressFrame_usingCDict, the
manifest holds each plaintext's length and XXH32) and against hand-built
blocks whose decoded bytes _lz4build computes.  No GPU."""
import json
import os

import pytest
import xxhash

import _lz4build
import lz4ada
import lz4frame
from conftest import GOLDEN

DICT_DIR = os.path.join(GOLDEN, "lz4f_dict")
KiB = 1024


def _read(name):
    with open(os.path.join(DICT_DIR, name), "rb") as fh:
        return fh.read()


with open(os.path.join(DICT_DIR, "manifest.json")) as _fh:
    MANIFEST = json.load(_fh)
DICTS = {k: _read(v["file"]) for k, v in MANIFEST["dicts"].items()}
FRAMES = MANIFEST["frames"]


def test_manifest_covers_the_shapes():
    assert len(FRAMES) >= 40
    assert {len(d) for d in DICTS.values()} == {20480, 100000}
    for key in ("linked", "content_checksum", "block_checksum", "content_size"):
        assert {f[key] for f in FRAMES} == {False, True}, key
    assert {f["dict_id"] is None for f in FRAMES} == {False, True}
    multi = [f for f in FRAMES if f["size"] > 64 * KiB]
    assert sorted(f["linked"] for f in multi) == [False, True]


@pytest.mark.parametrize("f", FRAMES, ids=[f["file"] for f in FRAMES])
def test_fixture_frame(f):
    frame = _read(f["file"])
    out, used = lz4ada.decode_frame_dict_host(frame, DICTS[f["dict"]])
    assert used == len(frame) == f["frame_len"]
    assert len(out) == f["size"] and xxhash.xxh32(out).intdigest() == f["xxh32"]


def first_dict_read(frame, dict_used):
    """Index into the dictionary's used tail of the first byte a match of the
    frame's first block reads there."""
    flg = frame[4]
    pos = 4 + 2 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0) + 1
    n = int.from_bytes(frame[pos:pos + 4], "little")
    assert not n & 0x80000000
    payload, p, o = frame[pos + 4:pos + 4 + n], 0, 0
    while p < len(payload):
        tok = payload[p]
        p += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                lit += payload[p]
                p += 1
                if payload[p - 1] != 255:
                    break
        p += lit
        o += lit
        if p >= len(payload):
            break
        off = payload[p] | (payload[p + 1] << 8)
        p += 2
        ml = tok & 15
        if ml == 15:
            while True:
                ml += payload[p]
                p += 1
                if payload[p - 1] != 255:
                    break
        if off > o:
            return dict_used - (off - o)
        o += ml + 4
    raise AssertionError("the block reads no dictionary byte")


def test_wrong_dictionary_is_a_checksum_error():
    f = next(f for f in FRAMES if f["content_checksum"] and not f["block_checksum"])
    frame, d = _read(f["file"]), bytearray(DICTS[f["dict"]])
    used = min(len(d), 65536)
    d[len(d) - used + first_dict_read(frame, used)] ^= 0x55
    with pytest.raises(lz4ada.ChecksumError):
        lz4ada.decode_frame_dict_host(frame, bytes(d))


def test_no_dictionary_is_data_corruption():
    for f in FRAMES[:6]:
        with pytest.raises(lz4ada.DataCorruption):
            lz4ada.decode_frame_dict_host(_read(f["file"]), b"")


def test_out_cap_one_short():
    f = FRAMES[5]
    frame, d = _read(f["file"]), DICTS[f["dict"]]
    out, _ = lz4ada.decode_frame_dict_host(frame, d, out_cap=f["size"])
    assert len(out) == f["size"]
    with pytest.raises(lz4ada.TooLittleMemory):
        lz4ada.decode_frame_dict_host(frame, d, out_cap=f["size"] - 1)


def one_block_frame(seqs, final, dictionary, **kw):
    """A frame of one hand-built block and its plaintext under the dictionary:
    the block is encoded over dictionary + block, as one LZ4 history."""
    comp, _ = _lz4build.encode(seqs, final)  # the payload; its own replay knows no dictionary
    # decoded bytes: replay the sequences over the dictionary's tail
    hist = bytearray(dictionary[-65536:])
    base = len(hist)
    for lits, off, ml in seqs:
        hist += lits
        assert 0 < off <= len(hist)
        for _ in range(ml):
            hist.append(hist[-off])
    hist += final or b""
    plain = bytes(hist[base:])
    frame, _ = lz4frame.build_frame([(comp, plain, False)], 64 * KiB, **kw)
    return frame, plain


def test_block_opens_with_a_match_at_position_0():
    d = bytes(range(256)) * 3
    frame, plain = one_block_frame([(b"", 100, 40), (b"xy", 7, 9)], b"tail!", d, content_cksum=True)
    assert plain[:40] == d[-100:-60]
    out, used = lz4ada.decode_frame_dict_host(frame, d)
    assert out == plain and used == len(frame)


@pytest.mark.parametrize("off", range(1, 16))
def test_period_pattern_crosses_from_the_dictionary(off):
    d = bytes((37 * i + 11) & 255 for i in range(1000))
    frame, plain = one_block_frame([(b"", off, off + 23)], b"12345", d, content_cksum=True)
    assert plain[:off + 23] == (d[-off:] * 40)[:off + 23]
    out, _ = lz4ada.decode_frame_dict_host(frame, d)
    assert out == plain


@pytest.mark.parametrize("dict_len", [1, 5, 300, 65535, 65536, 70000])
def test_reach_of_the_dictionary(dict_len):
    """A match may reach the dictionary's first used byte and no further (an
    offset is at most 65,535, so of 65,536 used bytes the first is out of reach)."""
    d = bytes((i * 7 + (i >> 8) + 1) & 255 for i in range(dict_len))
    reach = min(dict_len, 65535)
    frame, plain = one_block_frame([(b"", reach, 4)], b"end..", d, content_cksum=True)
    out, _ = lz4ada.decode_frame_dict_host(frame, d)
    assert out == plain and plain[:4] == (d[-reach:] * 4)[:4]
    if reach + 1 <= 65535:
        comp, _ = _lz4build.encode([(b"", reach + 1, 4)], b"end..")
        frame, _ = lz4frame.build_frame([(comp, b"", False)], 64 * KiB)
        with pytest.raises(lz4ada.DataCorruption):
            lz4ada.decode_frame_dict_host(frame, d)


def test_linked_frame_reads_dictionary_then_earlier_blocks():
    d = bytes((i * 131 + 7) & 255 for i in range(30000))
    blocks = lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, 5, 0, 0, lens=[65536, 65536, 1000], hist=d)
    recs = [(c, r, False) for c, r in blocks]
    frame, plain = lz4frame.build_frame(recs, 64 * KiB, indep=False, block_cksum=True, content_cksum=True,
                                        with_content_size=True, dict_id=77)
    out, used = lz4ada.decode_frame_dict_host(frame, d)
    assert out == plain and used == len(frame)
    with pytest.raises(lz4ada.ChecksumError):
        lz4ada.decode_frame_dict_host(frame, bytes(b ^ 0x55 for b in d))


def test_independent_blocks_each_read_the_dictionary():
    d = bytes((i * 29 + 3) & 255 for i in range(4096))
    blocks = [lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, 40 + i, 0, 0, lens=[3000], hist=d)[0] for i in range(3)]
    frame, plain = lz4frame.build_frame([(c, r, False) for c, r in blocks], 64 * KiB, content_cksum=True)
    out, _ = lz4ada.decode_frame_dict_host(frame, d)
    assert out == plain
    # the same payloads as a linked frame: blocks 2 and 3 would read block 1 instead
    linked, _ = lz4frame.build_frame([(c, r, False) for c, r in blocks], 64 * KiB, indep=False, content_cksum=True)
    with pytest.raises(lz4ada.LZ4AdaError):
        lz4ada.decode_frame_dict_host(linked, d)


def test_stored_blocks_and_statuses():
    d = b"dictionary " * 50
    comp, raw = lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, 9, 0, 0, lens=[500], hist=d)[0]
    frame, plain = lz4frame.build_frame([(b"stored bytes", b"stored bytes", True), (comp, raw, False)], 64 * KiB,
                                        block_cksum=True, content_cksum=True, with_content_size=True)
    out, _ = lz4ada.decode_frame_dict_host(frame, d)
    assert out == plain
    bad = bytearray(frame)
    bad[-1] ^= 1  # the content checksum
    with pytest.raises(lz4ada.ChecksumError):
        lz4ada.decode_frame_dict_host(bytes(bad), d)
    bad = bytearray(frame)
    bad[6] ^= 1  # the content size, and with it the header checksum
    with pytest.raises(lz4ada.LZ4AdaError):
        lz4ada.decode_frame_dict_host(bytes(bad), d)
    with pytest.raises(lz4ada.DataCorruption):
        lz4ada.decode_frame_dict_host(frame[:-5], d)
    with pytest.raises(lz4ada.NotSupported):
        lz4ada.decode_frame_dict_host(b"\x02\x21\x4c\x18" + b"\x00" * 8, d)
    with pytest.raises(lz4ada.NotSupported):
        lz4ada.decode_frame_dict_host(b"\x50\x2a\x4d\x18\x00\x00\x00\x00", d)
    assert "dictionary decode" in lz4ada._thread_error()
