"""The frame walk the device index runs (csrc/lz4ada_frame_walk.h), on the
host through lz4ada_frame_walk_host (no GPU needed), pinned to the two host
routines that own the rules: it accepts exactly the frames that
lz4ada_stream_index lists as batchable and lz4ada_frame_index indexes, with
the same info and descriptors byte for byte, and where the host has a reason
for a frame it gives the same one -- over the golden and error vectors, the
liblz4 fixtures, frames built across every header option, every truncation
of three frames and every bit flip in the first 20 bytes of two."""
import ctypes
import itertools
import os
import random
import struct

import pytest
import xxhash

from conftest import GOLDEN, VECTORS

import lz4ada
import lz4frame


def host_view(data):
    """(listed, reason, frame_index status, info, descs) of the frame at data[0:]."""
    n = ctypes.c_int64()
    entries = (lz4ada.StreamEntry * 1)()
    # one entry of room: a later frame only ends the call, the first is listed
    lz4ada._lib.lz4ada_stream_index(lz4ada._addr(data), len(data), entries, 1, ctypes.byref(n))
    info = lz4ada.FrameInfo()
    st = lz4ada._lib.lz4ada_frame_index(lz4ada._addr(data), len(data), ctypes.byref(info), None, 0)
    descs = None
    if st == 0:
        descs = (lz4ada.BlockDesc * max(info.nblocks, 1))()
        assert lz4ada._lib.lz4ada_frame_index(lz4ada._addr(data), len(data), ctypes.byref(info), descs,
                                              info.nblocks) == 0
    return n.value >= 1, entries[0].batchable, st, info, descs


def check(data):
    """The required agreement for one input; returns the walk's verdict."""
    listed, reason, st, info, descs = host_view(data)
    v, winfo, wdescs = lz4ada.frame_walk_host(data)
    assert (v == lz4ada.DEVFRAME_OK) == (listed and reason == lz4ada.BATCH_OK and st == 0)
    if listed:  # the host has a reason
        assert st == 0 and v == reason
        assert bytes(winfo) == bytes(info)
        assert bytes(wdescs)[:32 * info.nblocks] == bytes(descs)[:32 * info.nblocks]
    else:
        assert v == lz4ada.BATCH_NOT_INDEXED
    return v


# ------------------------------------------------------------------ frames

def stored(raw):
    return raw, raw, True


def compressed(n, seed):
    comp, raw = lz4ada.gen_block(lz4ada.GEN_MIXED, seed, n)
    return comp, raw, False


def small_blocks(rng, sizes):
    """Compressed and stored blocks in turn."""
    return [stored(rng.randbytes(n)) if k % 2 else compressed(n, 40 + k) for k, n in enumerate(sizes)]


def with_dict_id(frame, dict_id=0x11223344):
    """The frame with FLG.DictID set and the id after the content size."""
    flg = frame[4] | 1
    dlen = 2 + (8 if flg & 8 else 0)
    desc = bytes([flg]) + frame[5:4 + dlen] + struct.pack("<I", dict_id)
    hc = (xxhash.xxh32(desc).intdigest() >> 8) & 0xFF
    return frame[:4] + desc + bytes([hc]) + frame[4 + dlen + 1:]


def skippable(payload, nibble=7):
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload)) + payload


def legacy(blocks):
    return struct.pack("<I", 0x184C2102) + b"".join(struct.pack("<I", len(c)) + c for c, _, _ in blocks)


def built_frames():
    """name -> bytes: every header option, and one frame per reason."""
    rng = random.Random(515)
    out = {}
    for bck, cck, size, did, bmax in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (64 << 10, 4 << 20)):
        f, _ = lz4frame.build_frame(small_blocks(rng, [300, 17, 1, 4096]), bmax, block_cksum=bool(bck),
                                    content_cksum=bool(cck), with_content_size=bool(size))
        out[f"opt_b{bck}c{cck}s{size}d{did}_{bmax >> 10}k"] = with_dict_id(f) if did else f
    out["empty"] = lz4frame.build_frame([], 64 << 10, content_cksum=True)[0]
    lg = legacy([compressed(500, 1), compressed(700, 2)])
    out["legacy"] = lg
    out["legacy_then_magic"] = lg + out["opt_b1c1s1d0_64k"]
    out["legacy_then_skippable"] = lg + skippable(b"xyz")
    out["skippable"] = skippable(rng.randbytes(33))
    out["skippable_then_frame"] = skippable(b"") + out["opt_b0c1s0d1_64k"]
    out["skippable_cut"] = skippable(rng.randbytes(33))[:-1]
    out["linked"] = lz4frame.build_frame(small_blocks(rng, [300, 200]), 64 << 10, indep=False,
                                         content_cksum=True)[0]
    # few_large_blocks: one stored block of 600 KiB
    out["large_block"] = lz4frame.build_frame([stored(rng.randbytes(600 << 10))], 4 << 20)[0]
    # 25 blocks, one of them 600 KiB: over the lone-block rule's count, so batchable
    out["large_block_many"] = lz4frame.build_frame(
        [stored(rng.randbytes(600 << 10))] + [stored(rng.randbytes(5))] * 24, 4 << 20)[0]
    # a legacy block that may decode to over 4 MiB (255 bytes per payload byte)
    comp, raw = lz4ada.gen_block(lz4ada.GEN_LITERAL, 5, 20000)
    assert 255 * len(comp) + 64 > 4 << 20
    out["legacy_big_slot"] = legacy([(comp, raw, False)])
    # a size word over the block maximum, with and without the bits quirk Q2 masks
    hdr = lz4frame.header(64 << 10)
    out["word_over_max"] = hdr + struct.pack("<I", 65537) + bytes(65537) + lz4frame.trailer()
    out["word_high_bits"] = hdr + struct.pack("<I", 0x78000005) + bytes(5) + lz4frame.trailer()
    out["trailing_bytes"] = out["opt_b0c0s0d0_64k"] + b"\x04\x22\x4d\x18\x60"
    return out


BUILT = built_frames()
EXPECT = {"legacy": 0, "legacy_then_magic": 0, "legacy_then_skippable": 0, "skippable": 0,
          "skippable_then_frame": 0, "empty": 0, "large_block_many": 0, "word_high_bits": 0,
          "trailing_bytes": 0,
          "linked": lz4ada.BATCH_LINKED, "large_block": lz4ada.BATCH_BIG_BLOCK,
          "legacy_big_slot": lz4ada.BATCH_BIG_BLOCK, "skippable_cut": lz4ada.BATCH_NOT_INDEXED,
          "word_over_max": lz4ada.BATCH_NOT_INDEXED}


def folder(path, exts):
    return sorted(os.path.join(path, f) for f in os.listdir(path) if f.rsplit(".", 1)[-1] in exts)


FILES = folder(VECTORS, ("lz4", "err")) + folder(os.path.join(GOLDEN, "lz4f"), ("lz4",))


def test_file_sets_complete():
    names = {os.path.basename(p) for p in FILES}
    assert {"z100.lz4", "skipz100.lz4", "z100legacy.lz4", "concatlegacy.lz4", "corruptedmagic.err",
            "corruptedhdrchck.err", "linked64k.lz4", "indep4m.lz4"} <= names
    assert len(FILES) >= 50


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_walk_agrees_on_vectors_and_fixtures(path):
    with open(path, "rb") as fh:
        data = fh.read()
    check(data)
    # every frame of a concatenated vector, each with whatever follows it
    try:
        entries = lz4ada.stream_index(data)
    except lz4ada.LZ4AdaError as e:
        entries = e.entries
    for e in entries[1:]:
        check(data[e.offset:])


@pytest.mark.parametrize("name", sorted(BUILT))
def test_walk_agrees_on_built_frames(name):
    v = check(BUILT[name])
    assert v == EXPECT.get(name, lz4ada.DEVFRAME_OK)


def test_walk_info_of_built_frames():
    """The agreement is not vacuous: the frames carry what their names say."""
    v, info, descs = lz4ada.frame_walk_host(BUILT["opt_b1c1s1d1_4096k"])
    assert (v, info.header_len, info.nblocks, info.block_max) == (0, 19, 4, 4 << 20)
    assert (info.block_checksum, info.content_checksum, info.has_content_size) == (1, 1, 1)
    assert info.content_size == 300 + 17 + 1 + 4096 and info.frame_len == len(BUILT["opt_b1c1s1d1_4096k"])
    assert [d.flags for d in descs] == [2, 3, 2, 3]
    v, info, _ = lz4ada.frame_walk_host(BUILT["legacy_then_magic"])
    assert (v, info.format, info.frame_len) == (0, lz4ada.FORMAT_LEGACY, len(BUILT["legacy"]))
    v, info, _ = lz4ada.frame_walk_host(BUILT["skippable_then_frame"])
    assert (v, info.format, info.frame_len, info.nblocks) == (0, lz4ada.FORMAT_SKIPPABLE, 8, 0)


TRUNCATED = ["opt_b1c1s1d1_64k", "legacy_then_magic", "skippable_then_frame"]
# name -> the verdicts its flips give: the 19-byte header's checksum covers
# every descriptor bit and the 20th byte is a size word's; the legacy frame's
# 20 bytes hold its magic, a size word and payload bytes, which the walk ignores
FLIPPED = {"opt_b1c1s1d1_64k": {lz4ada.BATCH_NOT_INDEXED},
           "legacy_then_magic": {lz4ada.BATCH_NOT_INDEXED, lz4ada.DEVFRAME_OK}}


@pytest.mark.parametrize("name", TRUNCATED)
def test_walk_agrees_on_every_truncation(name):
    data = BUILT[name]
    verdicts = {check(data[:n]) for n in range(len(data) + 1)}
    assert verdicts == {lz4ada.DEVFRAME_OK, lz4ada.BATCH_NOT_INDEXED}


@pytest.mark.parametrize("name", sorted(FLIPPED))
def test_walk_agrees_on_every_bit_flip_of_the_first_20_bytes(name):
    data = BUILT[name]
    verdicts = set()
    for bit in range(20 * 8):
        b = bytearray(data)
        b[bit >> 3] ^= 1 << (bit & 7)
        verdicts.add(check(bytes(b)))
    assert verdicts == FLIPPED[name]


def test_walk_writes_no_more_descriptors_than_asked():
    data = BUILT["opt_b0c0s0d0_64k"]
    info = lz4ada.FrameInfo()
    descs = (lz4ada.BlockDesc * 4)()
    ctypes.memset(descs, 0xEE, ctypes.sizeof(descs))
    assert lz4ada._lib.lz4ada_frame_walk_host(data, len(data), ctypes.byref(info), descs, 2) == 0
    assert info.nblocks == 4
    assert bytes(descs)[64:] == b"\xee" * 64 and bytes(descs)[:64] != b"\xee" * 64
