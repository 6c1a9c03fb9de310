"""The size rule (csrc/lz4ada_block_size.h: the decoded length of a block
from its payload alone) on the host through
lz4ada_block_size_host, no GPU needed, pinned to the oracle: every block of
every golden vector and liblz4 fixture the oracle decodes, the generator's
blocks of every kind around the sizes where a length field grows, and the
malformed chains, each judged as the oracle judges the block alone in a frame.
No valid block may come out unknown."""
import os

import pytest

import _oracle as O
import lz4ada
import lz4frame
from _lz4build import encode
from conftest import GOLDEN, VECTORS

BMAX = 4 << 20


def folder(path):
    return sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".lz4"))


FILES = folder(VECTORS) + folder(os.path.join(GOLDEN, "lz4f"))
_DECODED = {}


def decoded(path):
    """(the file's bytes, the oracle's output or None when it raises); once per file."""
    if path not in _DECODED:
        with open(path, "rb") as fh:
            data = fh.read()
        st, out, _, _ = O.decode_stream(data)
        _DECODED[path] = (data, out if st == O.OK else None)
    return _DECODED[path]


def oracle_block_lengths(data):
    """The length of every non-empty output the oracle's Update returns over
    the stream: one block per call."""
    import ctypes
    ctx = O.Decompressor.init()
    buf = ctypes.create_string_buffer(ctx.min_buffer_size)
    lens, pos = [], 0
    while pos < len(data):
        st, c, f, l = ctx.update(data[pos:pos + 4096], buf)
        assert st == O.OK, ctx.last_error()
        if l >= f:
            lens.append(l - f + 1)
        pos += c
    return lens


def host_block_sizes(data):
    """block_size_host of every block of every frame of the stream, in order."""
    sizes = []
    for e in lz4ada.stream_index(data):
        if e.info.format == lz4ada.FORMAT_SKIPPABLE:
            continue
        frame = data[e.offset:e.offset + e.frame_len]
        info, descs = lz4ada.frame_index(frame)
        for d in descs[:info.nblocks]:
            payload = frame[d.in_off:d.in_off + d.in_len]
            sizes.append(lz4ada.block_size_host(payload, bool(d.flags & lz4ada.BLOCK_STORED)))
    return sizes


def test_file_set():
    """Every golden .lz4 file is covered, but the quirk-D1 fixtures: the oracle
    raises on those as the reference does (a content checksum over bytes the
    quirk changed), so it has no lengths for them."""
    names = {os.path.basename(p) for p in FILES}
    assert {"z100.lz4", "z100legacy.lz4", "t1111k.lz4", "linked64k.lz4", "indep4m.lz4", "big4m.lz4"} <= names
    assert len(FILES) >= 30
    raised = {os.path.basename(p) for p in FILES if decoded(p)[1] is None}
    assert all(n.startswith("d1_") for n in raised), raised


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_sizes_equal_the_oracles_block_lengths(path):
    data, out = decoded(path)
    sizes = host_block_sizes(data)
    assert all(s >= 0 for s in sizes), [k for k, s in enumerate(sizes) if s < 0]  # valid chains in any case
    if out is None:  # not a file the oracle decodes (test_file_set says which)
        return
    # Update returns nothing for a block that decodes to no byte
    assert [s for s in sizes if s > 0] == oracle_block_lengths(data)
    assert sum(sizes) == len(out)


SIZES = [1, 15, 16, 17, 4095, 65536, 65537]


@pytest.mark.parametrize("kind", range(6))
def test_generated_blocks(kind):
    for n in SIZES:
        comp, raw = lz4ada.gen_block(kind, 1000 * kind + n, n)
        assert len(raw) == n
        assert lz4ada.block_size_host(comp) == n, (kind, n)
        assert lz4ada.block_size_host(raw, stored=True) == n


def oracle_length(payload):
    """The oracle's decoded length of the payload as the only block of a frame,
    -1 when it raises."""
    frame = lz4frame.header(BMAX) + lz4frame.block_record(payload) + lz4frame.trailer()
    st, out, _, _ = O.decode_stream(frame)
    return len(out) if st == O.OK else -1


PRE, PRE_RAW = encode([(b"abcdefgh", 3, 9), (b"", 8, 40), (b"xy", 1, 4)])

MALFORMED = {
    "literal_extension_cut": PRE + b"\xf0\xff\xff",
    "literal_extension_cut_at_first": PRE + b"\xf0",
    "literals_one_past_the_end": PRE + b"\x50tail",
    "match_nibble_after_final_literals": PRE + b"\x54tail!",
    "match_nibble_on_a_last_token": PRE + b"\x07",
    "offset_cut_in_half": PRE + b"\x10A\x01",
    "match_extension_cut": PRE + b"\x1fA\x01\x00\xff\xff",
    "match_extension_cut_at_first": PRE + b"\x1fA\x01\x00",
    "lone_token_with_a_literal": b"\x10",
    "lone_token_with_a_match": b"\x01",
}

VALID = {
    "ends_after_a_match": (PRE, len(PRE_RAW)),
    "ends_with_an_empty_token": (PRE + b"\x00", len(PRE_RAW)),
    "lone_zero_token": (b"\x00", 0),
    "one_literal": (b"\x10A", 1),
    "long_extensions": encode([(b"L" * 600, 7, 15 + 4 + 255 * 3)], b"t" * 15)[:1] +
                       (600 + 15 + 4 + 255 * 3 + 15,),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_chains_are_unknown(name):
    payload = MALFORMED[name]
    assert oracle_length(payload) == -1  # the oracle raises on it
    assert lz4ada.block_size_host(payload) == -1


@pytest.mark.parametrize("name", sorted(VALID))
def test_edge_chains_as_the_oracle_judges_them(name):
    payload, want = VALID[name]
    assert oracle_length(payload) == want
    assert lz4ada.block_size_host(payload) == want


def test_no_payload():
    """n = 0: Decompress_Full_Block's loop does not run (lz4ada.adb:716-788),
    the block is 0 bytes; a frame cannot carry it (a zero size word is the end
    mark), so the rule is stated here."""
    assert lz4ada.block_size_host(b"") == 0
    assert lz4ada.block_size_host(b"", stored=True) == 0


def test_offsets_are_not_judged():
    """A zero offset and one before the block start have a size: the decoders
    judge them."""
    assert oracle_length(b"\x10A\x00\x00\x00") == -1
    assert lz4ada.block_size_host(b"\x10A\x00\x00\x00") == 5
    assert lz4ada.block_size_host(b"\x10A\x09\x00\x00") == 5
