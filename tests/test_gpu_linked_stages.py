"""The linked bulk path stage by stage (lz4ada_bulk_linked.cpp):
several batches with the history carried between them, a block that fails
inside a batch behind committed ones, the extra planes y and h in both plane
modes, and a quirk-D1 stop behind a committed prefix.  Every case compares the
decoded bytes or the raised error with the CPU oracle, and -- where PARENT has
a value -- with what the parent of the commit that cut bulk_linked into stages
gave for the same frame.  64 KiB blocks are the smallest at which the round
state reaches 65536 and quirk D1 can occur."""
import os
import random
import struct

import pytest
import torch

import _oracle as O

import lz4ada
import lz4frame

pytestmark = pytest.mark.gpu

KiB = 1024
BMAX = 64 * KiB
SEED = 0x4C5A3441
L, E = lz4ada.PATH_LINKED, lz4ada.PATH_EXACT

# From the parent commit's library, for these frames: last_path() after
# decode_frame, and what decode_linked_device gave (the decoded length, or
# "exact" for NeedsExactPath).
PARENT = {
    "batches_full": L,
    "batches_short_last": L,
    "fail_block_3": L | E,
    "fail_block_0": L | E,
    "planes": L,
    "d1_uniform": (L, 64 * 64 * KiB),
    "d1_short_block": (L | E, "exact"),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


@pytest.fixture
def env():
    """Set environment knobs of the library for one test."""
    saved = {}

    def set_(k, v):
        saved.setdefault(k, os.environ.get(k))
        os.environ[k] = v
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def oracle(frame):
    return O.unlz4ada(frame, out_cap=4 * len(frame) + (64 << 20))


def five_blocks(last=64 * KiB):
    """Five linked `mixed` blocks of 64 KiB (the last one `last` bytes)."""
    return lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED, SEED, 0, 0, lens=[64 * KiB] * 4 + [last])


def frame_of(blocks, bad=None):
    """A linked frame with block checksums; block `bad`'s stored checksum is wrong."""
    recs = [lz4frame.block_record(c, block_cksum=True) for c, _ in blocks]
    if bad is not None:
        recs[bad] = recs[bad][:-1] + bytes([recs[bad][-1] ^ 0x40])
    raw = b"".join(r for _, r in blocks)
    return (lz4frame.header(BMAX, indep=False, block_cksum=True, content_cksum=True) + b"".join(recs) +
            lz4frame.trailer(raw, content_cksum=True)), raw


def planes_frame():
    """Three linked blocks under a 256 KiB block maximum that need both extra
    planes (the three-plane rule).  Block 1 is literal-heavy: 33
    runs of 2,000 literals, each followed by a match of 31 bytes 30,000 back (the
    first ones read block 0).  Pass 1 declines a block whose first 16 KiB hold
    few sequence starts, but only from 64 KiB of payload on -- the `literal`
    generator's 65,000-byte block is below that and plane z decodes it -- so this
    one has 66,402: plane z gives nothing for it and it takes planes y and h
    (mode 2).  Block 2 begins with a match 65,400 bytes back, 8 long: history
    position 136 of its 65,536, below 256, so the z decoder flags it
    AUX_DEEP_HIST and it takes plane y (mode 1).  The rounds end at 132,028, so
    quirk D1 decides nothing here.  LZ4ADA_TRACE_LINKED=3 on the parent's
    library: block 1 with z 11 (DS_SPARSE), block 2 with z 0, and the `more
    planes` phase -- which a frame of a first block and block 2 alone prints too
    (block 2's mode 1), and a frame of the first block alone does not."""
    rng = random.Random(SEED)
    b0 = lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED, SEED, 0, 0, lens=[65000])
    comp1, out = bytearray(), bytearray(b0[0][1])
    for _ in range(33):
        lits = rng.randbytes(2000)
        comp1 += bytes([0xFF] + [255] * 7 + [2000 - 15 - 7 * 255]) + lits + struct.pack("<H", 30000) + bytes([31 - 19])
        out += lits
        out += out[len(out) - 30000:len(out) - 30000 + 31]
    comp1 += bytes([0x50]) + b"abcde"
    out += b"abcde"
    tail = b"vwxyz"
    comp2 = bytes([0x04]) + struct.pack("<H", 65400) + bytes([0x50]) + tail
    raw2 = bytes(out[len(out) - 65400:len(out) - 65400 + 8]) + tail
    blocks = b0 + [(bytes(comp1), bytes(out[65000:])), (comp2, raw2)]
    return lz4frame.build_frame([(c, r, False) for c, r in blocks], 256 * KiB, indep=False, block_cksum=True,
                                content_cksum=True)


def d1_uniform():
    """test_gpu_linked.py's test_d1_uniform_offsets_64k_frame: 64 linked `mixed`
    blocks of 64 KiB, quirk D1 in about one block of six.  Every block fills its
    slot, so every prediction holds and the decoders emulate each D1 read."""
    blocks = lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED, SEED, 64 * KiB, 64)
    return lz4frame.build_frame([(c, r, False) for c, r in blocks], BMAX, indep=False)


def d1_short_block():
    """A prediction that does not hold.  Block 0 fills 64 KiB, so a D1 round
    follows; block 1 decodes to 1,000 bytes where the prediction has it fill its
    slot, so block 2 starts at Output_Pos 1,000 and was decoded as if at 0; its
    match 65,533 back after 20 literals (test_gpu_linked.py's d1_frame) is a D1
    read.  The bulk path commits blocks 0 and 1 and stops at block 2."""
    blocks = lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED, SEED, 0, 0, lens=[64 * KiB, 1000])
    before = blocks[0][1] + blocks[1][1]
    lits, tail = bytes(range(65, 85)), b"vwxyz"
    comp2 = bytes([0xF6, 20 - 15]) + lits + struct.pack("<H", 65533) + bytes([0x50]) + tail
    at = len(before) + 20 - 65533
    spec2 = lits + before[at:at + 10] + tail  # contiguous history: the reference's bytes may differ (D1)
    return lz4frame.build_frame([(c, r, False) for c, r in blocks + [(comp2, spec2)]], BMAX, indep=False)


def like_oracle(frame):
    """decode_frame_partial gives the oracle's bytes and exception -> its status."""
    st, ref, msg = oracle(frame)
    out, _, exc = lz4ada.decode_frame_partial(frame)
    if st == O.OK:
        assert exc is None and out == ref
    else:
        assert exc is not None and str(exc) == O.exception_information(st, msg)
        assert out == ref  # the blocks the reference output before raising
        with pytest.raises(lz4ada.LZ4AdaError) as ei:
            lz4ada.decode_frame(frame)
        assert str(ei.value) == O.exception_information(st, msg)
    return st, ref


@pytest.mark.parametrize("case,last", [("batches_full", 64 * KiB), ("batches_short_last", 1000)])
def test_several_batches_carry_the_history(case, last, env):
    """200 KiB of budget hold one 64 KiB block and its history region: five
    batches, each resolved against the tail the one before left."""
    env("LZ4ADA_LINKED_BATCH_BYTES", str(200 * KiB))
    frame, raw = frame_of(five_blocks(last))
    st, ref = like_oracle(frame)
    assert st == O.OK and ref == raw
    assert lz4ada.last_path() == PARENT[case]


@pytest.mark.parametrize("case,bad,kept", [("fail_block_3", 3, 3), ("fail_block_0", 0, 0)])
def test_failure_inside_a_batch(case, bad, kept, env):
    """256 KiB of budget hold two blocks: batches [0, 1], [2, 3], [4].  Block
    3's stored checksum is wrong: block 2 of its batch is committed, and the
    reference's error follows the bytes of blocks 0 to 2.  Block 0's: nothing
    is committed."""
    env("LZ4ADA_LINKED_BATCH_BYTES", str(256 * KiB))
    blocks = five_blocks()
    frame, _ = frame_of(blocks, bad=bad)
    st, ref = like_oracle(frame)
    assert st == O.CHECKSUM_ERROR
    assert ref == b"".join(r for _, r in blocks[:kept])
    assert lz4ada.last_path() == PARENT[case]


@pytest.mark.parametrize("words", ["full", "sparse"])
def test_extra_planes_in_both_modes(words, env):
    env("LZ4ADA_LINK_WORDS", words)
    frame, raw = planes_frame()
    st, ref = like_oracle(frame)
    assert st == O.OK and ref == raw
    assert lz4ada.last_path() == PARENT["planes"]


@pytest.mark.parametrize("case", ["d1_uniform", "d1_short_block"])
def test_d1_stop_after_a_committed_prefix(case):
    """The blocks before the first one quirk D1 hands to the exact path are
    committed by the bulk path: decode_frame resumes there, and
    decode_linked_device says that the frame needs the exact path.  A frame
    whose predictions all hold stays on the bulk path in both."""
    frame, _ = {"d1_uniform": d1_uniform, "d1_short_block": d1_short_block}[case]()
    st, ref = like_oracle(frame)
    assert st == O.OK
    assert (lz4ada.last_path(), linked_device(frame, len(ref))) == PARENT[case]


def linked_device(frame, out_len):
    """decode_linked_device over the frame -> the decoded length (the bytes
    checked against the oracle's), or "exact"."""
    info, descs = lz4ada.frame_index(frame)
    d_frame = torch.frombuffer(bytearray(frame), dtype=torch.uint8).cuda()
    d_out = torch.empty(out_len + 16, dtype=torch.uint8, device="cuda")
    try:
        n = lz4ada.decode_linked_device(d_frame.data_ptr(), len(frame), descs, info.nblocks, info.block_max,
                                        d_out.data_ptr(), out_len + 16)
    except lz4ada.NeedsExactPath:
        return "exact"
    assert bytes(d_out[:n].cpu().numpy()) == oracle(frame)[1]
    return n
