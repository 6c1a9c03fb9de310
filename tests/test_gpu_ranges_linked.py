"""Ranged decode of linked frames through history checkpoints
(lz4ada_seek_index_build_opt with LZ4ADA_SEEK_LINKED).  The
expected bytes are always a slice of the oracle's decode of the whole frame
(for the liblz4 fixtures also pinned to their recorded digests): every block
boundary of a small frame for three checkpoint spacings; a crafted frame whose
blocks read both ends of their checkpoints; the liblz4 fixtures; an index that
mixes every kind of frame; what the selection marks against the chain rule's
model; what the build refuses; an index used after a block of its input
changed; the byte budget; the index's bytes."""
import hashlib
import json
import os
import random
import struct

import pytest
import torch

import lz4ada
import lz4frame
from _lz4build import encode
from conftest import read_vector
from test_gpu_frames_batch import three_blocks
from test_gpu_frames_device import layout, oracle_alone, to_device, to_host
from test_gpu_ranges import check, clip, ranged
from test_ranges_linked_cpu import model

pytestmark = pytest.mark.gpu

KiB = 1024
NOD1 = lz4ada.GEN_MIXED_NOD1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LINKED_PATH = lz4ada.PATH_BATCH | lz4ada.PATH_LINKED
BLOCK_FAILED = (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK, 0)
GAP = 65536 + 256  # dict_gap(65536): the checkpoint and the 32 bytes the ring fill may read behind it, to 256
SMALL_LENS = [65536] * 4 + [777]
SPACINGS = {65536: 1, 131072: 2, 0: 16}  # checkpoint_bytes -> K for 64 KiB blocks (0: the default, 1 MiB)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def passes():
    return lz4ada.last_batch_stats().passes


def linked_frame(lens, seed, bmax=64 * KiB, block_cksum=True, content_cksum=False):
    blocks = [(c, r, False) for c, r in lz4ada.gen_linked_blocks(NOD1, seed, 0, 0, lens=list(lens))]
    return lz4frame.build_frame(blocks, bmax, indep=False, block_cksum=block_cksum, content_cksum=content_cksum)[0]


def fixture_bytes(name):
    with open(os.path.join(GOLDEN, "lz4f", name + ".lz4"), "rb") as fh:
        return fh.read()


def boundary_ranges(lens, job=0, sizes=(1, 2, 65536, 65537)):
    """Ranges that start at every block boundary and one byte before it, and
    the whole frame."""
    size, out, at = sum(lens), [], 0
    for n in [0] + list(lens):
        at += n
        for off in {max(at - 1, 0), at}:
            out += [(job, off, k) for k in sizes]
    return out + [(job, 0, size)]


def index_bytes(nb, n, ckpts=None):
    """lz4ada_seek_index_bytes by the header's formula; ckpts None: built without LZ4ADA_SEEK_LINKED."""
    plain = 32 * nb + 8 * (n + 1) + 16 * (nb + n)
    return plain if ckpts is None else plain + 65536 * ckpts + 8 * (n + 1) + 8 * n


# ---------------------------------------------- every boundary of a small frame

@pytest.fixture(scope="module")
def small():
    """(frame, the oracle's bytes, tensor, spans) of test 3's frame between junk bytes; never modified."""
    frame = linked_frame(SMALL_LENS, 1601)
    raw = oracle_alone(frame)
    assert len(raw) == sum(SMALL_LENS)
    data, spans = layout([frame])
    data = b"\x5a" * 3 + data + b"\xa5" * 9
    spans = [(off + 3, n) for off, n in spans]
    return frame, raw, to_device(data), spans


@pytest.mark.parametrize("checkpoint_bytes", sorted(SPACINGS))
def test_every_boundary_of_a_small_frame(small, checkpoint_bytes):
    frame, raw, t, spans = small
    K = SPACINGS[checkpoint_bytes]
    with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=checkpoint_bytes) as idx:
        assert passes() == 1  # the build's one decode pass
        j = idx.jobs[0]
        assert (j.status, j.reason, j.out_len) == (0, 0, len(raw))
        starts = [sum(SMALL_LENS[:k]) for k in range(len(SMALL_LENS) + 1)]
        assert lz4ada.seek_index_debug(idx, cur_stream()) == [(0, starts)]
        assert idx.device_bytes == index_bytes(5, 1, (5 - 1) // K)
        ranges = boundary_ranges(SMALL_LENS)
        for r in ranges:  # each alone
            out, arr, _ = ranged(idx, t, [r])
            check(out, arr, [r], [raw])
            if clip(len(raw), r[1], r[2]):
                assert passes() == 1 and lz4ada.last_path() == LINKED_PATH
        random.Random(16).shuffle(ranges)
        out, arr, total = ranged(idx, t, ranges)  # all in one call
        check(out, arr, ranges, [raw])
        assert total == sum(clip(len(raw), off, n) for _, off, n in ranges)
        assert passes() == 1 and lz4ada.last_path() == LINKED_PATH


# ------------------------------------------- both ends of a checkpoint are read

def dense_block(rng, total, head, later):
    """A block of `total` decoded bytes in many short sequences (literal runs of
    4 .. 16 bytes, matches of 4 .. 40 bytes a short way back inside the block),
    which begins with the match `head` = (offset, length) and carries the match
    `later` = (offset, length) after `later[2]` decoded bytes -> its payload."""
    seqs, pos = [(b"", head[0], head[1])], head[1]
    placed = False
    while pos < total - 100:
        lits = rng.randbytes(rng.randrange(4, 17))
        if not placed and pos + len(lits) >= later[2]:
            lits = rng.randbytes(later[2] - pos) if later[2] > pos else b""
            seqs.append((lits, later[0], later[1]))
            pos += len(lits) + later[1]
            placed = True
            continue
        ml = rng.randrange(4, 41)
        off = rng.randrange(1, min(pos + len(lits), 2000) + 1)
        seqs.append((lits, off, ml))
        pos += len(lits) + ml
    assert placed
    return encode(seqs, rng.randbytes(total - pos))[0]


def test_both_ends_of_a_checkpoint_are_read():
    """Three full 256 KiB blocks (with 64 KiB blocks every block starts in quirk
    D1's round state, where a match this far back is the exact path's).  Block 1
    begins with a match of offset 65,535 at its first byte -- the farthest byte
    LZ4 can name, the checkpoint's second -- and later reads the checkpoint's
    last byte; block 2 begins with a match of offset 1, the checkpoint's last
    byte, and 4 bytes on carries a match of offset 65,535.  (A match cannot
    start at a block's second byte behind one at its first: a match is at least
    4 bytes long.)"""
    rng = random.Random(1604)
    bmax = 256 * KiB
    b0 = rng.randbytes(bmax)
    b1 = dense_block(rng, bmax, (65535, 8), (1009, 4, 1008))  # at 1,008: offset 1,009 is the byte before the block
    b2 = dense_block(rng, bmax, (1, 4), (65535, 6, 4))
    assert max(len(b1), len(b2)) <= bmax
    for b in (b1, b2):
        assert lz4ada.block_size_host(b) == bmax
    frame = lz4frame.build_frame([(b0, b0, True), (b1, b"", False), (b2, b"", False)], bmax, indep=False,
                                 block_cksum=True)[0]
    raw = oracle_alone(frame)
    assert len(raw) == 3 * bmax and raw[:bmax] == b0
    # the checkpoints' ends do reach the output: block 1 starts with its checkpoint's bytes 1 .. 8, ...
    assert raw[bmax:bmax + 8] == raw[bmax - 65535:bmax - 65527] and raw[bmax + 1008:bmax + 1012] == raw[bmax - 1:bmax + 3]
    assert raw[2 * bmax:2 * bmax + 4] == raw[2 * bmax - 1:2 * bmax] * 4
    assert raw[2 * bmax + 4:2 * bmax + 10] == raw[2 * bmax + 4 - 65535:2 * bmax + 10 - 65535]
    # block 1 alone, as an independent frame, does not decode: the frame needs its history
    alone = lz4frame.build_frame([(b1, b"", False)], bmax, block_cksum=True)[0]
    _, jobs = lz4ada.decode_frames_tensor(to_device(alone), [(0, len(alone))])
    assert jobs[0].status == lz4ada.EXACT_PATH
    data, spans = layout([frame])
    t = to_device(data)
    with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=65536) as idx:  # K = 1
        j = idx.jobs[0]
        assert (j.status, j.reason, j.out_len) == (0, 0, len(raw))
        assert idx.device_bytes == index_bytes(3, 1, 2)
        ranges = [(0, bmax, 16), (0, bmax + 1000, 20), (0, 2 * bmax, 16), (0, 2 * bmax - 5, 4), (0, 3 * bmax - 9, 100),
                  (0, bmax + 70000, 3), (0, 2 * bmax + 4, 6)]
        sel, marked = lz4ada.ranges_select_debug(idx, ranges, cur_stream())
        assert {f for f, _ in sel} == {1, 2} and marked == 2  # block 0 is not decoded
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, [raw])
        assert passes() == 1 and lz4ada.last_path() == LINKED_PATH


# ------------------------------------------------------------ liblz4 fixtures

DIGESTS = json.load(open(os.path.join(GOLDEN, "lz4f_digests.json")))


@pytest.mark.parametrize("checkpoint_bytes", [1, 0])  # K = 1, and the default
@pytest.mark.parametrize("name,nblocks,bmax", [("linked64k", 17, 64 * KiB), ("linked256k", 7, 256 * KiB)])
def test_liblz4_fixtures(name, nblocks, bmax, checkpoint_bytes):
    frame = fixture_bytes(name)
    raw = oracle_alone(frame)
    ent = DIGESTS["frames"][name]  # the recorded plaintext: the encoder's input
    assert ent["output_is_input"] and ent["input"] == {"len": len(raw), "sha256": hashlib.sha256(raw).hexdigest(),
                                                      "xxh32": ent["input"]["xxh32"]}
    lens = [bmax] * (nblocks - 1) + [len(raw) - bmax * (nblocks - 1)]
    assert 0 < lens[-1] <= bmax
    K = 1 if checkpoint_bytes else max(1, (1 << 20) // bmax)
    data, spans = layout([frame])
    t = to_device(data)
    with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=checkpoint_bytes) as idx:
        j = idx.jobs[0]
        assert (j.status, j.reason, j.out_len) == (0, 0, len(raw))
        assert idx.device_bytes == index_bytes(nblocks, 1, (nblocks - 1) // K)
        rng = random.Random(1605)
        ranges = [(0, rng.randrange(len(raw)), rng.choice([1, 3, 4096, 70000, 300000])) for _ in range(64)]
        ranges += boundary_ranges(lens, sizes=(1, 2))
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, [raw])
        assert passes() == 1 and lz4ada.last_path() == LINKED_PATH


# --------------------------------------------------------------- a mixed index

def test_a_mixed_index(monkeypatch):
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(6 * 65536))  # per call, as in the many-frame pass
    indep, indep_raw = three_blocks(block_cksum=True)
    frames = [indep, linked_frame([65536, 65536, 65536, 4000], 1611), read_vector("z100legacy", "lz4"),
              linked_frame([65536] * 6 + [5], 1612),  # 7 slots: over the cap
              struct.pack("<II", 0x184D2A57, 21) + bytes(range(21)), linked_frame([65536, 65536, 100], 1613, block_cksum=False),
              indep]
    OVER, SKIP = 3, 4
    raws = [oracle_alone(f) if i != SKIP else b"" for i, f in enumerate(frames)]
    data, spans = layout(frames)
    t = to_device(data)
    rng = random.Random(1606)
    ranges = []
    for _ in range(40):
        job = rng.randrange(len(frames))
        ranges.append((job, rng.randrange(len(raws[job]) + 2), rng.choice([1, 2, 300, 65536, 70000, 1 << 20])))
    ranges += [(1, 65535, 2), (1, 65535, 2), (5, 0, 1 << 20), (1, 131072, 1), (0, 0, 1 << 20), (OVER, 5, 5), (5, 131072, 100)]
    with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=65536) as idx:
        got = [(j.status, j.reason, j.out_len) for j in idx.jobs[:len(frames)]]
        want = [(0, 0, len(r)) for r in raws]
        want[OVER] = (lz4ada.EXACT_PATH, lz4ada.BATCH_LINKED, 0)
        assert got == want
        assert idx.device_bytes == index_bytes(3 + 4 + 1 + 0 + 0 + 3 + 3, 7, 3 + 2)  # the frame over the cap takes no room
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, raws, reasons={OVER: lz4ada.BATCH_LINKED})
        assert passes() == 1
        assert lz4ada.last_path() == lz4ada.PATH_BATCH | lz4ada.PATH_LINKED | lz4ada.PATH_INDEPENDENT
        only = [r for r in ranges if r[0] in (0, 2, 6)]
        mixed_out, mixed_arr, _ = ranged(idx, t, only)
        assert lz4ada.last_path() == lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT
    # the new entry without the flag is the plain build: both linked frames refused, the same independent bytes
    refused = {1: lz4ada.BATCH_LINKED, OVER: lz4ada.BATCH_LINKED, 5: lz4ada.BATCH_LINKED}
    with lz4ada.SeekIndex.build_tensor(t, spans, checkpoint_bytes=65536) as unflagged, \
            lz4ada.SeekIndex.build_tensor(t, spans) as plain:
        assert passes() == 0
        assert unflagged.device_bytes == plain.device_bytes == index_bytes(3 + 1 + 3, 7)
        assert [(j.status, j.reason, j.out_len) for j in unflagged.jobs[:7]] == \
            [(j.status, j.reason, j.out_len) for j in plain.jobs[:7]]
        out_u, arr_u, _ = ranged(unflagged, t, ranges)
        check(out_u, arr_u, ranges, raws, reasons=refused)
        out_p, arr_p, _ = ranged(plain, t, ranges)
        assert out_u == out_p
        assert ranged(unflagged, t, only)[0] == ranged(plain, t, only)[0] == mixed_out


# ------------------------------------------------------------ what gets marked

def test_what_gets_marked():
    lens = [65536] * 8 + [3000]
    frame = linked_frame(lens, 1607, block_cksum=False)
    data, spans = layout([frame])
    t = to_device(data)
    size = sum(lens)

    def touched(off, n):
        n = clip(size, off, n)
        return (off // 65536, (off + n - 1) // 65536 - off // 65536 + 1) if n else (0, 0)

    rng = random.Random(1608)
    sets = [[(70000, 1), (100000, 5)],              # two ranges in one group
            [(3 * 65536 + 5, 3 * 65536)],           # a range spanning three groups
            [(10, 10)],                             # a range in block 0
            [(8 * 65536 + 1, 10), (0, 1)], [(size - 1, 1)], [(65536, 65536), (65536 * 2, 1)], [(size, 4)]]
    while len(sets) < 12:
        sets.append([(rng.randrange(size), rng.choice([1, 2, 65536, 65537, 200000])) for _ in range(rng.randrange(1, 5))])
    with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=131072) as idx:  # K = 2
        assert idx.device_bytes == index_bytes(9, 1, 4)
        for s in sets:
            want = [touched(off, n) for off, n in s]
            sel, marked = lz4ada.ranges_select_debug(idx, [(0, off, n) for off, n in s], cur_stream())
            assert sel == want, s
            assert marked == len(model(9, 2, want)[0]), s


# --------------------------------------- the build refuses what the chain refuses

def refused_frame(case):
    if case == "d1_round_state":
        return fixture_bytes("d1_l13_o65529")
    if case == "short_middle_block":
        return linked_frame([65536, 30000, 65536], 1609)
    frame = linked_frame([65536, 65536, 2000], 1610)
    _, descs = lz4ada.frame_index(frame)
    b = bytearray(frame)
    b[descs[1].in_off + descs[1].in_len - 1] ^= 0x01  # the last literal of block 1: the chain still adds up
    return bytes(b)


@pytest.mark.parametrize("case", ["d1_round_state", "flipped_payload_byte", "short_middle_block"])
def test_the_build_refuses_what_the_chain_refuses(case):
    bad = refused_frame(case)
    before, after = linked_frame([65536, 65536, 900], 1614), linked_frame([65536, 1234], 1615)
    indep, indep_raw = three_blocks(block_cksum=True)
    frames = [before, bad, after, indep]
    raws = [oracle_alone(before), b"", oracle_alone(after), indep_raw]
    data, spans = layout(frames)
    t = to_device(data)
    with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=65536) as idx:
        got = [(j.status, j.reason, j.out_len) for j in idx.jobs[:4]]
        assert got == [(0, 0, len(raws[0])), BLOCK_FAILED, (0, 0, len(raws[2])), (0, 0, len(raws[3]))]
        assert lz4ada.seek_index_debug(idx, cur_stream())[1] == (lz4ada.DEVFRAME_BLOCK, [0])  # not half-indexed
        ranges = [(1, 0, 10), (0, 65530, 70000), (1, 70000, 5), (2, 65535, 2), (3, 5, 100), (1, 0, 1 << 20), (0, 0, 1),
                  (2, 0, 1 << 20)]
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, raws, reasons={1: lz4ada.DEVFRAME_BLOCK})
        assert ranged(idx, t, [(1, 0, 100)])[2] == 0 and passes() == 0


# ------------------------------------------------- input changed after the build

def test_input_changed_after_the_build():
    lens = [65536] * 4 + [5000]
    frame = linked_frame(lens, 1616, block_cksum=False)
    raw = oracle_alone(frame)
    _, descs = lz4ada.frame_index(frame)
    data, spans = layout([frame])
    t = to_device(data)
    at, n = spans[0][0] + descs[2].in_off, descs[2].in_len
    payload = b"\xf0" + b"\xff" * (n - 1)  # a literal length that never ends
    assert lz4ada.block_size_host(payload) == -1
    with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=131072) as idx:  # groups {0,1} {2,3} {4}
        assert (idx.jobs[0].status, idx.jobs[0].out_len) == (0, len(raw))
        t2 = t.clone()
        t2[at:at + n] = to_device(payload)
        changed = data[:at] + payload + data[at + n:]
        assert to_host(t2) == changed
        lo, hi = 2 * 65536, 4 * 65536  # the bytes of blocks 2 and 3
        mine = [(0, 100), (65536, 65536), (lo - 1, 1), (lo - 1, 2), (lo, 1), (lo + 70000, 5), (hi - 1, 1), (hi - 1, 2),
                (hi, 1), (hi, 1 << 20), (3 * 65536, 10), (0, 1 << 20), (5, 5), (hi + 4999, 1)]
        ranges = [(0, off, k) for off, k in mine]
        failed = {i for i, (off, k) in enumerate(mine) if off < hi and off + k > lo}
        assert len(failed) == 7 and len(mine) - len(failed) == 7
        out, arr, _ = ranged(idx, t2, ranges)  # (checks the sentinel tail and that the input is untouched)
        check(out, arr, ranges, [raw], failed=failed)
        assert passes() == 1 and lz4ada.last_path() == LINKED_PATH
        assert to_host(t2) == changed


# ---------------------------------------------------------------------- budget

def test_budget(small, monkeypatch):
    frame, raw, t, spans = small
    with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=131072) as idx:  # K = 2
        # two chains: blocks {2, 3} behind a gap, and block 4 behind a gap
        ranges = [(0, 3 * 65536 + 5, 10), (0, 4 * 65536 + 1, 700), (0, 3, 3)]
        whole, _, _ = ranged(idx, t, ranges)
        assert passes() == 1
        one = 2 * 65536 + GAP  # the first chain and its gap; the second needs 1,024 + GAP more
        monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(one + 1000))
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, [raw])
        assert out == whole and passes() > 1
        monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(one - 1))  # below that chain plus its gap
        out, arr, total = ranged(idx, t, ranges)
        r = arr[0]
        assert (r.status, r.reason, r.out_len, r.out_off) == (lz4ada.EXACT_PATH, lz4ada.BATCH_OVER_BUDGET, 0, 0)
        assert total == len(whole) and out[10:] == whole[10:]
        assert [(a.status, a.reason, a.out_len) for a in arr[1:3]] == [(0, 0, 700), (0, 0, 3)]


# ----------------------------------------------------------------- index bytes

def test_index_bytes(small):
    frame, raw, t, spans = small
    got = {}
    for checkpoint_bytes, K in SPACINGS.items():
        with lz4ada.SeekIndex.build_tensor(t, spans, linked=True, checkpoint_bytes=checkpoint_bytes) as idx:
            got[K] = idx.device_bytes
            assert got[K] == index_bytes(5, 1, 4 // K)
    per_frame = 8 * 2 + 8 * 1  # the checkpoints' prefix and K
    assert got[1] - got[16] == 4 * 65536 and got[2] - got[16] == 2 * 65536
    assert got[1] == index_bytes(5, 1) + 4 * 65536 + per_frame
