"""Seek index and ranged decode of device-resident frames
(lz4ada_seek_index_build, lz4ada_decode_ranges_device).  The
expected bytes are always a slice of the oracle's decode of the whole frame:
every (off, len) of a small frame of odd blocks, at every alignment of source
and destination; block counts and range counts around the scan steps; full
blocks through the real decoders and what the selection marks; a failing block
that costs only the ranges that touch it; what a range does not assert; linked
frames; the output bound; the byte budget; reuse, threads' scratch and the
index's lifetime; an index used after a block of its input changed."""
import random
import struct

import pytest
import torch

import lz4ada
import lz4frame
from _lz4build import encode
from conftest import read_vector
from test_block_size_cpu import MALFORMED, oracle_block_lengths
from test_gpu_frames_batch import bad_frame, three_blocks
from test_gpu_frames_device import (BAD_AT, NFRAMES, SENTINEL, TAIL, batch, layout, linked_frame,  # noqa: F401
                                    oracle_alone, to_device, to_host)
from test_gpu_frames_sizes import small_frame

pytestmark = pytest.mark.gpu

OK_PATH = lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT
BLOCK_FAILED = (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def passes():
    return lz4ada.last_batch_stats().passes


def clip(size, off, n):
    return max(0, min(off + n, size) - off)


def ranged(idx, t, ranges):
    """decode_ranges_device into a buffer of exactly the clipped total with a
    sentinel tail -> (the bytes, the FrameRange array, the total); the total
    from out_cap = 0, the tail and the input are checked."""
    before = to_host(t)
    try:
        total, _ = lz4ada.decode_ranges_device(idx, t.data_ptr(), t.numel(), ranges, None, 0, cur_stream())
        assert total == 0
    except lz4ada.TooLittleMemory as e:
        total = e.bound
        assert passes() == 0
    buf = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device=t.device)
    out, arr = lz4ada.decode_ranges_tensor(idx, t, ranges, out=buf[:max(total, 1)])
    torch.cuda.current_stream().synchronize()
    assert out.numel() == total
    whole = to_host(buf)
    assert whole[total:] == bytes([SENTINEL]) * TAIL  # nothing at or beyond *out_len
    assert to_host(t) == before
    return whole[:total], arr, total


def check(out, arr, ranges, raws, failed=(), reasons=None):
    """Every range: its place (the running sum of the clipped lengths, in the
    caller's order), its status, its length, its bytes.  failed: indices of
    ranges that keep their place and deliver nothing (DEVFRAME_BLOCK);
    reasons: {job: reason} of frames the index did not accept."""
    at = 0
    reasons = reasons or {}
    for i, (job, off, n) in enumerate(ranges):
        r = arr[i]
        assert (r.job, r.off, r.len) == (job, off, n), i
        assert r.out_off == at, i
        if job in reasons:
            assert (r.status, r.reason, r.out_len) == (lz4ada.EXACT_PATH, reasons[job], 0), i
            continue
        want = clip(len(raws[job]), off, n)
        if i in failed:
            assert (r.status, r.reason, r.out_len) == (*BLOCK_FAILED, 0), i
        else:
            assert (r.status, r.reason, r.out_len) == (0, 0, want), i
            assert out[at:at + want] == raws[job][off:off + want], i
        at += want
    assert at == len(out)


# ------------------------------------------------ exhaustive on a small frame

ODD_SIZES = [300, 0, 1, 256, 77, 0, 513]


def odd_frame():
    rng = random.Random(14)
    blocks = [(*lz4ada.gen_block(1, 141, 300), False), (b"", b"", True), (*lz4ada.gen_block(0, 142, 1), False)]
    raw = rng.randbytes(256)
    blocks += [(raw, raw, True), (*lz4ada.gen_block(1, 143, 77), False), (b"\x00", b"", False),
               (*lz4ada.gen_block(0, 144, 513), False)]
    assert [len(b[1]) for b in blocks] == ODD_SIZES
    return lz4frame.build_frame(blocks, 64 << 10, block_cksum=True)[0]


def test_every_range_of_a_small_frame():
    frame = odd_frame()
    raw = oracle_alone(frame)
    size = sum(ODD_SIZES)
    assert len(raw) == size
    rng = random.Random(15)
    data = rng.randbytes(13) + frame + rng.randbytes(7)
    t = to_device(data)
    with lz4ada.SeekIndex.build_tensor(t, [(13, len(frame))]) as idx:
        j = idx.jobs[0]
        assert (j.status, j.reason, j.out_len) == (0, 0, size)
        starts = [sum(ODD_SIZES[:k]) for k in range(len(ODD_SIZES) + 1)]
        assert lz4ada.seek_index_debug(idx, cur_stream()) == [(0, starts)]
        ranges = [(0, off, n) for off in range(size + 3) for n in (0, 1, 2, 255, 256, 257, size)]
        out, arr, total = ranged(idx, t, ranges)
        check(out, arr, ranges, [raw])
        assert total == sum(clip(size, off, n) for _, off, n in ranges)
        assert passes() == 1 and lz4ada.last_path() == OK_PATH
        # every residue of 16 of the destination, and of the source inside a slot
        assert {arr[i].out_off & 15 for i in range(len(ranges)) if arr[i].out_len >= 255} == set(range(16))


# ------------------------------------------- block counts around the scan steps

COUNTS = (1, 63, 64, 65, 129, 1025)


@pytest.fixture(scope="module")
def counted():
    """Frames of 1 .. 1,025 small blocks, an empty one, a skippable one and
    z100legacy, indexed once: (raws, tensor, index, block lengths per frame)."""
    frames = [small_frame(500 + k, n)[0] for k, n in enumerate(COUNTS)]
    frames.append(lz4frame.build_frame([], 64 << 10, content_cksum=True)[0])
    frames.append(struct.pack("<II", 0x184D2A57, 21) + bytes(range(21)))
    frames.append(read_vector("z100legacy", "lz4"))
    raws = [oracle_alone(f) if f[:4] != frames[-2][:4] else b"" for f in frames]
    lens = [oracle_block_lengths(f) if raws[i] else [] for i, f in enumerate(frames)]
    assert [len(x) for x in lens] == list(COUNTS) + [0, 0, 1]
    data, spans = layout(frames)
    t = to_device(data)
    idx = lz4ada.SeekIndex.build_tensor(t, spans)
    yield raws, t, idx, lens
    idx.free()


def test_index_is_the_running_sum_of_block_lengths(counted):
    raws, t, idx, lens = counted
    table = lz4ada.seek_index_debug(idx, cur_stream())
    nb = sum(len(x) for x in lens)
    assert idx.device_bytes == 32 * nb + 8 * (len(lens) + 1) + 16 * (nb + len(lens))
    for job, (reason, starts) in enumerate(table):
        assert reason == 0 and idx.jobs[job].out_len == len(raws[job]), job
        assert starts == [sum(lens[job][:k]) for k in range(len(lens[job]) + 1)], job


def test_ranges_at_every_block_boundary(counted):
    raws, t, idx, lens = counted
    ranges = []
    for job, raw in enumerate(raws):
        size = len(raw)
        ranges += [(job, 0, size), (job, size - 1 if size else 0, 1), (job, size, 1), (job, 0, size + 5)]
        at = 0
        for n in lens[job]:
            at += n
            ranges += [(job, at - 1, 1), (job, at - 1, 2), (job, at, 1), (job, max(at - 1 - n, 0), n + 2)]
    out, arr, _ = ranged(idx, t, ranges)
    check(out, arr, ranges, raws)
    assert passes() == 1


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_range_counts_around_the_scans(counted, count):
    raws, t, idx, _ = counted
    rng = random.Random(count)
    ranges = []
    for _ in range(count):
        job = rng.randrange(len(raws))
        ranges.append((job, rng.randrange(len(raws[job]) + 2), rng.choice([1, 2, 19, 70, 71, 4000])))
    out, arr, _ = ranged(idx, t, ranges)
    check(out, arr, ranges, raws)  # back to back in the caller's order


# ------------------------------------------- full blocks through the decoders

def full_frame(kind, seed):
    blocks = [(*lz4ada.gen_block(kind, seed + k, n), False) for k, n in enumerate([65536] * 3 + [1000])]
    return lz4frame.build_frame(blocks, 64 << 10, block_cksum=True, content_cksum=True)[0]


@pytest.fixture(scope="module")
def full():
    frames = [full_frame(lz4ada.GEN_MIXED, 900), full_frame(lz4ada.GEN_DENSE, 910)]
    raws = [oracle_alone(f) for f in frames]
    assert [len(r) for r in raws] == [3 * 65536 + 1000] * 2
    data, spans = layout(frames)
    t = to_device(data)
    idx = lz4ada.SeekIndex.build_tensor(t, spans)
    yield raws, t, idx
    idx.free()


def test_full_size_blocks(full):
    raws, t, idx = full
    size = len(raws[0])
    ranges = [(job, off, n) for job in (1, 0)
              for off, n in [(65535, 2), (0, 1), (131071, 65538), (0, size), (size, 1), (size - 1, 9)]]
    out, arr, _ = ranged(idx, t, ranges)
    check(out, arr, ranges, raws)
    assert passes() == 1 and lz4ada.last_path() == OK_PATH


def test_what_the_selection_marks(full):
    raws, t, idx = full
    sel = lambda ranges: lz4ada.ranges_select_debug(idx, ranges, cur_stream())  # noqa: E731
    assert sel([(0, 70000, 1)]) == ([(1, 1)], 1)                     # a byte: its block alone
    assert sel([(0, 70000, 1), (0, 131000, 50)]) == ([(1, 1), (1, 1)], 1)  # two in one block mark it once
    assert sel([(0, 65535, 2)]) == ([(0, 2)], 2)
    assert sel([(1, 131071, 65538), (0, 0, 1), (1, 0, 0), (1, 1 << 40, 5)]) == ([(1, 3), (0, 1), (0, 0), (0, 0)], 4)
    assert sel([(0, 0, 1 << 40), (0, 5, 5), (1, 196608, 1)]) == ([(0, 4), (0, 1), (3, 1)], 5)
    assert sel([(0, len(raws[0]), 1)]) == ([(0, 0)], 0)


# ------------------------------------- failures cost the ranges that touch them

FOUR = [3000, 2000, 1000, 500]
PRE_REF = b"\x10A\x05\x00" + b"\x50hello"  # a literal, then a match 5 back from position 1; decodes to 10 bytes


def four_blocks(case):
    """(frame of four blocks with block checksums, its blocks' plaintext with
    None for the one that fails, the decoded block sizes)."""
    blocks = [(*lz4ada.gen_block(1, 800 + k, n), False) for k, n in enumerate(FOUR)]
    sizes = list(FOUR)
    if case == "pre_block_ref":
        assert lz4ada.block_size_host(PRE_REF) == 10
        blocks[2] = (PRE_REF, b"?" * 10, False)
        sizes[2] = 10
    frame = lz4frame.build_frame(blocks, 64 << 10, block_cksum=True)[0]
    if case == "block_checksum":
        _, descs = lz4ada.frame_index(frame)
        b = bytearray(frame)
        b[descs[2].in_off + descs[2].in_len] ^= 0x10
        frame = bytes(b)
    raw = b"".join(b[1] for b in blocks)
    return frame, raw, sizes


@pytest.mark.parametrize("case", ["block_checksum", "pre_block_ref"])
def test_a_failing_block_costs_the_ranges_that_touch_it(batch, case):
    frame, raw, sizes = four_blocks(case)
    lo, hi = sum(sizes[:2]), sum(sizes[:3])  # block 2's bytes
    good = four_blocks(None)[0]
    assert oracle_alone(good)[:lo] == raw[:lo] and oracle_alone(good)[-sizes[3]:] == raw[hi:]
    items = list(batch)
    items[BAD_AT] = (frame, raw, False)
    raws = [r for _, r, _ in items]
    data, spans = layout([f for f, _, _ in items])
    t = to_device(data)
    with lz4ada.SeekIndex.build_tensor(t, spans) as idx:
        assert [(j.status, j.reason) for j in idx.jobs[:NFRAMES]] == [(0, 0)] * NFRAMES
        assert idx.jobs[BAD_AT].out_len == len(raw)
        ranges = [(i, 0, len(r) + 1) for i, r in enumerate(raws) if i != BAD_AT]
        mine = [(0, lo), (lo - 1, 1), (lo - 1, 2), (lo, 1), (hi - 1, 1), (hi - 1, 2), (hi, 1), (hi, 1 << 30),
                (0, len(raw)), (10, 5), (lo + 3, 2), (0, lo + 1)]
        touching = {k for k, (off, n) in enumerate(mine) if off < hi and off + n > lo}
        assert len(touching) == 7 and len(mine) - len(touching) == 5
        at = len(ranges) // 2
        ranges[at:at] = [(BAD_AT, off, n) for off, n in mine]
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, raws, failed={at + k for k in touching})
        assert passes() == 1 and lz4ada.last_path() == OK_PATH


@pytest.mark.parametrize("where", range(4))
def test_a_malformed_chain_rejects_the_frame_at_the_build(where):
    blocks = [(*lz4ada.gen_block(1, 820 + k, n), False) for k, n in enumerate(FOUR)]
    blocks[where] = (MALFORMED[sorted(MALFORMED)[where]], b"", False)
    bad = lz4frame.build_frame(blocks, 64 << 10, block_cksum=True)[0]
    good, raw = lz4frame.build_frame(blocks[:where] + blocks[where + 1:], 64 << 10, block_cksum=True)
    assert oracle_alone(good) == raw
    data, spans = layout([good, bad, good])
    t = to_device(data)
    with lz4ada.SeekIndex.build_tensor(t, spans) as idx:
        j = idx.jobs[1]
        assert (j.status, j.reason, j.out_len) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK, 0)
        assert lz4ada.seek_index_debug(idx, cur_stream())[1] == (lz4ada.DEVFRAME_BLOCK, [0])
        ranges = [(0, 5, 100), (1, 0, 100), (1, 5, 0), (2, 0, 1 << 20), (1, 1 << 20, 1)]
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, [raw, b"", raw], reasons={1: lz4ada.DEVFRAME_BLOCK})
        only_bad = [(1, 0, 100)]
        out, arr, total = ranged(idx, t, only_bad)
        assert total == 0 and passes() == 0 and lz4ada.last_path() == 0


# ------------------------------------------------ what a range does not assert

def test_a_range_does_not_assert_the_content_checksum():
    bad = bad_frame("content_checksum")
    good, raw = three_blocks(content_cksum=True)
    assert bad[:-1] == good[:-1] and bad != good and oracle_alone(good) == raw
    t = to_device(bad)
    _, jobs = lz4ada.decode_frames_tensor(t, [(0, len(bad))])
    assert (jobs[0].status, jobs[0].reason) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_CHECKSUM)
    with lz4ada.SeekIndex.build_tensor(t, [(0, len(bad))]) as idx:
        ranges = [(0, 0, len(raw)), (0, 65530, 12)]
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, [raw])


def test_linked_frames_are_refused():
    good, raw = three_blocks(block_cksum=True)
    data, spans = layout([good, linked_frame()])
    t = to_device(data)
    with lz4ada.SeekIndex.build_tensor(t, spans) as idx:
        j = idx.jobs[1]
        assert (j.status, j.reason, j.out_len) == (lz4ada.EXACT_PATH, lz4ada.BATCH_LINKED, 0)
        ranges = [(1, 0, 10), (0, 3, 10), (1, 70000, 1)]
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, [raw, b""], reasons={1: lz4ada.BATCH_LINKED})
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.SeekIndex.build(t.data_ptr(), t.numel(), spans, cur_stream(), flags=lz4ada.FRAMES_LINKED)


# --------------------------------------------------------------------- memory

def test_output_below_the_total(full):
    raws, t, idx = full
    ranges = [(0, 100, 70000), (1, 5, 5), (0, 0, 1)]
    total = 70000 + 5 + 1
    buf = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device=t.device)
    with pytest.raises(lz4ada.TooLittleMemory) as ei:
        lz4ada.decode_ranges_device(idx, t.data_ptr(), t.numel(), ranges, buf.data_ptr(), total - 1, cur_stream())
    torch.cuda.synchronize()
    assert ei.value.bound == total and str(total) in ei.value.message
    assert to_host(buf) == bytes([SENTINEL]) * (total + TAIL) and passes() == 0
    out, arr, got = ranged(idx, t, ranges)  # exactly the total works
    assert got == total
    check(out, arr, ranges, raws)
    out2, arr2 = lz4ada.decode_ranges_tensor(idx, t, ranges)  # allocates the total
    assert out2.numel() == total and to_host(out2) == out


# --------------------------------------------------------------------- budget

def test_budget_splits_the_passes(full, monkeypatch):
    raws, t, idx = full
    size = len(raws[0])
    ranges = [(0, 0, 1), (1, 70000, 1), (0, 140000, 1), (1, 196608, 3), (0, 65535, 2)]
    whole, _, _ = ranged(idx, t, ranges)
    assert passes() == 1
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", "140000")  # two blocks' slots, not three
    out, arr, _ = ranged(idx, t, ranges)
    check(out, arr, ranges, raws)
    assert out == whole and passes() > 1
    over = ranges + [(1, 0, size), (0, 5, 5)]
    out, arr, total = ranged(idx, t, over)
    r = arr[len(ranges)]
    assert (r.status, r.reason, r.out_len, r.out_off) == (lz4ada.EXACT_PATH, lz4ada.BATCH_OVER_BUDGET, 0, len(whole))
    assert total == len(whole) + size + 5 and out[:len(whole)] == whole
    assert out[-5:] == raws[0][5:10] and arr[len(over) - 1].out_off == len(whole) + size


# --------------------------------------------------------- reuse and lifetime

def test_reuse_and_lifetime():
    frames = [full_frame(lz4ada.GEN_MIXED, 950), small_frame(77, 65)[0]]
    raws = [oracle_alone(f) for f in frames]
    data, spans = layout(frames)
    t = to_device(data)
    lz4ada.release_device_cache()
    idle = lambda: (lambda s: (s.device_idle_bytes, s.pinned_idle_bytes))(lz4ada.device_cache_stats())  # noqa: E731
    before = idle()
    idx = lz4ada.SeekIndex.build_tensor(t, spans)
    assert idx.device_bytes == 32 * 69 + 8 * 3 + 16 * (69 + 2)
    ranges = [(1, 0, 1 << 20), (0, 65000, 70000), (1, 33, 3), (0, 0, 1)]
    out, arr, _ = ranged(idx, t, ranges)
    check(out, arr, ranges, raws)
    lz4ada.release_device_cache()  # the index's memory is not the scratch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out2, arr2, _ = ranged(idx, t, ranges)
    assert out2 == out
    assert [(r.out_off, r.out_len, r.status, r.reason) for r in arr2[:4]] == \
        [(r.out_off, r.out_len, r.status, r.reason) for r in arr[:4]]
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.decode_ranges_device(idx, t.data_ptr(), t.numel() - 1, ranges, None, 0, cur_stream())
    assert passes() == 0
    idx.free()
    lz4ada.release_device_cache()
    assert idle() == before


# ------------------------------------------- an index used after its input changed

CHANGES = ("same_size", "larger", "smaller", "malformed")


def changed_block(variant, seed=0):
    """Block 2 of the changed frame and its variants, all of one payload length:
    600 literals, a match, five last literals (1,000 bytes decoded; the match
    40 bytes longer or shorter: the same number of extension bytes); the
    malformed one is a valid sequence, then MALFORMED's literals one past the
    end.  -> (payload, decoded bytes or None)."""
    rng = random.Random(1400 + seed)
    if variant == "malformed":
        head = encode([(rng.randbytes(600 - len(MALFORMED["literals_one_past_the_end"]) + 6), 3, 395)])[0]
        return head + MALFORMED["literals_one_past_the_end"], None
    ml = dict(larger=435, smaller=355).get(variant, 395)
    return encode([(rng.randbytes(600), 3 if variant is None else 7, ml)], rng.randbytes(5))


@pytest.fixture(scope="module")
def changed():
    """A frame of four blocks without block checksums between two other
    frames, indexed once: (data, spans, tensor, index, the original bytes per
    frame, block 2's payload position, the variants, block 2's extent in the
    frame's plaintext).  The parts a CPU can check are checked here."""
    blocks = [(*lz4ada.gen_block(1, 830 + k, n), False) for k, n in enumerate(FOUR)]
    blocks[2] = (*changed_block(None), False)
    frame = lz4frame.build_frame(blocks, 64 << 10)[0]
    info, descs = lz4ada.frame_index(frame)
    assert info.nblocks == 4 and not any(d.flags & lz4ada.BLOCK_HAS_CKSUM for d in descs[:4])
    variants = {v: changed_block(v, 1 + k) for k, v in enumerate(CHANGES)}
    n = len(blocks[2][0])
    assert descs[2].in_len == n and all(len(p) == n for p, _ in variants.values())
    assert lz4ada.block_size_host(blocks[2][0]) == 1000 == len(blocks[2][1])
    assert [lz4ada.block_size_host(variants[v][0]) for v in CHANGES] == [1000, 1040, 960, -1]
    assert variants["same_size"][1] != blocks[2][1]
    frames = [full_frame(lz4ada.GEN_MIXED, 930), frame, four_blocks(None)[0]]
    raws = [oracle_alone(f) for f in frames]
    assert raws[1] == b"".join(b[1] for b in blocks)
    same = frame[:descs[2].in_off] + variants["same_size"][0] + frame[descs[2].in_off + n:]
    lo, hi = sum(FOUR[:2]), sum(FOUR[:2]) + 1000
    assert oracle_alone(same) == raws[1][:lo] + variants["same_size"][1] + raws[1][hi:]
    data, spans = layout(frames)
    t = to_device(data)
    idx = lz4ada.SeekIndex.build_tensor(t, spans)
    assert [(j.status, j.reason, j.out_len) for j in idx.jobs[:3]] == [(0, 0, len(r)) for r in raws]
    yield data, spans, t, idx, raws, spans[1][0] + descs[2].in_off, variants, (lo, hi)
    idx.free()


@pytest.mark.parametrize("variant", CHANGES)
def test_an_index_used_after_its_input_changed(changed, variant):
    """DESIGN.md §14, "If the input changed since the build": a block whose
    bytes changed under the index decodes to other bytes inside its own slot
    or fails its size, and costs only the ranges that touch it."""
    data, spans, t, idx, raws, at, variants, (lo, hi) = changed
    payload, new = variants[variant]
    t2 = t.clone()
    t2[at:at + len(payload)] = to_device(payload)
    assert to_host(t2) == data[:at] + payload + data[at + len(payload):]
    raws = list(raws)
    size = len(raws[1])
    mine = [(0, lo), (lo - 1, 1), (lo - 1, 2), (lo, 1), (hi - 1, 1), (hi - 1, 2), (hi, 1), (hi, 1 << 30),
            (0, size), (10, 5), (lo + 3, 2), (0, lo + 1), (lo, hi - lo), (hi, size - hi)]
    touching = {k for k, (off, n) in enumerate(mine) if off < hi and off + n > lo}
    assert len(touching) == 8 and len(mine) - len(touching) == 6
    ranges = [(0, 0, len(raws[0]) + 1), (0, 65535, 2)] + [(1, off, n) for off, n in mine] + \
        [(2, 0, 1 << 20), (2, 2999, 2), (0, len(raws[0]) - 1, 1)]
    failed = set()
    if variant == "same_size":
        raws[1] = raws[1][:lo] + new + raws[1][hi:]
    else:
        failed = {2 + k for k in touching}
    out, arr, _ = ranged(idx, t2, ranges)
    check(out, arr, ranges, raws, failed=failed)
    assert passes() == 1 and lz4ada.last_path() == OK_PATH
