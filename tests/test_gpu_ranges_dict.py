"""Seek index over dictionary frames (lz4ada_seek_index_build_dict, DESIGN.md
§19): ranged decode against the dictionary the index was built with.  The
reference for every byte is lz4ada.decode_frame_dict_host(frame, dict) sliced
to the clipped range.  Dictionary lengths and alignments over every block
boundary; the reach of a match into the dictionary; chains from the dictionary
beside chains from checkpoints in one launch; liblz4's fixtures; a mixed index
with every verdict; the compressor's frames read back by position; the index's
own copy of the dictionary; the byte budget; the build without a dictionary;
the size formula; an input that changed after the build; the chain decoder
alone."""
import ctypes
import json
import os
import random
import struct

import pytest
import torch
import xxhash

import lz4ada
import lz4frame
from _compress_cases import pseudo_text
from conftest import GOLDEN, read_vector
from test_gpu_frames_device import oracle_alone, to_host
from test_gpu_frames_dict import dict_bytes, hand_frame, indep_frame, layout, linked_frame, to_device
from test_gpu_ranges import check, clip, ranged
from test_gpu_ranges_linked import boundary_ranges

pytestmark = pytest.mark.gpu

KiB = 1024
BLOCK_FAILED = (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK)
DICT_DIR = os.path.join(GOLDEN, "lz4f_dict")
BLOCK_SIZES = [1, 63, 64, 4096, 65535, 65536]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.delenv("LZ4ADA_BATCH_LINKED", raising=False)
    monkeypatch.delenv("LZ4ADA_BATCH_BYTES", raising=False)


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def passes():
    return lz4ada.last_batch_stats().passes


def host(frame, d):
    return lz4ada.decode_frame_dict_host(frame, d or b"")[0]


def build(frames, d, at=0, **kw):
    """The frames and the dictionary (`at` bytes into its allocation) on the
    device and the index over them -> (frames tensor, index, dictionary tensor)."""
    data, spans = layout(frames)
    t, dt = to_device(data), (to_device(d, at) if d is not None else None)
    return t, lz4ada.SeekIndex.build_tensor(t, spans, dict=dt, **kw), dt


def index_bytes(nb, n, dict_len=None, ckpts=None):
    """lz4ada_seek_index_bytes by the header's formula.  nb: the blocks of the
    accepted frames; n: the jobs; ckpts None: built without LZ4ADA_SEEK_LINKED;
    dict_len None: built without a dictionary."""
    total = 32 * nb + 8 * (n + 1) + 16 * (nb + n)
    if ckpts is not None:
        total += 65536 * ckpts + 8 * (n + 1) + 8 * n
    if dict_len:
        used = min(dict_len, 65536)
        total += (used + 32 + 255) // 256 * 256 + 8 * n
    return total


def end_ranges(lens, job):
    size = sum(lens)
    return boundary_ranges(lens, job) + [(job, 0, 1), (job, size - 1, 1), (job, 0, size), (job, size - 1, 5)]


# ------------------------------------------------- dictionary lengths and edges

_EDGES = {}


def edges_case(dict_len):
    """Six independent single-block frames and one of three 64 KiB blocks under
    a dictionary of dict_len bytes -> (dictionary, frames, the host decoder's
    bytes, block lengths per frame, shuffled ranges with repeats and overlaps).
    Made once per length and never modified."""
    if dict_len not in _EDGES:
        d = dict_bytes(dict_len, seed=dict_len)
        frames, lens = [], []
        for k, n in enumerate(BLOCK_SIZES):
            f, p = indep_frame([n], d, 100 + k, content_cksum=bool(k & 1), block_cksum=bool(k & 2))
            assert host(f, d) == p
            frames.append(f), lens.append([n])
        f, p = indep_frame([65536, 65536, 65536], d, 200, block_cksum=True)
        assert host(f, d) == p
        frames.append(f), lens.append([65536] * 3)
        raws = [host(f, d) for f in frames]
        ranges = [r for job, ln in enumerate(lens) for r in end_ranges(ln, job)]
        rng = random.Random(dict_len)
        ranges += rng.sample(ranges, 12)  # repeats
        rng.shuffle(ranges)
        _EDGES[dict_len] = (d, tuple(frames), tuple(raws), tuple(lens), tuple(ranges))
    return _EDGES[dict_len]


@pytest.mark.parametrize("dict_len", [1, 4, 255, 256, 257, 65535, 65536, 65537, 100000])
def test_dictionary_lengths_and_edges(dict_len):
    d, frames, raws, lens, ranges = edges_case(dict_len)
    for at in (0, 3):
        t, idx, _ = build(frames, d, at=at)
        with idx:
            assert all((j.status, j.reason, j.out_len) == (0, 0, len(raws[i])) for i, j in enumerate(idx.jobs[:7]))
            assert idx.device_bytes == index_bytes(9, 7, dict_len)
            out, arr, _ = ranged(idx, t, list(ranges))
            check(out, arr, ranges, raws)
            assert passes() == 1
            assert lz4ada.last_path() == lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT


# ------------------------------------------------------------------------ reach

@pytest.mark.parametrize("dict_len", [1000, 65534, 65536])
def test_reach_into_the_dictionary(dict_len):
    """A match exactly dict_used back from the block start is delivered, one
    byte further fails its range alone.  With 65,536 used bytes the format's
    largest offset, 65,535, is the farthest a match at position 0 reaches, so
    there the failing side cannot be written down and 65,534 stands in for it."""
    d = dict_bytes(dict_len, seed=77)
    used = min(dict_len, 65536)
    far = min(used, 65535)
    frames, plains = [], []
    f, p = hand_frame([(b"", far, 8)], b"end..", d, content_cksum=True)
    assert p[:8] == d[-far:][:8] and host(f, d) == p
    frames.append(f), plains.append(p)
    if used + 1 <= 65535:
        f, p = hand_frame([(b"", used + 1, 8)], b"end..", d)
        assert p is None
        with pytest.raises(lz4ada.DataCorruption):
            host(f, d)
        frames.append(f), plains.append(b"?" * 13)  # (its size: 8 + 5, known without decoding)
    f, p = hand_frame([(b"ab", 50, 9)], b"tail.", d, content_cksum=True)
    frames.append(f), plains.append(p)
    t, idx, _ = build(frames, d, at=3)
    with idx:
        assert all(j.status == 0 for j in idx.jobs[:len(frames)])  # the sizes stage decodes nothing
        ranges = [(j, 0, 100) for j in range(len(frames))] + [(j, 3, 4) for j in range(len(frames))]
        failed = [i for i, r in enumerate(ranges) if len(frames) == 3 and r[0] == 1]
        out, arr, _ = ranged(idx, t, ranges)
        check(out, arr, ranges, plains, failed=failed)


# ------------------------------------------- two history lengths in one launch

@pytest.mark.parametrize("dict_len", [1000, 65536])
def test_chains_from_the_dictionary_and_from_checkpoints(dict_len):
    d = dict_bytes(dict_len, seed=31)
    lens = [65536] * 5
    f, p = linked_frame(lens, d, 41, content_cksum=True)
    assert host(f, d) == p
    ranges = boundary_ranges(lens)
    for every, ckpts in ((1, 4), (131072, 2), (0, 0)):  # K = 1, K = 2, the default: no head
        t, idx, _ = build([f], d, at=1, linked=True, checkpoint_bytes=every)
        with idx:
            assert (idx.jobs[0].status, idx.jobs[0].reason, idx.jobs[0].out_len) == (0, 0, len(p))
            assert idx.device_bytes == index_bytes(5, 1, dict_len, ckpts)
            out, arr, _ = ranged(idx, t, ranges)
            check(out, arr, ranges, [p])
            assert passes() == 1  # one pass: a chain from block 0 beside the chains from heads
            assert lz4ada.last_path() == lz4ada.PATH_BATCH | lz4ada.PATH_LINKED


# --------------------------------------------------------------------- fixtures

def test_liblz4_fixtures():
    with open(os.path.join(DICT_DIR, "manifest.json")) as fh:
        m = json.load(fh)
    seen = 0
    for name, info in m["dicts"].items():
        with open(os.path.join(DICT_DIR, info["file"]), "rb") as fh:
            d = fh.read()
        mine = [f for f in m["frames"] if f["dict"] == name]
        frames = []
        for f in mine:
            with open(os.path.join(DICT_DIR, f["file"]), "rb") as fh:
                frames.append(fh.read())
        seen += len(frames)
        raws = [host(f, d) for f in frames]
        rng = random.Random(len(d))
        ranges = []
        for job, raw in enumerate(raws):
            size = len(raw)
            ranges += [(job, 0, size), (job, 0, 1), (job, max(size - 1, 0), 1)]
            for _ in range(20):
                off = rng.randrange(size + 1)
                ranges.append((job, off, rng.randrange(1, min(size, 70000) + 2)))
        t, idx, _ = build(frames, d, at=1, linked=True)
        with idx:
            for f, j in zip(mine, idx.jobs):
                assert (j.status, j.reason, j.out_len) == (0, 0, f["size"]), f["file"]
            out, arr, _ = ranged(idx, t, ranges)
            check(out, arr, ranges, raws)
            for job, f in enumerate(mine):  # the whole frames against the manifest
                r = arr[ranges.index((job, 0, f["size"]))]
                assert r.out_len == f["size"]
                assert xxhash.xxh32(out[r.out_off:r.out_off + r.out_len]).intdigest() == f["xxh32"], f["file"]
    assert seen == 42


# ---------------------------------------------------------------- a mixed index

def skippable(payload):
    return struct.pack("<II", 0x184D2A53, len(payload)) + payload


MIXED_DICT_LEN = 30000


@pytest.fixture(scope="module")
def mixed():
    """(dictionary, frames, expected bytes, {job: reason of a frame the index
    does not take}, blocks of the accepted frames); never modified."""
    d = dict_bytes(MIXED_DICT_LEN, seed=17)
    frames, raws = [], []
    for k, lens in enumerate(([3000], [65536, 500], [1024])):
        f, p = indep_frame(lens, d, 900 + k, content_cksum=True, block_cksum=bool(k & 1))
        frames.append(f), raws.append(p)
    f, p = linked_frame([65536, 65536, 65536, 700], d, 950, content_cksum=True)
    frames.append(f), raws.append(p)
    frames.append(read_vector("z100legacy", "lz4")), raws.append(oracle_alone(frames[-1]))
    frames.append(skippable(b"between")), raws.append(b"")
    frames.append(lz4frame.build_frame([], 64 * KiB, content_cksum=True)[0]), raws.append(b"")
    blocks = lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, 300, 0, 0, lens=[2000], hist=d)
    f, p = lz4frame.build_frame([(c, r, False) for c, r in blocks], 64 * KiB, content_cksum=True, dict_id=8)
    frames.append(f), raws.append(p)  # names another dictionary
    f, p = indep_frame([5000], d, 960)
    frames.append(f[:len(f) - 40]), raws.append(p)  # cut short
    for i in (0, 1, 2, 3):
        assert host(frames[i], d) == raws[i]
    reasons = {7: lz4ada.DEVFRAME_DICT, 8: lz4ada.BATCH_NOT_INDEXED}
    return d, tuple(frames), tuple(raws), reasons, 1 + 2 + 1 + 4 + 1


def mixed_ranges(raws):
    ranges = []
    for job, raw in enumerate(raws):
        size = len(raw)
        ranges += [(job, 0, size), (job, size // 2, 300), (job, max(size - 1, 0), 9), (job, 0, 1)]
    ranges += boundary_ranges([65536, 65536, 65536, 700], job=3, sizes=(1, 65537))
    random.Random(5).shuffle(ranges)
    return ranges


def test_mixed_index(mixed):
    d, frames, raws, reasons, nb = mixed
    t, idx, _ = build(frames, d, at=3, linked=True, checkpoint_bytes=131072, dict_id=7)
    with idx:
        for job in range(len(frames)):
            j = idx.jobs[job]
            if job in reasons:
                assert (j.status, j.reason, j.out_len) == (lz4ada.EXACT_PATH, reasons[job], 0), job
            else:
                assert (j.status, j.reason, j.out_len) == (0, 0, len(raws[job])), job
        # the frame with another id and the one cut short hold no block
        assert idx.device_bytes == index_bytes(nb, len(frames), MIXED_DICT_LEN, ckpts=1)
        ranges = mixed_ranges(raws)
        out, arr, total = ranged(idx, t, ranges)  # (the guard region behind *out_len, the input)
        check(out, arr, ranges, raws, reasons=reasons)
        assert passes() == 1
        guard = torch.full((total + 512,), 0x5A, dtype=torch.uint8, device="cuda")
        with pytest.raises(lz4ada.TooLittleMemory) as e:
            lz4ada.decode_ranges_device(idx, t.data_ptr(), t.numel(), ranges, guard.data_ptr(), total - 1, cur_stream())
        assert e.value.bound == total and passes() == 0
        torch.cuda.synchronize()
        assert to_host(guard) == bytes([0x5A]) * (total + 512)


# -------------------------------------------------- the write side closes the loop

def test_compressed_records_by_position():
    ident = 0xC0FFEE42
    text = pseudo_text(65536 + 64 * KiB + 300000, 19)
    d = text[:65536]
    lens = [KiB] * 64 + [300000]
    spans, at = [], 65536
    for n in lens:
        spans.append((at, n))
        at += n
    t, dt = to_device(text), to_device(d, 3)
    frames, fspans = lz4ada.compress_frames_tensor(t, spans, dict=dt, dict_id=ident)
    frames = frames.contiguous()
    fbytes = to_host(frames)
    records = [text[o:o + n] for o, n in spans]
    for (o, n), rec in list(zip(fspans, records))[::16]:
        assert host(fbytes[o:o + n], d) == rec
    ranges = [(job, off, n) for job in range(65) for off, n in ((0, lens[job]), (lens[job] // 3, 200), (lens[job] - 1, 1))]
    ranges += boundary_ranges([65536] * 4 + [300000 - 4 * 65536], job=64, sizes=(1, 65537))
    random.Random(6).shuffle(ranges)
    idx = lz4ada.SeekIndex.build(frames.data_ptr(), frames.numel(), fspans, cur_stream(), dict=dt.data_ptr(),
                                 dict_len=len(d), dict_id=ident)
    with idx:
        assert all((j.status, j.out_len) == (0, lens[i]) for i, j in enumerate(idx.jobs[:65]))
        out, arr, _ = ranged(idx, frames, ranges)
        check(out, arr, ranges, records)
    # the same frames without a dictionary: a block that references it fails its range
    pick = None
    for job, (o, n) in enumerate(fspans[:64]):
        try:
            differs = host(fbytes[o:o + n], b"") != records[job]
        except lz4ada.LZ4AdaError:
            differs = True
        if differs:
            pick = job
            break
    assert pick is not None
    with lz4ada.SeekIndex.build_tensor(frames, fspans) as plain:
        ranges = [(pick, 0, KiB), (pick, 100, 10)]
        out, arr, _ = ranged(plain, frames, ranges)
        check(out, arr, ranges, records, failed=(0, 1))


# ------------------------------------------------ the index owns the dictionary

def test_the_index_owns_its_dictionary():
    d, frames, raws, lens, ranges = edges_case(257)
    t, idx, dt = build(frames, d, at=3)
    with idx:
        dt.zero_()
        torch.cuda.synchronize()
        lz4ada.release_device_cache()
        out, arr, _ = ranged(idx, t, list(ranges))
        check(out, arr, ranges, raws)


# ----------------------------------------------------------------------- budget

def test_gaps_are_charged_to_the_budget(monkeypatch):
    d = dict_bytes(65536, seed=53)
    frames, raws = [], []
    for k in range(12):
        f, p = indep_frame([KiB], d, 700 + k, content_cksum=True)
        frames.append(f), raws.append(p)
    frames.append(read_vector("z100legacy", "lz4")), raws.append(oracle_alone(frames[-1]))
    need = KiB + 65792  # one record's slot and the gap in front of it
    assert len(raws[12]) <= need - 1 - 256
    t, idx, _ = build(frames, d)
    ranges = [(job, off, n) for job in range(13) for off, n in ((0, KiB), (500, 24))]
    random.Random(8).shuffle(ranges)
    with idx:
        for budget in (need + 1, need):
            monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(budget))
            out, arr, _ = ranged(idx, t, ranges)
            check(out, arr, ranges, raws)
            assert passes() >= 24  # a pass holds one record's range; the legacy frame's ride where they fit
        monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(need - 1))
        out, arr, _ = ranged(idx, t, ranges)
        at = 0
        for i, (job, off, n) in enumerate(ranges):
            want = clip(len(raws[job]), off, n)
            assert arr[i].out_off == at
            if job == 12:
                assert (arr[i].status, arr[i].reason, arr[i].out_len) == (0, 0, want)
                assert out[at:at + want] == raws[job][off:off + want]
            else:  # in place
                assert (arr[i].status, arr[i].reason, arr[i].out_len) == (lz4ada.EXACT_PATH, lz4ada.BATCH_OVER_BUDGET, 0)
            at += want


# ------------------------------------------------- no dictionary is the old call

def test_no_dictionary_is_the_opt_build():
    frames, raws = [], []
    for k, lens in enumerate(([3000], [65536, 500])):
        blocks = [(*lz4ada.gen_block(1, 800 + 7 * k + i, n), False) for i, n in enumerate(lens)]
        f, p = lz4frame.build_frame(blocks, 64 * KiB, content_cksum=True)
        frames.append(f), raws.append(p)
    f, p = linked_frame([65536, 65536, 900], b"", 810, content_cksum=True)
    frames.append(f), raws.append(p)
    frames.append(read_vector("z100legacy", "lz4")), raws.append(oracle_alone(frames[-1]))
    frames.append(skippable(b"xyz")), raws.append(b"")
    data, spans = layout(frames)
    t, dt = to_device(data), to_device(b"xyz")
    ranges = mixed_ranges(raws)[:30] + boundary_ranges([65536, 65536, 900], job=2)
    opt = lz4ada.SeekOptions(lz4ada.SEEK_LINKED, 0, 65536)

    def report(jobs):
        return [(j.out_off, j.out_len, j.consumed, j.status, j.reason) for j in jobs[:len(spans)]]

    def run(dd, entry):
        jobs, ptr = lz4ada._device_jobs(spans), ctypes.c_void_p()
        args = [t.data_ptr(), t.numel(), jobs, len(spans), ctypes.byref(opt)]
        args += [None if dd is None else ctypes.byref(dd)] if entry == "dict" else []
        st = getattr(lz4ada._lib, "lz4ada_seek_index_build_" + entry)(*args, ctypes.byref(ptr), cur_stream())
        assert st == 0
        built = passes()
        with lz4ada.SeekIndex(ptr.value, jobs, len(spans), t.numel()) as idx:
            out, arr, _ = ranged(idx, t, ranges)
            check(out, arr, ranges, raws)
            recs = [(r.out_off, r.out_len, r.status, r.reason) for r in arr[:len(ranges)]]
            return report(jobs), idx.device_bytes, built, out, recs, passes(), lz4ada.last_path()

    want = run(None, "opt")
    assert want[1] == index_bytes(1 + 2 + 3 + 1, 5, None, ckpts=2)
    for dd in (None, lz4ada.DeviceDict(None, 0, 0, 0), lz4ada.DeviceDict(dt.data_ptr(), 0, 5, lz4ada.DICT_CHECK_ID)):
        assert run(dd, "dict") == want


def test_misuse_builds_nothing():
    d = dict_bytes(100)
    f, _ = indep_frame([500], d, 3)
    data, spans = layout([f])
    t, dt = to_device(data), to_device(d)
    for dd in (lz4ada.DeviceDict(dt.data_ptr(), -1, 0, 0), lz4ada.DeviceDict(None, 5, 0, 0),
               lz4ada.DeviceDict(dt.data_ptr(), dt.numel(), 0, 2)):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.SeekIndex.build(t.data_ptr(), t.numel(), spans, cur_stream(), dict=dd)
        assert passes() == 0


# ------------------------------------------------- input changed after the build

def test_input_changed_after_the_build():
    d, frames, raws, lens, ranges = edges_case(4)
    data, spans = layout(frames)
    _, descs = lz4ada.frame_index(frames[6])
    flip = spans[6][0] + descs[1].in_off + descs[1].in_len // 2  # a payload byte of its second block
    t, dt = to_device(data), to_device(d)
    with lz4ada.SeekIndex.build_tensor(t, spans, dict=dt) as idx:
        t[flip] ^= 0x20
        torch.cuda.synchronize()
        out, arr, _ = ranged(idx, t, list(ranges))  # (the guard region behind *out_len)
        at = 0
        for i, (job, off, n) in enumerate(ranges):
            want = clip(len(raws[job]), off, n)
            assert arr[i].out_off == at
            touches = job == 6 and off < 2 * 65536 and off + want > 65536
            good = (arr[i].status, arr[i].reason, arr[i].out_len) == (0, 0, want) and \
                out[at:at + want] == raws[job][off:off + want]
            if touches:
                assert (arr[i].status, arr[i].reason, arr[i].out_len) in ((*BLOCK_FAILED, 0), (0, 0, want)), i
                assert not good or want == 0, i
            else:
                assert good, i
            at += want


# ------------------------------------------------------- the chain decoder alone

def r256(v):
    return (v + 255) & ~255


def test_chain_decoder_takes_the_history_from_the_record():
    """k_index + k_decode_idx_chains through lz4ada_decode_idx_chains_debug: in
    one launch a chain of three blocks under 1,000 bytes of history, chains of
    one block under 65,536, a history length past the format's reach (clamped:
    its gap is too small for anything else), and the two chains the kernel must
    refuse -- a first block without a gap, and one that lies less than its gap
    into the slots.  Nothing outside the decoded slots is written."""
    canary = 0xA5
    d1, d2 = dict_bytes(1000, seed=61), dict_bytes(65536, seed=62)
    gen = lambda seed, lens, h: lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, seed, 0, 0, lens=lens, hist=h)
    w, yc, x, z, y = gen(1, [400], d1), gen(2, [5000], d2), gen(3, [65536, 65536, 300], d1), gen(4, [700], b""), \
        gen(5, [4096], d2)
    data, descs, plains, hist_at = b"", [], [], []

    def place(blocks, out_off, h):
        nonlocal data
        for comp, raw in blocks:
            descs.append(lz4ada.BlockDesc(len(data), len(comp), 0, out_off, len(raw), 0))
            plains.append(raw)
            data += comp
            out_off += len(raw)  # (a chain's slots continue each other)
        hist_at.append((descs[-len(blocks)].out_off, h))
        return r256(out_off)

    at = place(w, 256, b"")  # gapped by its record, but only 256 bytes into the slots
    at = place(yc, at + 65792, d2)
    assert 65792 <= descs[1].out_off < r256(100000 + 32)  # room for 65,536 bytes of history and no more
    at = place(x, at + 1280, d1)
    at = place(z, at, b"")  # no gap
    at = place(y, at + 65792, d2)
    out = bytearray([canary]) * (at + 4096)
    for off, h in hist_at:
        out[off - len(h):off] = h
    before = bytes(out)
    chains = [(0, 1, 1000, True), (1, 1, 100000, True), (2, 3, 1000, True), (5, 1, 0, False), (6, 1, 65536, True)]
    arr = (lz4ada.BlockDesc * len(descs))(*descs)
    d_in, d_out = to_device(data), torch.frombuffer(out, dtype=torch.uint8).to("cuda")
    d_st = torch.zeros(32 * len(descs), dtype=torch.uint8, device="cuda")
    lz4ada.decode_idx_chains_debug(d_in.data_ptr(), len(data), arr, len(descs), chains, d_out.data_ptr(),
                                   d_st.data_ptr(), cur_stream())
    st = (lz4ada.BlockStatus * len(descs)).from_buffer_copy(to_host(d_st))
    got = to_host(d_out)
    want = bytearray(before)
    for b in (1, 2, 3, 4, 6):
        assert (st[b].code, st[b].out_len) == (0, len(plains[b])), b
        want[descs[b].out_off:descs[b].out_off + len(plains[b])] = plains[b]
    assert st[0].code != 0 and st[5].code != 0
    assert got == bytes(want)  # the decoded slots, and not a byte besides: gaps, refused slots, canaries
