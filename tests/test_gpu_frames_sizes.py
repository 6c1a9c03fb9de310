"""Exact decoded sizes of device-resident frames (lz4ada_frames_device_sizes)
and the decode laid out by them (LZ4ADA_FRAMES_EXACT): every
frame's size against the generator's plaintext and the oracle; blocks crafted
for each branch of k_block_sizes (pass 1's records added up, the wave's own
walk of RLE and literal-heavy blocks with length extensions around the 64-byte
scan step, stored blocks) against the oracle's lengths and the host statement
of the rule; frame counts around the scans; malformed chains rejected with a
reason and nothing else disturbed; a buffer of exactly the total, where the
call without the flag demands sixteen times as much; the pass count under a
byte budget; linked frames; and everything else by comparison with the call
without the flag."""
import random

import pytest
import torch

import _oracle as O
import lz4ada
import lz4frame
import test_gpu_frames_linked as L
from _lz4build import encode
from test_block_size_cpu import MALFORMED
from test_gpu_frames_batch import bad_frame, resized
from test_gpu_frames_device import (BAD_AT, NFRAMES, SENTINEL, TAIL, batch, check_jobs, laid, layout,  # noqa: F401
                                    oracle_alone, slot_cap, stats, to_device, to_host)
from test_gpu_frames_linked import batch as linked_batch, cap_and_switch  # noqa: F401

pytestmark = pytest.mark.gpu

MiB = 1 << 20
BMAX = 4 * MiB
RUNS = (63, 64, 65, 127, 128, 129)  # bytes 255 in a length extension: around one and two scan steps


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def sizes_of(t, spans, linked=False):
    return lz4ada.frames_device_sizes(t.data_ptr(), t.numel(), spans, cur_stream(), linked=linked)


def decode_exact(t, spans, linked=False):
    """Sizes, then decode_frames_tensor(exact=True) into exactly `total` bytes
    with a sentinel tail -> (decoded bytes, jobs, total); the tail and the
    input are checked."""
    before = to_host(t)
    total, _ = sizes_of(t, spans, linked)
    buf = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device=t.device)
    out, jobs = lz4ada.decode_frames_tensor(t, spans, out=buf[:total], linked=linked, exact=True)
    torch.cuda.current_stream().synchronize()
    assert out.numel() <= total
    whole = to_host(buf)
    assert whole[out.numel():] == bytes([SENTINEL]) * (total + TAIL - out.numel())  # at and beyond *out_len
    assert to_host(t) == before
    return whole[:out.numel()], jobs, total


def check_sizes(jobs, items, skip=()):
    for i, (f, raw, _) in enumerate(items):
        if i in skip:
            continue
        j = jobs[i]
        assert (j.status, j.reason, j.out_len, j.out_off, j.consumed) == (0, 0, len(raw), 0, 0), i


# ------------------------------------------------------- sizes equal lengths

@pytest.mark.parametrize("side_stream", [False, True])
def test_sizes_equal_lengths(batch, laid, side_stream):
    data, spans, t = laid  # every byte alignment: a legacy, a skippable, an empty frame, one of 40 blocks
    if side_stream:
        with torch.cuda.stream(torch.cuda.Stream()):
            total, jobs = sizes_of(t, spans)
    else:
        total, jobs = sizes_of(t, spans)
    check_sizes(jobs, batch)
    assert total == sum(len(raw) for _, raw, _ in batch)
    assert stats()["passes"] == 0 and to_host(t) == data


# ------------------------------------------------------------ crafted blocks

class Payload:
    """Sequences for _lz4build.encode with the payload position in hand."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.seqs = [(b"Z", 1, 4)]
        self.n = 4

    def add(self, lits, ml):
        L, m4 = len(lits), ml - 4
        self.seqs.append((lits, 1, ml))
        self.n += 1 + (0 if L < 15 else (L - 15) // 255 + 1) + L + 2 + (0 if m4 < 15 else (m4 - 15) // 255 + 1)

    def pad_to(self, want, lead):
        """3-byte sequences until a sequence of `lead` bytes before its length
        extension puts that extension at payload offset want mod 64."""
        while (self.n + lead) % 64 != want:
            self.add(b"", 4)


def rle_block(seed, last_run_ends_payload):
    """Every run of RUNS as a match-length extension at payload offsets 0-3 mod
    64, padded to 4,096 payload bytes and more; the ratio is over 64."""
    p = Payload(seed)
    for a in range(4):
        for run in RUNS:
            p.pad_to(a, 3)  # token, offset pair, then the extension
            at = p.n + 3
            p.add(b"", 4 + 15 + 255 * run + 7)
            assert at % 64 == a and p.n == at + run + 1
    while p.n < 4096:
        p.add(p.rng.randbytes(14), 4)
    if last_run_ends_payload:
        p.add(b"", 4 + 15 + 255 * 64 + 9)
        comp, raw = encode(p.seqs)  # the block ends after the match: its last extension byte is the payload's last
        assert comp[-1] == 9 and comp[-2] == 255
    else:
        comp, raw = encode(p.seqs, b"tail!")
    assert len(comp) >= 4096 and len(raw) > 64 * len(comp) and len(raw) <= BMAX
    return comp, raw


def literal_block(seed):
    """Literal runs with extensions of RUNS bytes 255, at payload offsets 0-3
    mod 64 in turn: 16 KiB and more of input per sequence, over 64 KiB and more
    (and under the 512 KiB from which a lone block goes another way)."""
    p = Payload(seed)
    for a, run in enumerate(RUNS):
        p.pad_to(a % 4, 1)  # the extension follows the token
        at = p.n + 1
        p.add(p.rng.randbytes(15 + 255 * run + 11), 4)
        assert at % 64 == a % 4
    comp, raw = encode(p.seqs, b"tail!")
    assert 65536 <= len(comp) < (512 << 10) and len(raw) <= BMAX
    return comp, raw


def crafted_blocks():
    """name -> (payload, decoded bytes, stored)."""
    rng = random.Random(13)
    c = {}
    # one sub-segment's sequences decode to 0xFFFF bytes and more: the record's 16-bit
    # count saturates and its high word holds the count (a payload under 4 KiB: pass 1 takes it)
    c["saturated_record"] = encode([(rng.randbytes(300), 7, 66000), (b"ab", 2, 9)], b"tail!") + (False,)
    # ... and eight sequences that start in the payload's first 32 bytes, each under 0xFFFF
    c["saturated_sum"] = encode([(b"a", 1, 4)] + [(b"", 1, 273)] * 6 + [(b"", 1, 65535 - 6 * 273 + 40)],
                                b"tail!") + (False,)
    c["rle"] = rle_block(1, False) + (False,)
    c["rle_run_ends_payload"] = rle_block(2, True) + (False,)
    c["literal_heavy"] = literal_block(3) + (False,)
    c["ends_after_match"] = encode([(b"abcdefgh", 3, 9), (b"xy", 1, 40)]) + (False,)
    c["one_byte_block"] = (b"\x00", b"", False)
    c["one_literal"] = (b"\x10A", b"A", False)
    for n in (0, 1, 65536):
        raw = rng.randbytes(n)
        c[f"stored_{n}"] = (raw, raw, True)
    return c


@pytest.fixture(scope="module")
def crafted():
    """[(name, frame, payload, stored, the oracle's bytes)]: one block per frame."""
    res = []
    for name, (comp, raw, stored) in crafted_blocks().items():
        frame, _ = lz4frame.build_frame([(comp, raw, stored)], BMAX)
        ref = oracle_alone(frame)
        assert ref == raw, name  # the builder's bytes are the reference's
        res.append((name, frame, comp, stored, ref))
    return tuple(res)


def test_crafted_blocks_reach_the_branches(crafted):
    by = {name: (comp, ref) for name, _, comp, _, ref in crafted}
    assert len(by["saturated_record"][0]) < 4096 and len(by["saturated_record"][1]) >= 0xFFFF + 300
    # DS_SPARSE by ratio: RLE_MIN_IN payload bytes, and 64 times them under the slot capacity
    for name in ("rle", "rle_run_ends_payload"):
        n = len(by[name][0])
        assert n >= 4096 and 64 * n < min(BMAX, 255 * n + 64)
    # DS_SPARSE by density: 64 KiB and more, under 128 of the first chunk's 512 sub-segments start a sequence
    n = len(by["literal_heavy"][0])
    assert n >= 65536 and 64 * n >= BMAX
    # and pass 1 says so, over the descriptors the sizes stage fills (nominal slots)
    data, spans = layout([f for _, f, _, _, _ in crafted])
    t = to_device(data)
    verdict, nblocks, descs = lz4ada.frames_index_device_debug(t.data_ptr(), t.numel(), spans)
    nb = len(crafted)
    assert list(verdict) == [lz4ada.BATCH_OK] * nb and list(nblocks) == [1] * nb
    d_desc = to_device(bytes(descs)[:nb * 32])
    d_st = torch.zeros(nb * 32, dtype=torch.uint8, device=t.device)
    tab = lz4ada.index_table_debug(t.data_ptr(), t.numel(), d_desc.data_ptr(), nb, d_st.data_ptr(), cur_stream())
    st = (lz4ada.BlockStatus * nb).from_buffer_copy(to_host(d_st))
    want = {"rle": lz4ada.DS_SPARSE, "rle_run_ends_payload": lz4ada.DS_SPARSE, "literal_heavy": lz4ada.DS_SPARSE}
    for i, (name, *_) in enumerate(crafted):
        assert st[i].code == want.get(name, 0), (name, st[i].code)
    # the saturated records: a low count of 0xFFFF, the whole count in the high word
    for i, (name, _, comp, _, ref) in enumerate(crafted):
        if name.startswith("saturated"):
            base = 64 * ((descs[i].in_off >> 8) + i)
            recs = [int.from_bytes(tab[base + 8 * k:base + 8 * k + 8], "little") for k in range((len(comp) + 31) // 32)]
            assert sum(r >> 32 for r in recs) == len(ref), name
            assert max(r >> 32 for r in recs) >= 0xFFFF, name


def test_crafted_block_sizes(crafted):
    data, spans = layout([f for _, f, _, _, _ in crafted])
    t = to_device(data)
    total, jobs = sizes_of(t, spans)
    for i, (name, frame, comp, stored, ref) in enumerate(crafted):
        assert lz4ada.block_size_host(comp, stored) == len(ref), name
        assert (jobs[i].status, jobs[i].reason, jobs[i].out_len) == (0, 0, len(ref)), name
    assert total == sum(len(ref) for *_, ref in crafted)
    out, jobs, _ = decode_exact(t, spans)
    check_jobs(out, jobs, [(f, ref, False) for _, f, _, _, ref in crafted])
    assert len(out) == total


# ----------------------------------------------------- counts around the scans

def small_frame(i, nblocks=None):
    rng = random.Random(4000 + i)
    blocks = []
    for k in range(nblocks if nblocks is not None else 1 + i % 3):
        n = rng.choice([1, 17, 40, 300, 2000]) if nblocks is None else 20 + (k * 7) % 50
        if (i + k) % 5 == 4:
            raw = rng.randbytes(n)
            blocks.append((raw, raw, True))
        else:
            blocks.append((*lz4ada.gen_block((i + k) % 2, 10 * i + k, n), False))
    return lz4frame.build_frame(blocks, 64 << 10, content_cksum=bool(i & 1), with_content_size=bool(i & 2))


@pytest.fixture(scope="module")
def small_frames():
    """257 small frames, then one of 1,025 blocks: (frame, plaintext, has checksum)."""
    items = [small_frame(i) for i in range(257)] + [small_frame(999, 1025)]
    assert lz4ada.frame_index(items[-1][0])[0].nblocks == 1025
    return tuple((f, raw, False) for f, raw in items)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, "blocks1025"])
def test_frame_counts_around_the_scans(small_frames, count):
    items = small_frames[-1:] if count == "blocks1025" else small_frames[:count]
    for f, raw, _ in items[:3]:
        assert oracle_alone(f) == raw
    data, spans = layout([f for f, _, _ in items])
    t = to_device(data)
    total, jobs = sizes_of(t, spans)
    check_sizes(jobs, items)
    assert total == sum(len(raw) for _, raw, _ in items)
    out, jobs, _ = decode_exact(t, spans)
    check_jobs(out, jobs, items)
    assert len(out) == total and stats()["passes"] == 1


def test_sizes_stage_in_chunks(small_frames, monkeypatch):
    """The stage cut into chunks of at most 64 blocks (whole frames: the frame
    of 1,025 blocks is a chunk of its own): the same sizes and bytes."""
    monkeypatch.setenv("LZ4ADA_SIZES_CHUNK_BLOCKS", "64")
    items = small_frames[:100] + small_frames[-1:] + small_frames[100:]
    data, spans = layout([f for f, _, _ in items])
    t = to_device(data)
    total, jobs = sizes_of(t, spans)
    check_sizes(jobs, items)
    assert total == sum(len(raw) for _, raw, _ in items)
    out, jobs, _ = decode_exact(t, spans)
    check_jobs(out, jobs, items)
    assert len(out) == total and stats()["passes"] == 1


# ----------------------------------------------------------------- malformed

def frame_with_middle(payload):
    good = [(*lz4ada.gen_block(1, 700 + k, 3000), False) for k in range(2)]
    return lz4frame.build_frame([good[0], (payload, b"", False), good[1]], 64 << 10)[0]


@pytest.mark.parametrize("name", sorted(MALFORMED) + ["size_plus_1", "size_minus_1"])
def test_malformed_is_rejected_with_a_reason(batch, name):
    if name in MALFORMED:
        frame, reason = frame_with_middle(MALFORMED[name]), lz4ada.DEVFRAME_BLOCK
    else:
        frame, reason = resized(1 if name == "size_plus_1" else -1), lz4ada.DEVFRAME_SIZE
    assert O.decode_stream(frame)[0] != O.OK
    items = list(batch)
    items[BAD_AT] = (frame, b"", False)
    data, spans = layout([f for f, _, _ in items])
    t = to_device(data)
    total, jobs = sizes_of(t, spans)
    check_sizes(jobs, items, skip={BAD_AT})
    j = jobs[BAD_AT]
    assert (j.status, j.reason, j.out_len, j.out_off, j.consumed) == (lz4ada.EXACT_PATH, reason, 0, 0, 0)
    assert total == sum(len(raw) for _, raw, _ in items)
    # the decode rejects it with the same reason, and it costs only itself
    out, jobs, _ = decode_exact(t, spans)
    check_jobs(out, jobs, items, skip={BAD_AT})
    j = jobs[BAD_AT]
    assert (j.status, j.reason, j.out_len, j.consumed) == (lz4ada.EXACT_PATH, reason, 0, 0)
    assert stats()["batched"] == NFRAMES - 1 and stats()["passes"] == 1


# ------------------------------------------------------- a decode that fits

def fit_frame(i):
    """A 4 MiB-block-maximum frame of one block with 1-3 KiB of payload, no
    content size.  The generator's RLE kind is left out: at this payload it
    decodes to nearly its slot capacity, and the point here is the frames
    whose capacity is far from their size."""
    kind, n = [(0, 2000), (1, 4000), (3, 2500), (4, 40000), (5, 5000), (6, 2000)][i % 6]
    n += 37 * (i % 11)
    if kind == 6:
        raw = random.Random(i).randbytes(n)
        comp, stored = raw, True
    else:
        comp, raw = lz4ada.gen_block(kind, 7000 + i, n)
        stored = False
    assert 1024 <= len(comp) <= 3072, (i, len(comp))
    return lz4frame.build_frame([(comp, raw, stored)], BMAX, block_cksum=bool(i & 1), content_cksum=bool(i & 2))


@pytest.fixture(scope="module")
def fit():
    """(items, data, spans, device tensor, nominal bound, nominal slots, tight slots); checked on the CPU."""
    items = []
    for i in range(300):
        f, raw = fit_frame(i)
        items.append((f, raw, bool(i & 2)))
    for f, raw, _ in items[:12]:
        assert oracle_alone(f) == raw
    bound = slots = tight = 0
    for f, raw, _ in items:
        v, info, descs = lz4ada.frame_walk_host(f)
        assert v == lz4ada.BATCH_OK and info.nblocks == 1 and info.block_max == BMAX
        cap = slot_cap(descs[0], info.block_max)
        bound += cap
        slots += (cap + 255) & ~255
        tight += (len(raw) + 255) & ~255
    total = sum(len(raw) for _, raw, _ in items)
    assert total * 16 < bound  # by construction of slot_cap for these payloads
    data, spans = layout([f for f, _, _ in items])
    return tuple(items), data, spans, to_device(data), bound, slots, tight


def test_decode_fits_the_total(fit):
    items, data, spans, t, bound, _, _ = fit
    total, jobs = sizes_of(t, spans)
    check_sizes(jobs, items)
    assert total == sum(len(raw) for _, raw, _ in items) and total * 16 < bound
    assert lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, cur_stream())[0] == bound
    out, jobs, _ = decode_exact(t, spans)
    check_jobs(out, jobs, items)
    assert len(out) == total
    at = 0
    for i in range(len(items)):  # dense in rising in_off
        assert jobs[i].out_off == at, i
        at += jobs[i].out_len
    assert stats()["batched"] == len(items) and stats()["passes"] == 1
    # the tensor call allocates the total, not the bound
    out2, jobs2 = lz4ada.decode_frames_tensor(t, spans, exact=True)
    assert out2.numel() == total and to_host(out2) == out
    # without the flag the same buffer is too little
    buf = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device=t.device)
    with pytest.raises(lz4ada.TooLittleMemory) as ei:
        lz4ada.decode_frames_device(t.data_ptr(), t.numel(), spans, buf.data_ptr(), total, cur_stream())
    torch.cuda.synchronize()
    assert ei.value.bound == bound
    assert to_host(buf) == bytes([SENTINEL]) * (total + TAIL)
    # and with it, one byte less is too: the total is reported, nothing is written
    with pytest.raises(lz4ada.TooLittleMemory) as ei:
        lz4ada.decode_frames_device(t.data_ptr(), t.numel(), spans, buf.data_ptr(), total - 1, cur_stream(),
                                    exact=True)
    torch.cuda.synchronize()
    assert ei.value.bound == total and stats()["passes"] == 0
    assert to_host(buf) == bytes([SENTINEL]) * (total + TAIL)


def test_passes_split_by_the_tight_slots(fit, monkeypatch):
    items, data, spans, t, bound, slots, tight = fit
    budget = 8 * MiB
    assert tight < budget < slots  # and no frame's capacity alone is over it
    assert 255 * 3072 + 64 + 255 <= budget
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(budget))
    out, jobs, total = decode_exact(t, spans)
    check_jobs(out, jobs, items)
    assert stats()["passes"] == 1 and stats()["batched"] == len(items)
    buf = torch.empty(bound, dtype=torch.uint8, device=t.device)
    plain, jobs0 = lz4ada.decode_frames_tensor(t, spans, out=buf)
    assert stats()["passes"] > 1 and stats()["batched"] == len(items)
    assert to_host(plain) == out


# --------------------------------------------------------------- linked frames

def job_view(j):
    return (j.in_off, j.in_len, j.out_len, j.consumed, j.status, j.reason)


def test_linked_frames_as_without_the_flag(linked_batch):
    short_middle, raw = L.linked_frame([65536, 30000, 65536, 100], seed=5)
    st, ref, msg = L.oracle(short_middle)
    assert st == O.OK and ref == raw
    items = linked_batch + ((short_middle, st, ref, msg, "short"),)
    plain, jobs0, data = L.decode_device(items, True)
    path0 = lz4ada.last_path()
    s0 = lz4ada.last_batch_stats()
    spans = [(j.in_off, j.in_len) for j in jobs0]
    t = to_device(data)
    out, jobs, total = decode_exact(t, spans, linked=True)
    s1 = lz4ada.last_batch_stats()
    assert lz4ada.last_path() == path0 == lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT | lz4ada.PATH_LINKED
    assert (s1.frames_batched, s1.passes) == (s0.frames_batched, s0.passes)
    for i, (f, st, ref, msg, kind) in enumerate(items):
        assert job_view(jobs[i]) == job_view(jobs0[i]), (i, kind)
        a, b = jobs0[i], jobs[i]
        assert out[b.out_off:b.out_off + b.out_len] == plain[a.out_off:a.out_off + a.out_len], (i, kind)
        if kind in ("indep", "linked"):
            assert b.status == 0 and out[b.out_off:b.out_off + b.out_len] == ref, (i, kind)
        else:  # a D1 frame, a corrupt block checksum, a short middle block: the single way
            assert (b.status, b.reason) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK), (i, kind)
    _, sized = sizes_of(t, spans, linked=True)
    assert (sized[len(items) - 1].status, sized[len(items) - 1].reason) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK)
    for i, (f, st, ref, msg, kind) in enumerate(items):
        if kind in ("indep", "linked"):
            assert (sized[i].status, sized[i].out_len) == (0, len(ref)), (i, kind)


# ------------------------------------------------- everything else, by comparison

def test_same_results_as_without_the_flag(batch, monkeypatch):
    monkeypatch.setenv("LZ4ADA_BATCH_HASH_MAX", "4096")  # frames above it: the host chain
    items = list(batch)
    items[BAD_AT] = (bad_frame("content_checksum"), b"", True)
    data, spans = layout([f for f, _, _ in items])
    t = to_device(data)
    bound, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, cur_stream())
    plain, jobs0 = lz4ada.decode_frames_tensor(t, spans, out=torch.empty(bound, dtype=torch.uint8, device=t.device))
    plain, s0 = to_host(plain), stats()
    out, jobs, total = decode_exact(t, spans)
    assert stats() == s0 and s0["host"] > 0 and s0["gpu"] > 0
    assert out == plain
    for i in range(NFRAMES):
        a, b = jobs0[i], jobs[i]
        assert job_view(a) + (a.out_off,) == job_view(b) + (b.out_off,), i
    check_jobs(out, jobs, items, skip={BAD_AT})
    j = jobs[BAD_AT]
    assert (j.status, j.reason, j.out_len, j.consumed) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_CHECKSUM, 0, 0)
    # the checksum-mismatch frame has a size: its chains are good
    info, descs = lz4ada.frame_index(items[BAD_AT][0])
    bad_size = sum(lz4ada.block_size_host(items[BAD_AT][0][d.in_off:d.in_off + d.in_len])
                   for d in descs[:info.nblocks])
    assert bad_size == 2 * 65536 + 1000
    assert total == sum(len(raw) for _, raw, _ in items) + bad_size


def test_misuse_is_judged_as_in_the_other_calls(laid):
    data, spans, t = laid
    past = list(spans)
    past[-1] = (len(data) - 5, 10)
    overlapping = list(spans)
    overlapping[5] = (spans[5][0], spans[6][0] + 10 - spans[5][0])
    for bad in (past, overlapping, [(-1, 8)] + spans[1:]):
        with pytest.raises(lz4ada.AssertionFailure):
            sizes_of(t, bad)
    total, jobs = lz4ada.frames_device_sizes(0, 0, [])
    assert total == 0
