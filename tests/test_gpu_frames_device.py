"""Many frames from device memory to device memory
(lz4ada_decode_frames_device): the frames are indexed where they lie, at
every byte alignment, and decoded into the caller's device buffer -- every
frame's bytes, extent and verdict against the generator's plaintext and the
oracle, on the default and on a side stream; the index kernels against the
host walk; one bad frame among 70 costs only itself and gets a reason, not a
text; the output bound, the sentinel behind it and the untouched input; API
misuse; the byte budget; content checksums above G."""
import os
import random
import struct

import pytest
import torch

import _oracle as O
import lz4ada
import lz4frame
from conftest import VECTORS, read_vector
from test_gpu_frames_batch import SIZES, bad_frame, make_frame, three_blocks

pytestmark = pytest.mark.gpu

NFRAMES = 70    # more than one wave of the walk (64 frames)
MANY_AT = 33    # the frame of 40 blocks
LEGACY_AT, SKIP_AT = 10, 20
BAD_AT = 37     # where the rejection cases put their frame
SENTINEL = 0xA5
TAIL = 4096
OK_PATH = lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


def oracle_alone(frame: bytes) -> bytes:
    st, out, _, msg = O.decode_stream(frame, out_cap=4 << 20)
    assert st == O.OK, msg
    return out


@pytest.fixture(scope="module")
def batch():
    """[(frame, plaintext, has content checksum)] * 70; never modified.  The
    plaintext is the generator's and was checked against the oracle."""
    out = []
    for i in range(NFRAMES):
        if i == LEGACY_AT:
            f = read_vector("z100legacy", "lz4")
            out.append((f, oracle_alone(f), False))
        elif i == SKIP_AT:
            out.append((struct.pack("<II", 0x184D2A57, 21) + bytes(range(21)), b"", False))
        else:
            f, raw = make_frame(i, [65536] * 39 + [777] if i == MANY_AT else None)
            assert oracle_alone(f) == raw
            out.append((f, raw, bool(i & 2)))
    assert any(len(raw) == 0 and f[:4] == b"\x04\x22\x4d\x18" for f, raw, _ in out)  # an empty frame
    assert {len(raw) for _, raw, _ in out} >= set(SIZES)
    assert lz4ada.frame_index(out[MANY_AT][0])[0].nblocks == 40
    return tuple(out)


def layout(frames, junk=True):
    """The frames in one buffer with 0-3 junk bytes in front of each ->
    (buffer, [(in_off, in_len)])."""
    rng = random.Random(77)
    parts, spans, at = [], [], 0
    for i, f in enumerate(frames):
        gap = bytes(rng.randrange(1, 256) for _ in range((i * 3 + 1) % 4)) if junk else b""
        parts += [gap, f]
        spans.append((at + len(gap), len(f)))
        at += len(gap) + len(f)
    return b"".join(parts), spans


def to_device(data: bytes):
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t


def to_host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def stats():
    s = lz4ada.last_batch_stats()
    return dict(batched=s.frames_batched, single=s.frames_single, passes=s.passes,
                gpu=s.gpu_hashed, host=s.host_hashed)


def decode_guarded(t, spans):
    """decode_frames_tensor into a buffer with a sentinel tail behind the bound
    -> (decoded bytes, jobs, bound); the tail and the input are checked."""
    before = to_host(t)
    bound, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans,
                                          torch.cuda.current_stream().cuda_stream)
    buf = torch.full((bound + TAIL,), SENTINEL, dtype=torch.uint8, device=t.device)
    out, jobs = lz4ada.decode_frames_tensor(t, spans, out=buf[:bound])
    torch.cuda.current_stream().synchronize()
    assert out.data_ptr() == buf.data_ptr() and out.numel() <= bound
    whole = to_host(buf)
    assert whole[bound:] == bytes([SENTINEL]) * TAIL
    assert whole[out.numel():bound] == bytes([SENTINEL]) * (bound - out.numel())  # not written
    assert to_host(t) == before
    return whole[:out.numel()], jobs, bound


def check_jobs(out, jobs, items, skip=()):
    """Every job but `skip`: OK, its extent, its bytes; spans ordered and disjoint."""
    end = 0
    for i, (f, raw, _) in enumerate(items):
        j = jobs[i]
        if i in skip:
            continue
        assert (j.status, j.reason, j.consumed, j.out_len) == (0, 0, len(f), len(raw)), i
        assert j.out_off >= end, i
        end = j.out_off + j.out_len
        assert out[j.out_off:end] == raw, i
    assert end <= len(out)


# ------------------------------------------------------------------ parity

@pytest.fixture(scope="module")
def laid(batch):
    data, spans = layout([f for f, _, _ in batch])
    assert {off & 3 for off, _ in spans} == {0, 1, 2, 3}
    return data, spans, to_device(data)


@pytest.mark.parametrize("side_stream", [False, True])
def test_parity(batch, laid, side_stream):
    data, spans, t = laid
    if side_stream:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out, jobs, bound = decode_guarded(t, spans)
    else:
        out, jobs, bound = decode_guarded(t, spans)
    check_jobs(out, jobs, batch)
    assert len(out) == sum(len(raw) for _, raw, _ in batch) <= bound  # no holes: every frame is good
    assert lz4ada.last_path() == OK_PATH
    assert stats() == dict(batched=NFRAMES, single=0, passes=1, host=0,
                           gpu=sum(1 for _, _, ck in batch if ck))


def test_parity_whatever_follows(batch):
    """Back to back, every job's range running to the end of the input."""
    data, spans = layout([f for f, _, _ in batch], junk=False)
    t = to_device(data)
    out, jobs, _ = decode_guarded(t, [(off, len(data) - off) for off, _ in spans])
    check_jobs(out, jobs, batch)
    # ... as long as no accepted frame reaches into the next job's range: job 5
    # now starts 10 bytes into frame 4
    inside = [(off, len(data) - off) for off, _ in spans]
    assert spans[4][1] > 10
    inside[5] = (spans[4][0] + 10, len(data) - spans[4][0] - 10)
    with pytest.raises(lz4ada.AssertionFailure):
        lz4ada.decode_frames_tensor(t, inside)
    assert stats()["passes"] == 0


def test_allocates_from_the_bound(batch, laid):
    _, spans, t = laid
    out, jobs = lz4ada.decode_frames_tensor(t, spans)
    check_jobs(to_host(out), jobs, batch)
    # jobs in any order: the same spans, whichever job asks for them
    order = list(range(NFRAMES))
    random.Random(5).shuffle(order)
    out2, shuffled = lz4ada.decode_frames_tensor(t, [spans[i] for i in order])
    assert to_host(out2) == to_host(out)
    for k, i in enumerate(order):
        a, b = jobs[i], shuffled[k]
        assert (a.in_off, a.out_off, a.out_len, a.consumed, a.status, a.reason) == \
            (b.in_off, b.out_off, b.out_len, b.consumed, b.status, b.reason), i


# ------------------------------------------------------------------- index

def slot_cap(d, block_max):
    return d.in_len if d.flags & lz4ada.BLOCK_STORED else min(block_max, 255 * d.in_len + 64)


def check_index(data, spans, t, order=None):
    """The index kernels against the host walk, job by job; the descriptors
    rebased as documented: in_off absolute, out_off the slot layout."""
    order = list(range(len(spans))) if order is None else order
    verdict, nblocks, descs = lz4ada.frames_index_device_debug(t.data_ptr(), t.numel(),
                                                               [spans[i] for i in order])
    verdict = {i: verdict[k] for k, i in enumerate(order)}
    nblocks = {i: nblocks[k] for k, i in enumerate(order)}
    at, slot_at = 0, 0
    for i, (off, n) in enumerate(spans):  # rising in_off: the pass order
        v, info, host = lz4ada.frame_walk_host(data[off:off + n])
        assert verdict[i] == v, i
        assert nblocks[i] == (0 if v == lz4ada.BATCH_NOT_INDEXED else info.nblocks), i
        if v != lz4ada.BATCH_OK:
            continue
        for k in range(info.nblocks):
            d, h = descs[at + k], host[k]
            cap = slot_cap(h, info.block_max)
            assert (d.in_off, d.in_len, d.flags, d.cksum, d.out_cap, d.out_off) == \
                (off + h.in_off, h.in_len, h.flags, h.cksum, cap, slot_at), (i, k)
            slot_at += (cap + 255) & ~255
        at += info.nblocks
    return verdict


def test_index_kernels_equal_host_walk(batch, laid):
    data, spans, t = laid
    verdict = check_index(data, spans, t)
    assert set(verdict.values()) == {lz4ada.BATCH_OK}
    order = list(range(len(spans)))
    random.Random(3).shuffle(order)
    assert check_index(data, spans, t, order) == verdict


def test_index_kernels_on_golden_vectors():
    names = sorted(f for f in os.listdir(VECTORS) if f.endswith((".lz4", ".err")))
    files = []
    for name in names:
        with open(os.path.join(VECTORS, name), "rb") as fh:
            files.append(fh.read())
    data, spans = layout(files)
    verdict = check_index(data, spans, to_device(data))
    assert {lz4ada.BATCH_OK, lz4ada.BATCH_NOT_INDEXED} <= set(verdict.values())


# -------------------------------------------------------------- rejections

def linked_frame():
    blocks = [(c, r, False) for c, r in lz4ada.gen_linked_blocks(lz4ada.GEN_MIXED_NOD1, 77, 65536, 3)]
    return lz4frame.build_frame(blocks, 64 << 10, indep=False, content_cksum=True)[0]


def rejection(kind):
    """(frame bytes, bytes of it the job is given, expected reason)."""
    good, _ = three_blocks(block_cksum=True, content_cksum=True)
    assert lz4ada.frame_walk_host(good)[0] == lz4ada.BATCH_OK and len(lz4frame.header(64 << 10)) == 7
    if kind == "linked":
        return linked_frame(), None, lz4ada.BATCH_LINKED
    if kind == "bad_magic":
        return b"\x05" + good[1:], None, lz4ada.BATCH_NOT_INDEXED
    if kind == "header_checksum":
        return good[:6] + bytes([good[6] ^ 0x40]) + good[7:], None, lz4ada.BATCH_NOT_INDEXED
    if kind == "cut_inside_block":
        _, descs = lz4ada.frame_index(good)
        return good, descs[1].in_off + 100, lz4ada.BATCH_NOT_INDEXED
    if kind == "block_checksum":
        return bad_frame(kind), None, lz4ada.DEVFRAME_BLOCK
    if kind == "content_checksum":
        return bad_frame(kind), None, lz4ada.DEVFRAME_CHECKSUM
    assert kind == "content_size"
    return bad_frame("size_long"), None, lz4ada.DEVFRAME_SIZE


def check_rejected(t, data, job, given: bytes, reason):
    assert (job.status, job.reason, job.out_len, job.consumed) == (lz4ada.EXACT_PATH, reason, 0, 0)
    assert data[job.in_off:job.in_off + job.in_len] == given
    got = lz4ada.explain_frame(t, job)
    want = lz4ada.decode_frame_partial(given)
    assert got[:2] == want[:2]
    assert (type(got[2]), getattr(got[2], "message", None)) == (type(want[2]), getattr(want[2], "message", None))
    return want


@pytest.mark.parametrize("kind", ["linked", "bad_magic", "header_checksum", "cut_inside_block",
                                  "block_checksum", "content_checksum", "content_size"])
def test_one_bad_frame_does_not_cost_the_others(batch, kind):
    frame, cut, reason = rejection(kind)
    items = list(batch)
    items[BAD_AT] = (frame, b"", False)
    data, spans = layout([f for f, _, _ in items])
    if cut is not None:
        spans[BAD_AT] = (spans[BAD_AT][0], cut)  # the job's length, not the allocation
    t = to_device(data)
    out, jobs, _ = decode_guarded(t, spans)
    check_jobs(out, jobs, items, skip={BAD_AT})
    want = check_rejected(t, data, jobs[BAD_AT], frame[:cut], reason)
    if kind != "linked":  # a linked frame is good; this pass just does not take it
        assert want[2] is not None
    assert stats()["batched"] == NFRAMES - 1 and stats()["passes"] == 1


# ------------------------------------------------------------------ bounds

def test_output_below_the_bound(laid):
    _, spans, t = laid
    bound, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans)
    assert bound > 0
    buf = torch.full((bound + TAIL,), SENTINEL, dtype=torch.uint8, device=t.device)
    with pytest.raises(lz4ada.TooLittleMemory) as ei:
        lz4ada.decode_frames_device(t.data_ptr(), t.numel(), spans, buf.data_ptr(), bound - 1)
    torch.cuda.synchronize()
    assert ei.value.bound == bound and str(bound) in ei.value.message
    assert to_host(buf) == bytes([SENTINEL]) * (bound + TAIL)
    assert stats()["passes"] == 0


def test_misuse(laid):
    data, spans, t = laid
    buf = torch.empty(1 << 20, dtype=torch.uint8, device=t.device)
    overlapping = list(spans)
    overlapping[5] = (spans[5][0], spans[6][0] + 10 - spans[5][0])
    past = list(spans)
    past[-1] = (len(data) - 5, 10)
    for bad in (overlapping, past, [(-1, 8)] + spans[1:]):
        random.Random(1).shuffle(bad)
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.decode_frames_device(t.data_ptr(), t.numel(), bad, buf.data_ptr(), buf.numel())
        assert stats() == dict(batched=0, single=0, passes=0, gpu=0, host=0)
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.frames_device_bound(t.data_ptr(), t.numel(), bad)
    n, jobs = lz4ada.decode_frames_device(t.data_ptr(), t.numel(), [], 0, 0)
    assert n == 0 and stats()["passes"] == 0


# ------------------------------------------------------------------ budget

def test_budget_splits_the_pass(batch, laid, monkeypatch):
    data, spans, t = laid
    whole, jobs0, _ = decode_guarded(t, spans)
    budget = 1 << 20
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(budget))

    def slots(frame):
        info, descs = lz4ada.frame_index(frame)
        return sum((slot_cap(descs[k], info.block_max) + 255) & ~255 for k in range(info.nblocks))
    over = {i for i, (f, _, _) in enumerate(batch) if i != SKIP_AT and slots(f) > budget}
    assert MANY_AT in over and len(over) < NFRAMES // 2
    out, jobs, _ = decode_guarded(t, spans)
    check_jobs(out, jobs, batch, skip=over)
    for i in over:
        j = jobs[i]
        assert (j.status, j.reason, j.out_len, j.consumed) == \
            (lz4ada.EXACT_PATH, lz4ada.BATCH_OVER_BUDGET, 0, 0), i
    for i in set(range(NFRAMES)) - over:
        a, b = jobs0[i], jobs[i]
        assert out[b.out_off:b.out_off + b.out_len] == whole[a.out_off:a.out_off + a.out_len]
    s = stats()
    assert s["passes"] > 1 and s["batched"] == NFRAMES - len(over)


# ---------------------------------------------------------- large checksum

def test_host_hash_branch(batch, monkeypatch):
    monkeypatch.setenv("LZ4ADA_BATCH_HASH_MAX", "4096")
    bad = bad_frame("content_checksum")
    items = list(batch)
    data, spans = layout([f for f, _, _ in items])
    t = to_device(data)
    out, jobs, _ = decode_guarded(t, spans)
    check_jobs(out, jobs, items)
    s = stats()
    assert s["host"] == sum(1 for _, raw, ck in batch if ck and len(raw) > 4096) > 0
    assert s["gpu"] == sum(1 for _, raw, ck in batch if ck and len(raw) <= 4096) > 0
    assert s["batched"] == NFRAMES
    # a flipped content checksum on a host-hashed frame
    items[BAD_AT] = (bad, b"", True)
    data, spans = layout([f for f, _, _ in items])
    t = to_device(data)
    out, jobs, _ = decode_guarded(t, spans)
    check_jobs(out, jobs, items, skip={BAD_AT})
    want = check_rejected(t, data, jobs[BAD_AT], bad, lz4ada.DEVFRAME_CHECKSUM)
    assert isinstance(want[2], lz4ada.ChecksumError) and len(want[0]) > 4096
    assert stats()["host"] == s["host"] + 1
