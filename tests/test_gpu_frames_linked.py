"""Linked frames in the many-frame passes (LZ4ADA_FRAMES_LINKED, DESIGN.md
§12).  The kernel alone (k_index + k_decode_idx_frames through
lz4ada_decode_idx_frames_debug): chains of every shape, one wave per frame,
70 frames in a launch, nothing written outside a frame's slots and statuses;
quirk D1 judged from the round state, on the committed fixtures.  Then the
host pass (decode_frames, decode_stream under LZ4ADA_BATCH_LINKED=1) and the
device pass (decode_frames_tensor) over independent and linked frames in turn,
with a D1 frame and a corrupt one among them.  Every byte is checked against
the oracle, frame by frame."""
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import _oracle as O
import lz4ada
import lz4frame
from conftest import GOLDEN
from test_gpu_frames_batch import make_frame

pytestmark = pytest.mark.gpu

KiB = 1024
NOD1 = lz4ada.GEN_MIXED_NOD1
CANARY = 0xA5
EDGE = 4096  # canary bytes before the first slot and behind the last
LINKED_PATH = lz4ada.PATH_BATCH | lz4ada.PATH_LINKED
INDEP_PATH = lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT
BIG_CAP = str(64 << 20)  # a cap every frame here is within: the tests do not hang on the tuned default


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


@pytest.fixture(autouse=True)
def cap_and_switch(monkeypatch):
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", BIG_CAP)
    monkeypatch.delenv("LZ4ADA_BATCH_LINKED", raising=False)


def fixture_bytes(name):
    with open(os.path.join(GOLDEN, "lz4f", name + ".lz4"), "rb") as fh:
        return fh.read()


def oracle(frame):
    """(status, bytes output before any exception, message) of the frame alone."""
    st, out, _, msg = O.decode_stream(frame, out_cap=8 << 20)
    return st, out, msg


def oracle_alone(frame):
    st, out, msg = oracle(frame)
    assert st == O.OK, msg
    return out


def linked_frame(lens, bmax=64 * KiB, seed=1, stored_at=(), block_cksum=False, content_cksum=True,
                 size=False):
    """A linked frame of blocks decoding to lens bytes whose matches reach into
    the earlier blocks (the blocks at stored_at are stored) -> (frame, plaintext)."""
    blocks = lz4ada.gen_linked_blocks(NOD1, seed, 0, 0, lens=list(lens))
    recs = [(r, r, True) if i in stored_at else (c, r, False) for i, (c, r) in enumerate(blocks)]
    return lz4frame.build_frame(recs, bmax, indep=False, block_cksum=block_cksum,
                                content_cksum=content_cksum, with_content_size=size)


# ------------------------------------------------------------ the kernel alone

def round256(v):
    return (v + 255) & ~255


def pass_layout(frames):
    """The frames back to back and their descriptors as a pass lays them out
    (in_off absolute, out_cap the slot capacity, out_off from EDGE on in steps
    of round256) -> (input bytes, BlockDesc array, first[], decoded length bound)."""
    data, descs, first, slot_at = b"", [], [0], EDGE
    for f in frames:
        info, ds = lz4ada.frame_index(f)
        for d in ds[:info.nblocks]:
            cap = d.in_len if d.flags & lz4ada.BLOCK_STORED else min(info.block_max, 255 * d.in_len + 64)
            descs.append(lz4ada.BlockDesc(len(data) + d.in_off, d.in_len, d.flags, slot_at, cap, d.cksum))
            slot_at += round256(cap)
        first.append(len(descs))
        data += f
    arr = (lz4ada.BlockDesc * max(len(descs), 1))(*descs)
    return data, arr, first, slot_at + EDGE


def run_kernel(frames, marks=None):
    """k_index + k_decode_idx_frames over the frames -> (statuses, slot buffer,
    descriptors, first[]).  The slots start as CANARY bytes and the statuses of
    unmarked frames as 0xEE bytes."""
    marks = [True] * len(frames) if marks is None else marks
    data, descs, first, out_len = pass_layout(frames)
    nb = first[-1]
    dev = torch.device("cuda:0")
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_desc = torch.frombuffer(bytearray(bytes(descs)[:max(nb, 1) * 32]), dtype=torch.uint8).to(dev)
    d_out = torch.full((out_len,), CANARY, dtype=torch.uint8, device=dev)
    st0 = bytearray(nb * 32)
    for i, m in enumerate(marks):
        if not m:
            st0[first[i] * 32:first[i + 1] * 32] = b"\xee" * (32 * (first[i + 1] - first[i]))
    d_st = torch.frombuffer(bytearray(st0) or bytearray(32), dtype=torch.uint8).to(dev)
    lz4ada.decode_idx_frames_debug(d_in.data_ptr(), len(data), d_desc.data_ptr(), nb, first, marks,
                                   d_out.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    st = (lz4ada.BlockStatus * max(nb, 1)).from_buffer_copy(d_st.cpu().numpy().tobytes())
    return st, d_out.cpu().numpy().tobytes(), descs, first


def check_slots(frames, marks, st, out, descs, first, want_codes=None):
    """Every DS_OK block of a marked frame holds the oracle's bytes of that
    block; nothing lies outside the slots' own bytes; an unmarked frame's
    statuses and slots are untouched.  want_codes: per frame, 0 / non-zero per block."""
    owned = np.zeros(len(out), dtype=bool)  # where a marked frame's slot lies
    for i, f in enumerate(frames):
        _, ref, _ = oracle(f)
        at = 0
        for b in range(first[i], first[i + 1]):
            d, s = descs[b], st[b]
            if not marks[i]:
                assert bytes(s) == b"\xee" * 32, (i, b)
                continue
            owned[d.out_off:d.out_off + d.out_cap] = True
            if want_codes is not None:
                assert (s.code != 0) == (want_codes[i][b - first[i]] != 0), (i, b, s.code)
            if s.code == 0:
                assert s.out_len <= d.out_cap
                assert out[d.out_off:d.out_off + s.out_len] == ref[at:at + s.out_len], (i, b)
                assert at + s.out_len <= len(ref), (i, b)
                at += s.out_len
            else:  # the chain ended: every later block of the frame is declined too
                assert all(st[r].code != 0 for r in range(b, first[i + 1])), (i, b)
                break
    outside = np.frombuffer(out, dtype=np.uint8)[~owned]
    assert len(outside) >= 2 * EDGE and (outside == CANARY).all()


ALONE = {
    "one_short_block": ([1234], {}),
    "two_blocks_last_1_byte": ([65536, 1], {}),
    "three_full_and_7000": ([65536] * 3 + [7000], {}),
    "stored_between_compressed": ([65536] * 3 + [500], dict(stored_at=(1,))),
    "blocks_256k": ([262144] * 3, dict(bmax=256 * KiB)),
}


@pytest.mark.parametrize("name", sorted(ALONE))
def test_kernel_chain(name):
    lens, kw = ALONE[name]
    frame, raw = linked_frame(lens, seed=11, **kw)
    assert oracle_alone(frame) == raw
    st, out, descs, first = run_kernel([frame])
    check_slots([frame], [True], st, out, descs, first, want_codes=[[0] * len(lens)])
    assert [s.out_len for s in st[:len(lens)]] == lens


def test_kernel_matches_reach_the_previous_block():
    """Not vacuous: decoded as independent blocks, the later blocks are declined."""
    frame, _ = linked_frame([65536] * 3 + [7000], seed=11)
    st, _, _, first = run_kernel([frame], [True])
    assert [s.code for s in st[:4]] == [0, 0, 0, 0]
    info, descs = lz4ada.frame_index(frame)
    dev = torch.device("cuda:0")
    d_in = torch.frombuffer(bytearray(frame), dtype=torch.uint8).to(dev)
    d_desc = torch.frombuffer(bytearray(bytes(descs)[:4 * 32]), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(4 * 65536, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(4 * 32, dtype=torch.uint8, device=dev)
    lz4ada.launch_decode_variant(d_in.data_ptr(), len(frame), d_desc.data_ptr(), 4, d_out.data_ptr(),
                                 d_st.data_ptr(), lz4ada.DECODE_IDX_ALONE)
    torch.cuda.synchronize()
    alone = (lz4ada.BlockStatus * 4).from_buffer_copy(d_st.cpu().numpy().tobytes())
    assert alone[0].code == 0 and all(alone[b].code != 0 for b in (1, 2, 3))


def test_kernel_short_middle_block():
    lens = [65536, 30000, 65536, 100]
    frame, raw = linked_frame(lens, seed=5)
    assert oracle_alone(frame) == raw
    st, out, descs, first = run_kernel([frame])
    assert [s.code for s in st[:4]] == [0, 0, lz4ada.DS_RETRY, lz4ada.DS_RETRY]
    check_slots([frame], [True], st, out, descs, first)


def test_kernel_reference_before_the_frame_start():
    """A first block whose match reads before the frame: declined, and not a
    byte outside the frame's own slots (canaries on both sides); the frames
    beside it decode."""
    bad = bytes([0x14]) + b"A" + struct.pack("<H", 5) + bytes([0x50]) + b"abcde"
    comp, raw = lz4ada.gen_block(NOD1, 7, 3000)
    broken, _ = lz4frame.build_frame([(bad, b"", False), (comp, raw, False)], 64 * KiB, indep=False)
    assert oracle(broken)[0] == O.DATA_CORRUPTION
    good, _ = linked_frame([65536, 700], seed=3)
    frames = [good, broken, good]
    st, out, descs, first = run_kernel(frames)
    assert st[first[1]].code != 0 and st[first[1] + 1].code != 0
    check_slots(frames, [True] * 3, st, out, descs, first, want_codes=[[0, 0], [1, 1], [0, 0]])


def test_kernel_leaves_an_unmarked_frame_alone():
    frames = [linked_frame([65536, 900], seed=s)[0] for s in (21, 22, 23)]
    marks = [True, False, True]
    st, out, descs, first = run_kernel(frames, marks)
    check_slots(frames, marks, st, out, descs, first, want_codes=[[0, 0]] * 3)


def test_kernel_70_frames_uneven_chains():
    """More frames than a wave has lanes, 1 to 5 blocks each."""
    rng = random.Random(70)
    frames, lens_of = [], []
    for i in range(70):
        n = 1 + i % 5
        lens = [65536] * (n - 1) + [rng.choice([1, 17, 4095, 30000, 65536])]
        frames.append(linked_frame(lens, seed=100 + 7 * i, block_cksum=bool(i & 1))[0])
        lens_of.append(lens)
    st, out, descs, first = run_kernel(frames)
    check_slots(frames, [True] * 70, st, out, descs, first, want_codes=[[0] * len(l) for l in lens_of])
    assert [st[b].out_len for b in range(first[-1])] == [n for l in lens_of for n in l]


# ---- quirk D1 from the round state (the fixtures' facts: tests/golden/make_lz4_fixtures.py)

@pytest.mark.parametrize("name,nblocks", [("linked64k", 17), ("linked256k", 7)])
def test_d1_rule_takes_frames_outside_the_round_state(name, nblocks):
    """linked256k holds two blocks with matches >= 65,529 back before the block
    start, yet the round state is never in [65536, 65542]: the rule is the
    state, not the flag alone."""
    frame = fixture_bytes(name)
    st, out, descs, first = run_kernel([frame])
    assert first == [0, nblocks]
    assert [s.code for s in st[:nblocks]] == [0] * nblocks
    check_slots([frame], [True], st, out, descs, first)
    if name == "linked256k":
        assert sum(1 for s in st[:nblocks] if s.aux & 1) == 2  # AUX_D1_RISK


@pytest.mark.parametrize("name", ["d1_cksum", "d1_l1_o65535", "d1_l3_o65533", "d1_l13_o65529", "d1_l20_o65535"])
def test_d1_rule_stops_a_flagged_block_in_the_round_state(name):
    frame = fixture_bytes(name)
    st, out, descs, first = run_kernel([frame])
    assert first == [0, 2]
    assert (st[0].code, st[0].out_len, st[1].code) == (0, 65536, lz4ada.DS_RETRY)
    check_slots([frame], [True], st, out, descs, first)


# ------------------------------------------------------------------ the passes

@pytest.fixture(scope="module")
def batch():
    """[(frame, oracle status, oracle bytes, oracle message, kind)]: 40 frames
    alternating independent and linked, then linked64k, linked256k, a D1
    frame and a linked frame with a corrupt block checksum.  kind: "indep",
    "linked" (a pass takes it), "d1", "corrupt".  Never modified."""
    out = []
    for i in range(40):
        if i % 2 == 0:
            f, _ = make_frame(2 * i + 1, [65536, 65536, 1000 + i])
            kind = "indep"
        else:
            f, _ = linked_frame([65536] * (1 + i % 4) + [1 + 777 * (i % 3)], seed=300 + i,
                                block_cksum=bool(i & 2), content_cksum=bool(i & 4), size=bool(i & 8))
            kind = "linked"
        out.append((f, kind))
    out += [(fixture_bytes("linked64k"), "linked"), (fixture_bytes("linked256k"), "linked"),
            (fixture_bytes("d1_l13_o65529"), "d1")]
    blocks = lz4ada.gen_linked_blocks(NOD1, 41, 0, 0, lens=[65536, 65536, 5000])
    recs = [lz4frame.block_record(c, block_cksum=True) for c, _ in blocks]
    r = bytearray(recs[1])
    r[100] ^= 1
    recs[1] = bytes(r)
    raw = b"".join(x for _, x in blocks)
    corrupt = lz4frame.header(64 * KiB, indep=False, block_cksum=True, content_cksum=True) + b"".join(recs) + \
        lz4frame.trailer(raw, content_cksum=True)
    out.append((corrupt, "corrupt"))
    res = []
    for f, kind in out:
        st, ref, msg = oracle(f)
        assert (st == O.OK) == (kind != "corrupt"), (kind, msg)
        res.append((f, st, ref, msg, kind))
    return tuple(res)


def stats():
    s = lz4ada.last_batch_stats()
    return dict(batched=s.frames_batched, single=s.frames_single, passes=s.passes)


def check_host(batch, out, jobs, linked, refused=()):
    """Every job's bytes, extent and path; refused: linked frames over the cap."""
    at = 0
    for i, (f, st, ref, msg, kind) in enumerate(batch):
        j = jobs[i]
        kind = "refused" if i in refused else kind
        assert j.out_off == at, i
        at += j.out_len
        assert out[j.out_off:j.out_off + j.out_len] == ref, (i, kind)  # a failed job: the bytes before the exception
        if kind == "corrupt":
            assert j.status != 0 and not j.path & lz4ada.PATH_BATCH
            exc = lz4ada._ERRORS[j.status](lz4ada._lib.lz4ada_frames_error(i).decode())
            assert str(exc) == O.exception_information(st, msg)
            continue
        assert (j.status, j.consumed) == (0, len(f)), (i, kind)
        if kind == "indep":
            # (without the flag an independent frame between two linked ones has no
            # neighbour to share a pass with, and goes the single way)
            assert j.path == INDEP_PATH if linked else j.path & lz4ada.PATH_INDEPENDENT, i
        elif kind == "linked" and linked:
            assert j.path == LINKED_PATH, i
        elif kind == "skip":  # consumed by the pass, no output
            assert j.path == lz4ada.PATH_BATCH, i
        else:  # the single way
            assert j.path and not j.path & lz4ada.PATH_BATCH, (i, kind)
    assert at == len(out)


def test_host_pass_with_the_flag(batch):
    frames = [b[0] for b in batch]
    good = sum(1 for b in batch if b[4] in ("indep", "linked"))
    out, jobs = lz4ada.decode_frames_jobs(frames, linked=True)
    check_host(batch, out, jobs, True)
    assert stats() == dict(batched=good, single=len(batch) - good, passes=1)
    assert lz4ada.last_path() & LINKED_PATH == LINKED_PATH
    res = lz4ada.decode_frames(frames, linked=True)
    for (data, consumed, exc), (f, st, ref, msg, kind) in zip(res, batch):
        assert data == ref
        assert (str(exc) == O.exception_information(st, msg)) if kind == "corrupt" else exc is None


def test_host_pass_without_the_flag(batch):
    frames = [b[0] for b in batch]
    out, jobs = lz4ada.decode_frames_jobs(frames)
    check_host(batch, out, jobs, False)
    assert stats()["batched"] == 0  # no two batchable frames are neighbours


def test_host_pass_environment_switch(batch, monkeypatch):
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED", "1")
    out, jobs = lz4ada.decode_frames_jobs([b[0] for b in batch])
    check_host(batch, out, jobs, True)


def test_host_pass_cap_below_a_frame(batch, monkeypatch):
    """linked64k's slots are 17 x 64 KiB: one byte less and the frame is refused
    with BATCH_LINKED, and still decodes right, on its own (as linked256k does,
    whose slots are 7 x 256 KiB); the smaller linked frames still share the pass."""
    at = [i for i, b in enumerate(batch) if b[0] == fixture_bytes("linked64k")][0]
    big = [i for i, b in enumerate(batch) if b[0] == fixture_bytes("linked256k")][0]
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(17 * 65536 - 1))
    assert lz4ada.stream_index(batch[at][0], linked=True)[0].batchable == lz4ada.BATCH_LINKED
    out, jobs = lz4ada.decode_frames_jobs([b[0] for b in batch], linked=True)
    check_host(batch, out, jobs, True, refused=(at, big))
    assert not jobs[at].path & lz4ada.PATH_BATCH
    assert stats()["batched"] == sum(1 for b in batch if b[4] in ("indep", "linked")) - 2
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", str(17 * 65536))
    assert lz4ada.stream_index(batch[at][0], linked=True)[0].batchable == lz4ada.BATCH_OK


CHILD = r"""
import sys
sys.path[:0] = sys.argv[3:]
import lz4ada
with open(sys.argv[1], "rb") as fh:
    data = fh.read()
out = lz4ada.decode_stream(data)
s = lz4ada.last_batch_stats()
with open(sys.argv[2], "wb") as fh:
    fh.write(out)
print(s.frames_batched, s.frames_single, s.passes, lz4ada.last_path())
"""


def test_stream_under_the_environment_switch(batch, tmp_path):
    """decode_stream in a fresh process with LZ4ADA_BATCH_LINKED=1: the frames
    that decode, concatenated; bytes as the oracle gives them frame by frame."""
    items = [b for b in batch if b[4] != "corrupt"]
    src, dst = tmp_path / "stream.lz4", tmp_path / "stream.out"
    src.write_bytes(b"".join(b[0] for b in items))
    env = dict(os.environ, LZ4ADA_BATCH_LINKED="1", LZ4ADA_BATCH_LINKED_MAX=BIG_CAP)
    paths = [os.path.dirname(lz4ada.__file__)]
    r = subprocess.run([sys.executable, "-c", CHILD, str(src), str(dst)] + paths, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert dst.read_bytes() == b"".join(b[2] for b in items)
    batched, single, passes, path = map(int, r.stdout.split())
    good = sum(1 for b in items if b[4] in ("indep", "linked"))
    assert (batched, single, passes) == (good, len(items) - good, 1)
    assert path & LINKED_PATH == LINKED_PATH


def layout(frames):
    rng = random.Random(78)
    parts, spans, at = [], [], 0
    for i, f in enumerate(frames):
        gap = bytes(rng.randrange(1, 256) for _ in range((i * 3 + 1) % 4))
        parts += [gap, f]
        spans.append((at + len(gap), len(f)))
        at += len(gap) + len(f)
    return b"".join(parts), spans


def to_host(t):
    return t.cpu().numpy().tobytes()


def decode_device(batch, linked):
    data, spans = layout([b[0] for b in batch])
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    bound, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, stream, linked=linked)
    buf = torch.full((bound + EDGE,), CANARY, dtype=torch.uint8, device=t.device)
    out, jobs = lz4ada.decode_frames_tensor(t, spans, out=buf[:bound], linked=linked)
    torch.cuda.current_stream().synchronize()
    whole = to_host(buf)
    assert out.numel() <= bound  # the bound suffices
    assert whole[out.numel():] == bytes([CANARY]) * (bound + EDGE - out.numel())  # at and beyond *out_len
    assert to_host(t) == data
    return whole[:out.numel()], jobs, data


def test_device_pass_with_the_flag(batch):
    out, jobs, data = decode_device(batch, True)
    assert lz4ada.last_path() == lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT | lz4ada.PATH_LINKED
    good = sum(1 for b in batch if b[4] in ("indep", "linked"))
    s = lz4ada.last_batch_stats()
    assert (s.frames_batched, s.passes) == (good, 1)
    end = 0
    for i, (f, st, ref, msg, kind) in enumerate(batch):
        j = jobs[i]
        if kind in ("indep", "linked"):
            assert (j.status, j.reason, j.consumed, j.out_len) == (0, 0, len(f), len(ref)), (i, kind)
            assert j.out_off >= end, i
            end = j.out_off + j.out_len
            assert out[j.out_off:end] == ref, (i, kind)
        else:
            assert (j.status, j.reason, j.out_len, j.consumed) == \
                (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK, 0, 0), (i, kind)
            got, _, exc = lz4ada.explain_frame(data, j)
            assert got == ref
            assert (str(exc) == O.exception_information(st, msg)) if st != O.OK else exc is None


def test_device_pass_without_the_flag(batch):
    out, jobs, _ = decode_device(batch, False)
    for i, (f, st, ref, msg, kind) in enumerate(batch):
        j = jobs[i]
        if kind == "indep":
            assert (j.status, j.reason) == (0, 0) and out[j.out_off:j.out_off + j.out_len] == ref, i
        else:
            assert (j.status, j.reason) == (lz4ada.EXACT_PATH, lz4ada.BATCH_LINKED), (i, kind)
    assert lz4ada.last_path() == INDEP_PATH


# ------------------------------------------- frames without blocks at the seams

def seam_frames():
    """[(frame, kind)] where the runs of a pass are cut with frames without
    blocks on both sides of every cut: kind "indep", "linked", "skip" or "bad"
    (a bad magic, which only the device engine is given: it rides along).
    Blocks of 300 to 5,000 bytes, but the first of the linked frame of two: the
    wave ends a chain after a block short of the block size
    (test_kernel_short_middle_block), so that one is full."""
    def skip(n):
        return struct.pack("<II", 0x184D2A53, n) + bytes(range(n))
    empty_linked = lz4frame.build_frame([], 64 * KiB, indep=False, content_cksum=True)[0]
    one_block = make_frame(3, [2000])[0]
    return [(make_frame(2, [])[0], "indep"),          # empty, with a content checksum
            (linked_frame([65536, 700], seed=61)[0], "linked"),
            (skip(33), "skip"),
            (linked_frame([1200], seed=62, block_cksum=True)[0], "linked"),
            (make_frame(0, [])[0], "indep"),          # empty
            (make_frame(7, [5000, 300])[0], "indep"),
            (empty_linked, "linked"),
            (one_block, "indep"),
            (b"\x05" + one_block[1:], "bad"),
            (linked_frame([4000], seed=63, size=True)[0], "linked"),
            (skip(5), "skip")]


@pytest.fixture(scope="module")
def seams():
    """seam_frames() with the oracle's (status, bytes, message), as `batch`."""
    res = []
    for f, kind in seam_frames():
        st, ref, msg = oracle(f)
        assert (st == O.OK) == (kind != "bad"), (kind, msg)
        res.append((f, st, ref, msg, kind))
    return tuple(res)


def test_runs_cut_beside_frames_without_blocks(seams):
    host = [b for b in seams if b[4] != "bad"]
    out, jobs = lz4ada.decode_frames_jobs([b[0] for b in host], linked=True)
    check_host(host, out, jobs, True)
    assert stats() == dict(batched=len(host), single=0, passes=1)

    out, jobs, data = decode_device(seams, True)
    assert lz4ada.last_path() == lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT | lz4ada.PATH_LINKED
    s = lz4ada.last_batch_stats()
    assert (s.frames_batched, s.passes) == (len(host), 1)
    end = 0
    for i, (f, st, ref, msg, kind) in enumerate(seams):
        j = jobs[i]
        if kind != "bad":
            assert (j.status, j.reason, j.consumed, j.out_len) == (0, 0, len(f), len(ref)), (i, kind)
            assert j.out_off >= end, i
            end = j.out_off + j.out_len
            assert out[j.out_off:end] == ref, (i, kind)
        else:
            assert (j.status, j.reason, j.out_len, j.consumed) == \
                (lz4ada.EXACT_PATH, lz4ada.BATCH_NOT_INDEXED, 0, 0), (i, kind)
            got, _, exc = lz4ada.explain_frame(data, j)
            assert got == ref and str(exc) == O.exception_information(st, msg)
