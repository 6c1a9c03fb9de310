"""Dictionary decode in the many-frame device pass
(lz4ada_decode_frames_device_dict).  Kernel edges through the
product call -- dictionary lengths, alignments of d_dict, block sizes,
hand-built matches at the dictionary's edges -- then the structure of a pass
(the two gap rules, a mixed pass of 70 frames, exact sizes, split passes), the
verdicts, and the committed liblz4 fixtures.  Frames come from
lz4ada.gen_linked_blocks with the dictionary as history, so no liblz4 is
needed here; expected bytes are the generator's raw output and, as a
cross-check, lz4ada.decode_frame_dict_host."""
import ctypes
import json
import os
import struct

import pytest
import torch
import xxhash

import _lz4build
import lz4ada
import lz4frame
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

KiB = 1024
NOD1 = lz4ada.GEN_MIXED_NOD1
CANARY = 0xA5
LINKED_PATH = lz4ada.PATH_BATCH | lz4ada.PATH_LINKED
INDEP_PATH = lz4ada.PATH_BATCH | lz4ada.PATH_INDEPENDENT
DICT_DIR = os.path.join(GOLDEN, "lz4f_dict")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.delenv("LZ4ADA_BATCH_LINKED", raising=False)
    monkeypatch.delenv("LZ4ADA_BATCH_BYTES", raising=False)


def dict_bytes(n, seed=1):
    """Seeded text-like bytes (a period no match length shares)."""
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta", b"iota", b"kappa"]
    out, x = bytearray(), seed * 2654435761 & 0xffffffff
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7fffffff
        out += words[(x >> 16) % len(words)] + bytes([32 + (x >> 8) % 90])
    return bytes(out[:n])


def linked_frame(lens, d, seed, **kw):
    """A linked frame whose first block reads the dictionary and whose later
    blocks read the earlier ones -> (frame, plaintext)."""
    blocks = lz4ada.gen_linked_blocks(NOD1, seed, 0, 0, lens=list(lens), hist=d)
    return lz4frame.build_frame([(c, r, False) for c, r in blocks], 64 * KiB, indep=False, **kw)


def indep_frame(lens, d, seed, **kw):
    """An independent frame every block of which reads the dictionary."""
    blocks = [lz4ada.gen_linked_blocks(NOD1, seed + 17 * i, 0, 0, lens=[n], hist=d)[0] for i, n in enumerate(lens)]
    return lz4frame.build_frame([(c, r, False) for c, r in blocks], 64 * KiB, indep=True, **kw)


def hand_frame(seqs, final, d, **kw):
    """One hand-built block under the dictionary -> (frame, plaintext or None
    when a match reaches before the dictionary's first used byte)."""
    comp, _ = _lz4build.encode(seqs, final)
    hist = bytearray(d[-65536:])
    base, ok = len(hist), True
    for lits, off, ml in seqs:
        hist += lits
        if off > len(hist):
            ok = False
            break
        for _ in range(ml):
            hist.append(hist[-off])
    hist += final or b""
    plain = bytes(hist[base:]) if ok else b""
    frame, _ = lz4frame.build_frame([(comp, plain, False)], 64 * KiB, **kw)
    return frame, plain if ok else None


def to_device(data, at=0):
    """The bytes in device memory, `at` bytes into their allocation."""
    t = torch.empty(at + max(len(data), 1), dtype=torch.uint8, device="cuda")
    t[at:at + len(data)] = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8)[:len(data)]
    return t[at:at + len(data)]


def layout(frames):
    data, spans = b"", []
    for f in frames:
        spans.append((len(data), len(f)))
        data += f + b"\x00" * (-len(f) % 4 + 4)
    return data, spans


def run(frames, d, at=0, linked=True, exact=False, dict_id=None, out=None):
    data, spans = layout(frames)
    t, dt = to_device(data), (to_device(d, at) if d is not None else None)
    got, jobs = lz4ada.decode_frames_tensor(t, spans, out=out, linked=linked, exact=exact, dict=dt, dict_id=dict_id)
    return bytes(got.cpu().numpy().tobytes()), jobs


def check(frames, plains, d, **kw):
    """Every frame with a plaintext is delivered with exactly those bytes (and
    the host decoder agrees); one with None is EXACT_PATH / DEVFRAME_BLOCK."""
    out, jobs = run(frames, d, **kw)
    for i, (f, want) in enumerate(zip(frames, plains)):
        j = jobs[i]
        if want is None:
            assert (j.status, j.reason, j.out_len) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK, 0), i
            continue
        assert (j.status, j.reason) == (0, lz4ada.DEVFRAME_OK), (i, j.reason)
        assert out[j.out_off:j.out_off + j.out_len] == want, i
        assert j.consumed == len(f)
    return out, jobs


def host(frame, d):
    return lz4ada.decode_frame_dict_host(frame, d or b"")[0]


# ------------------------------------------------------------- kernel edges

BLOCK_SIZES = [1, 63, 64, 4096, 65535, 65536]


@pytest.mark.parametrize("dict_len", [1, 4, 15, 16, 17, 255, 256, 257, 65535, 65536, 65537, 100000])
def test_dictionary_lengths_block_sizes_and_alignment(dict_len):
    d = dict_bytes(dict_len, seed=dict_len)
    frames, plains = [], []
    for k, n in enumerate(BLOCK_SIZES):
        f, p = indep_frame([n], d, 100 + k, content_cksum=bool(k & 1), block_cksum=bool(k & 2))
        frames.append(f), plains.append(p)
    f, p = linked_frame([65536, 65536, 300], d, 7, content_cksum=True, with_content_size=True)
    frames.append(f), plains.append(p)
    for f, p in zip(frames, plains):
        assert host(f, d) == p
    for at in (0, 1, 3, 13):
        check(frames, plains, d, at=at)


def test_hand_built_edges():
    d = dict_bytes(300, seed=5)
    frames, plains = [], []
    f, p = hand_frame([(b"", 100, 40), (b"xy", 7, 9)], b"tail!", d, content_cksum=True)  # a match at position 0
    frames.append(f), plains.append(p)
    for off in range(1, 16):  # the period pattern crosses from the dictionary into the output
        f, p = hand_frame([(b"", off, off + 23)], b"12345", d, content_cksum=True)
        assert p[:off + 23] == (d[-off:] * 40)[:off + 23]
        frames.append(f), plains.append(p)
    f, p = hand_frame([(b"", 300, 4)], b"end..", d, content_cksum=True)  # exactly the first used byte
    assert p[:4] == d[:4]
    frames.append(f), plains.append(p)
    f, p = hand_frame([(b"", 301, 4)], b"end..", d)  # one byte further
    assert p is None
    frames.append(f), plains.append(p)
    f, p = hand_frame([(b"ab", 302, 5)], b"end..", d, content_cksum=True)  # the neighbour behind it
    frames.append(f), plains.append(p)
    for f, p in zip(frames, plains):
        if p is None:
            with pytest.raises(lz4ada.DataCorruption):
                host(f, d)
        else:
            assert host(f, d) == p
    check(frames, plains, d, at=3)


def test_reach_of_a_full_dictionary():
    """Offset 65,535 at position 0 reads the second of 65,536 used bytes."""
    d = dict_bytes(70000, seed=9)
    f, p = hand_frame([(b"", 65535, 8)], b"end..", d, content_cksum=True)
    assert p[:8] == d[-65535:][:8]
    check([f], [p], d, at=1)


# ------------------------------------------------------ structure of the pass

def test_independent_blocks_read_the_dictionary_not_block_1():
    d = dict_bytes(20000, seed=11)
    blocks = [lz4ada.gen_linked_blocks(NOD1, 21 + i, 0, 0, lens=[n], hist=d)[0]
              for i, n in enumerate([65536, 40000, 3000])]
    recs = [(c, r, False) for c, r in blocks]
    f, p = lz4frame.build_frame(recs, 64 * KiB, indep=True, content_cksum=True, block_cksum=True)
    assert host(f, d) == p
    # the same payloads behind a linked header decode to other bytes: blocks 2
    # and 3 do hold matches that start before their block
    as_linked, _ = lz4frame.build_frame(recs, 64 * KiB, indep=False, content_cksum=True)
    with pytest.raises(lz4ada.LZ4AdaError):
        host(as_linked, d)
    check([f], [p], d)
    assert lz4ada.last_path() == INDEP_PATH


def test_linked_frame_of_three_full_blocks():
    d = dict_bytes(65536, seed=13)
    f, p = linked_frame([65536, 65536, 65536], d, 31, content_cksum=True, with_content_size=True)
    assert host(f, d) == p
    check([f], [p], d)
    assert lz4ada.last_path() == LINKED_PATH


def skippable(payload):
    return struct.pack("<II", 0x184D2A53, len(payload)) + payload


def legacy(blocks):
    return struct.pack("<I", 0x184C2102) + b"".join(struct.pack("<I", len(c)) + c for c, _ in blocks)


@pytest.fixture(scope="module")
def mixed():
    """70 frames, seven kinds in turn -> (dictionary, frames, plaintexts, which hold no dictionary match)."""
    d = dict_bytes(30000, seed=17)
    frames, plains, plain_kind = [], [], []
    for i in range(70):
        kind = i % 7
        n = [200, 2048, 4096, 8000, 65536][i % 5]
        if kind == 0:
            f, p = indep_frame([n, 1000 + i], d, 1000 + i, content_cksum=bool(i & 1), block_cksum=bool(i & 2))
        elif kind == 1:
            f, p = linked_frame([65536, 65536, n], d, 2000 + i, content_cksum=True, with_content_size=bool(i & 2))
        elif kind == 2:
            f, p = skippable(bytes(i)), b""
        elif kind == 3:
            blocks = [lz4ada.gen_block(lz4ada.GEN_MIXED, 3000 + i + k, 300 + 10 * k) for k in range(2)]
            f, p = legacy(blocks), b"".join(r for _, r in blocks)
        elif kind == 4:
            f, p = lz4frame.build_frame([], 64 * KiB, content_cksum=True)
        elif kind == 5:
            raw = dict_bytes(n, seed=4000 + i)
            f, p = lz4frame.build_frame([(raw, raw, True)], 64 * KiB, block_cksum=True, content_cksum=True)
        else:
            c, r = lz4ada.gen_block(lz4ada.GEN_MIXED, 5000 + i, n)
            f, p = lz4frame.build_frame([(c, r, False)], 64 * KiB, content_cksum=True)
        frames.append(f), plains.append(p), plain_kind.append(kind >= 2)
    return d, tuple(frames), tuple(plains), tuple(plain_kind)


def check_mixed(mixed, out, jobs, n_out):
    d, frames, plains, _ = mixed
    end = 0
    for i, (f, want) in enumerate(zip(frames, plains)):
        j = jobs[i]
        assert (j.status, j.reason) == (0, lz4ada.DEVFRAME_OK), (i, j.reason)
        assert out[j.out_off:j.out_off + j.out_len] == want, i
        assert j.consumed == len(f) and j.out_off >= end
        end = j.out_off + j.out_len
    assert n_out == sum(len(p) for p in plains) == end


def test_mixed_pass(mixed):
    d, frames, plains, plain_kind = mixed
    for f, p, k in zip(frames, plains, plain_kind):
        if f[:4] == struct.pack("<I", 0x184D2204):
            assert host(f, d) == p
    data, spans = layout(frames)
    t, dt = to_device(data), to_device(d, 13)
    bound, bjobs = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, torch.cuda.current_stream().cuda_stream,
                                              True, lz4ada.DeviceDict(dt.data_ptr(), dt.numel(), 0, 0))
    assert all(j.status == 0 for j in bjobs[:len(frames)])
    buf = torch.full((bound + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    got, jobs = lz4ada.decode_frames_tensor(t, spans, out=buf[:bound], linked=True, dict=dt)
    n = got.numel()
    whole = bytes(buf.cpu().numpy().tobytes())
    check_mixed(mixed, whole, jobs, n)
    assert whole[n:] == bytes([CANARY]) * (len(whole) - n)  # untouched at and beyond *out_len
    s = lz4ada.last_batch_stats()
    assert (s.frames_batched, s.passes) == (70, 1)
    # the frames without a dictionary match: the bytes the _opt call gives
    got0, jobs0 = lz4ada.decode_frames_tensor(t, spans, linked=True)
    out0 = bytes(got0.cpu().numpy().tobytes())
    for i, plain in enumerate(plain_kind):
        if plain:
            assert (jobs0[i].status, jobs0[i].out_len) == (0, jobs[i].out_len)
            assert out0[jobs0[i].out_off:jobs0[i].out_off + jobs0[i].out_len] == plains[i]
        else:  # the contrast, before and after this feature: no dictionary, no decode
            assert (jobs0[i].status, jobs0[i].reason) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK), i


def test_mixed_pass_exact(mixed):
    d, frames, plains, _ = mixed
    data, spans = layout(frames)
    t, dt = to_device(data), to_device(d, 1)
    total = sum(len(p) for p in plains)
    sized, _ = lz4ada.frames_device_sizes(t.data_ptr(), t.numel(), spans, torch.cuda.current_stream().cuda_stream, True)
    assert sized == total
    buf = torch.full((total + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    got, jobs = lz4ada.decode_frames_tensor(t, spans, out=buf[:total], linked=True, exact=True, dict=dt)
    whole = bytes(buf.cpu().numpy().tobytes())
    check_mixed(mixed, whole, jobs, got.numel())
    assert whole[total:] == bytes([CANARY]) * 4096


def test_gaps_split_the_passes(mixed, monkeypatch):
    """A budget that holds every slot of the pass at once (laid out by the exact
    sizes) and, with a 64 KiB dictionary, less than half of slots plus gaps."""
    d, frames, plains, _ = mixed
    long_d = dict_bytes(65536 - len(d), seed=41) + d  # the same tail, a gap of 65,792 bytes
    total = sum(len(p) for p in plains)
    budget = total + 256 * 200  # every slot rounded up to 256; fewer than 200 blocks
    gapped = 10 * 2 + 10 + 10 + 10  # independent blocks, linked frames, stored-only and no-dictionary frames
    assert total + gapped * 65792 > 2 * budget
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(budget))
    data, spans = layout(frames)
    got, jobs = lz4ada.decode_frames_tensor(to_device(data), spans, linked=True, exact=True)
    assert lz4ada.last_batch_stats().passes == 1
    out, jobs = run(frames, long_d, at=3, exact=True)
    # (passes lay their bytes back to back, so the layout is one pass's)
    check_mixed(mixed, out, jobs, len(out))
    assert lz4ada.last_batch_stats().passes >= 3


# ------------------------------------------------------------------ verdicts

def test_wrong_dictionary_is_a_checksum_verdict():
    d = dict_bytes(5000, seed=23)
    with_ck, p1 = hand_frame([(b"", 50, 20)], b"tail.", d, content_cksum=True)
    without, p2 = hand_frame([(b"", 50, 20)], b"tail.", d)
    other, p3 = hand_frame([(b"", 500, 20)], b"tail.", d, content_cksum=True)  # reads elsewhere
    bad = bytearray(d)
    bad[-45] ^= 0x40
    out, jobs = run([with_ck, without, other], bytes(bad))
    assert (jobs[0].status, jobs[0].reason) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_CHECKSUM)
    assert jobs[1].status == 0 and out[jobs[1].out_off:jobs[1].out_off + jobs[1].out_len] != p2
    assert jobs[2].status == 0 and out[jobs[2].out_off:jobs[2].out_off + jobs[2].out_len] == p3
    with pytest.raises(lz4ada.ChecksumError):
        host(with_ck, bytes(bad))


def test_dictionary_id():
    d = dict_bytes(3000, seed=29)
    frames, plains = [], []
    for did in (None, 7, 8):
        blocks = lz4ada.gen_linked_blocks(NOD1, 300, 0, 0, lens=[2000], hist=d)
        f, p = lz4frame.build_frame([(c, r, False) for c, r in blocks], 64 * KiB, content_cksum=True,
                                    with_content_size=(did == 8), dict_id=did)
        frames.append(f), plains.append(p)
    frames.append(skippable(b"abc")), plains.append(b"")
    out, jobs = run(frames, d, dict_id=7)
    assert [(j.status, j.reason) for j in jobs[:4]] == [(0, 0), (0, 0), (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_DICT), (0, 0)]
    assert out[jobs[0].out_off:jobs[0].out_off + jobs[0].out_len] == plains[0]
    assert out[jobs[1].out_off:jobs[1].out_off + jobs[1].out_len] == plains[1]
    assert jobs[2].out_len == 0
    out, jobs = run(frames, d)  # no check asked for: every id is accepted
    assert [j.status for j in jobs[:4]] == [0, 0, 0, 0]
    data, spans = layout(frames)
    t, dt = to_device(data), to_device(d)
    stream = torch.cuda.current_stream().cuda_stream
    dd = lz4ada.DeviceDict(dt.data_ptr(), dt.numel(), 8, lz4ada.DICT_CHECK_ID)
    bound, jobs = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, stream, True, dd)
    assert [(j.status, j.reason) for j in jobs[:4]] == [(0, 0), (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_DICT), (0, 0), (0, 0)]
    bound0, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, stream, True)
    assert 0 < bound < bound0  # the rejected frame takes no room


def test_misuse_launches_nothing():
    d = dict_bytes(100)
    f, p = indep_frame([500], d, 3, content_cksum=True)
    data, spans = layout([f])
    t, dt = to_device(data), to_device(d)
    out = torch.full((70000,), CANARY, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for dd in (lz4ada.DeviceDict(dt.data_ptr(), -1, 0, 0), lz4ada.DeviceDict(None, 5, 0, 0),
               lz4ada.DeviceDict(dt.data_ptr(), dt.numel(), 0, 2)):
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.decode_frames_device(t.data_ptr(), t.numel(), spans, out.data_ptr(), out.numel(), stream, True,
                                        False, dd)
        assert lz4ada.last_batch_stats().passes == 0
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, stream, True, dd)
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy().tobytes()) == bytes([CANARY]) * 70000


def test_no_dictionary_is_the_opt_call(mixed):
    _, frames, plains, _ = mixed
    data, spans = layout(frames)
    t = to_device(data)

    def stats():
        s = lz4ada.last_batch_stats()
        return (s.frames_batched, s.frames_single, s.passes, s.gpu_hashed, s.host_hashed), lz4ada.last_path()

    got0, jobs0 = lz4ada.decode_frames_tensor(t, spans, linked=True)
    want = bytes(got0.cpu().numpy().tobytes()), [(j.out_off, j.out_len, j.consumed, j.status, j.reason) for j in jobs0[:70]], stats()
    stream = torch.cuda.current_stream().cuda_stream
    bound, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans, stream, True)
    dt = to_device(b"xyz")
    for dd in (None, lz4ada.DeviceDict(None, 0, 0, 0), lz4ada.DeviceDict(dt.data_ptr(), 0, 5, lz4ada.DICT_CHECK_ID)):
        out = torch.empty(bound, dtype=torch.uint8, device="cuda")
        jobs = lz4ada._device_jobs(spans)
        n = lz4ada._i64()
        st = lz4ada._lib.lz4ada_decode_frames_device_dict(t.data_ptr(), t.numel(), jobs, len(spans), lz4ada.FRAMES_LINKED,
                                                          None if dd is None else ctypes.byref(dd), out.data_ptr(),
                                                          out.numel(), ctypes.byref(n), stream)
        assert st == 0
        got = bytes(out[:n.value].cpu().numpy().tobytes()), [(j.out_off, j.out_len, j.consumed, j.status, j.reason) for j in jobs[:70]], stats()
        assert got == want


# ------------------------------------------------------------------ fixtures

def test_liblz4_fixtures():
    with open(os.path.join(DICT_DIR, "manifest.json")) as fh:
        m = json.load(fh)
    for name, info in m["dicts"].items():
        with open(os.path.join(DICT_DIR, info["file"]), "rb") as fh:
            d = fh.read()
        mine = [f for f in m["frames"] if f["dict"] == name]
        frames = []
        for f in mine:
            with open(os.path.join(DICT_DIR, f["file"]), "rb") as fh:
                frames.append(fh.read())
        out, jobs = run(frames, d, at=1)
        for f, j in zip(mine, jobs):
            assert (j.status, j.reason) == (0, lz4ada.DEVFRAME_OK), (f["file"], j.reason)
            assert j.out_len == f["size"] and j.consumed == f["frame_len"]
            assert xxhash.xxh32(out[j.out_off:j.out_off + j.out_len]).intdigest() == f["xxh32"], f["file"]
        # the contrast, before and after this feature: the call without a dictionary rejects them
        out0, jobs0 = run(frames, None)
        assert all((j.status, j.reason) == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK) for j in jobs0[:len(frames)])
