"""A compress call that writes the seek index of its own frames
(lz4ada_compress_frames_device_indexed).  Two yardsticks: the
existing compress calls for the frames, byte for byte, and
lz4ada_seek_index_build* over those frames for the index -- what it reports,
what it keeps (block starts, device bytes, the selection of a set of ranges, the
checkpoint store) and what ranges through it deliver, status by status and byte
for byte.  Then what the writer's index does that the build does not: a linked
frame past lz4ada_batch_linked_max(), and records whose linked frames carry
offsets of exactly 65,535 across a block boundary."""
import ctypes

import pytest
import torch

import lz4ada
from _compress_cases import KiB, noise, pseudo_text, record
from _compress_dict_cases import dict_frame_blocks, text_dict
from _compress_linked_cases import B, LENGTHS, crafted, mixed_jobs, parse_block_linked, rows_record

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4 * KiB
ALL = dict(block_checksum=True, content_checksum=True, content_size=True)
MIXED = mixed_jobs()


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not lz4ada.device_available():
        pytest.fail("MI355X not usable: " + lz4ada._thread_error())


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for name in ("LZ4ADA_BATCH_BYTES", "LZ4ADA_BATCH_HASH_MAX", "LZ4ADA_BATCH_LINKED_MAX", "LZ4ADA_BATCH_LINKED"):
        monkeypatch.delenv(name, raising=False)


def to_device(data, at=0):
    """The bytes in device memory, `at` bytes into their allocation."""
    t = torch.empty(at + max(len(data), 1), dtype=torch.uint8, device="cuda")
    t[at:at + len(data)] = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8)[:len(data)]
    return t[at:at + len(data)]


def to_host(t):
    return t.cpu().numpy().tobytes()


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def mixed_on_device():
    return to_device(MIXED[0])


def compress(t, spans, dd=None, dict_id=None, linked=False, index=False, checkpoint_bytes=0, **kw):
    """One call into a canary-filled buffer of bound + GUARD bytes -> (the
    buffer, bytes written, jobs[, the index])."""
    bound = lz4ada.compress_frames_bound([n for _, n in spans], dict=dd, dict_id=dict_id, **kw)
    out = torch.full((bound + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    got = lz4ada.compress_frames_device(t.data_ptr() if t.numel() else None, t.numel(), spans, out.data_ptr(), bound,
                                        stream(), dict=dd, dict_id=dict_id, linked=linked, index=index,
                                        checkpoint_bytes=checkpoint_bytes, **kw)
    return (out,) + tuple(got)


def job_tuple(j):
    return (j.in_off, j.in_len, j.out_off, j.out_len, j.status, j.stored_blocks)


def laid_out(recs):
    data, spans = b"", []
    for i, p in enumerate(recs):
        data += b"\x55" * (1 + i % 3)
        spans.append((len(data), len(p)))
        data += p
    return data, spans


def block_ranges(j, p, blen=B):
    """The straddling ranges of test_round_trip_through_a_linked_seek_index, the
    whole frame, and the first and last byte of every block."""
    r = [(j, blen - 5, 10), (j, blen - 1, 2), (j, 0, len(p)), (j, blen + 1, len(p) - blen - 1), (j, len(p) - 3, 100)]
    if len(p) > 2 * blen:
        r += [(j, blen - 100, blen + 200), (j, 2 * blen - 1, 1), (j, 2 * blen, 1)]
    for b in range(-(-len(p) // blen)):
        r += [(j, b * blen, 1), (j, min(len(p), (b + 1) * blen) - 1, 1)]
    return r


def build(out, n, jobs, count, linked=False, checkpoint_bytes=0, dt=None):
    where = [(jobs[i].out_off, jobs[i].out_len) for i in range(count)]
    return lz4ada.SeekIndex.build(out.data_ptr(), n, where, stream(), linked=linked, checkpoint_bytes=checkpoint_bytes,
                                  dict=dt.data_ptr() if dt is not None else None,
                                  dict_len=dt.numel() if dt is not None else 0)


def frame_report(idx):
    return [(j.in_off, j.in_len, j.out_off, j.out_len, j.consumed, j.status, j.reason)
            for j in (idx.jobs[i] for i in range(idx.njobs))]


def deliver(idx, frames, ranges):
    got, arr = lz4ada.decode_ranges_tensor(idx, frames, ranges)
    got = to_host(got)
    return [(arr[k].status, arr[k].reason, arr[k].out_off, arr[k].out_len,
             got[arr[k].out_off:arr[k].out_off + arr[k].out_len]) for k in range(len(ranges))]


def same_index(ix, built, frames, ranges, store=True):
    """Everything two indexes over the same frames can be asked."""
    assert frame_report(ix) == frame_report(built)
    assert lz4ada.seek_index_debug(ix) == lz4ada.seek_index_debug(built)
    assert ix.device_bytes == built.device_bytes
    assert lz4ada.ranges_select_debug(ix, ranges) == lz4ada.ranges_select_debug(built, ranges)
    if store:
        assert lz4ada.seek_index_store_debug(ix) == lz4ada.seek_index_store_debug(built)
    a, b = deliver(ix, frames, ranges), deliver(built, frames, ranges)
    for k in range(len(ranges)):
        assert a[k] == b[k], (k, ranges[k], a[k][:4], b[k][:4])
    return a


def check_delivered(res, ranges, recs):
    for k, (j, off, n) in enumerate(ranges):
        want = recs[j][off:off + n]
        assert res[k][0] == 0 and res[k][3] == len(want) and res[k][4] == want, (k, ranges[k], res[k][:4])


# ------------------------------------------------------------------- the frames

@pytest.mark.parametrize("shape", ["plain", "dict3", "dict1024", "dict65536", "linked", "linked_dict65536"])
def test_frames_equal_the_existing_calls(shape, mixed_on_device):
    """d_out, *out_len and jobs[] of the matching existing call, with no flag
    and under all three checksums; the guard region stays canary."""
    data, spans, plains = MIXED
    linked = shape.startswith("linked")
    dl = int(shape.split("dict")[1]) if "dict" in shape else None
    dt = to_device(text_dict(dl), dl % 3) if dl else None
    dd = (dt.data_ptr(), dl) if dl else None
    for kw in (dict(), ALL):
        want, wn, wjobs = compress(mixed_on_device, spans, dd, dict_id=5 if dl == 1024 else None, linked=linked, **kw)
        out, n, jobs, idx = compress(mixed_on_device, spans, dd, dict_id=5 if dl == 1024 else None, linked=linked,
                                     index=True, **kw)
        with idx:
            assert n == wn and [job_tuple(jobs[i]) for i in range(len(spans))] == \
                [job_tuple(wjobs[i]) for i in range(len(spans))]
            assert to_host(out) == to_host(want), "the indexed call's bytes differ, or the guard region was written"
            assert idx.in_len == n and idx.njobs == len(spans)
            rep = frame_report(idx)
            for i, p in enumerate(plains):
                assert rep[i] == (jobs[i].out_off, jobs[i].out_len, 0, len(p), 0, 0, 0), i


# ------------------------------------------------------ the index is the build's

def index_records():
    return [pseudo_text(n, n + 3) for n in (2 * B + 1, B + 1024, 4 * B + 777, 3 * B)] + \
        [rows_record(), b"", record(1), record(13)]


@pytest.mark.parametrize("every", [65536, 131072])
@pytest.mark.parametrize("shape", ["plain", "dict", "linked", "linked_dict"])
def test_index_equals_the_builds(shape, every):
    recs = index_records()
    data, spans = laid_out(recs)
    linked = shape.startswith("linked")
    dt = to_device(text_dict(65536), 1) if "dict" in shape else None
    dd = (dt.data_ptr(), dt.numel()) if dt is not None else None
    ranges = [r for j, p in enumerate(recs) for r in block_ranges(j, p) if r[1] >= 0 and r[2] >= 0]
    out, n, jobs, ix = compress(to_device(data), spans, dd, linked=linked, index=True, checkpoint_bytes=every,
                                block_checksum=True)
    frames = out[:n]
    with ix, build(out, n, jobs, len(spans), linked, every, dt) as built:
        assert all(built.jobs[j].status == 0 and built.jobs[j].out_len == len(p) for j, p in enumerate(recs)), \
            "the build must accept every frame of this comparison"
        res = same_index(ix, built, frames, ranges)
        check_delivered(res, ranges, recs)


def test_checkpoints_are_the_records_bytes():
    recs = index_records()
    data, spans = laid_out(recs)
    for every, K in ((65536, 1), (131072, 2), (0, 16)):
        out, n, jobs, ix = compress(to_device(data), spans, linked=True, index=True, checkpoint_bytes=every)
        with ix:
            store = lz4ada.seek_index_store_debug(ix)
            want = b""
            for p in recs:
                nb = -(-len(p) // B)
                for b in range(K, nb, K):
                    want += p[b * B - 65536:b * B]
            assert len(store) == len(want) and store == want
            assert bool(want) == (K < 16)  # (the default: a checkpoint per MiB, none in frames this short)


def test_past_the_linked_limit(monkeypatch):
    """The build puts one wave on a whole linked frame and refuses one over
    lz4ada_batch_linked_max(); the writer's index takes it."""
    rec = pseudo_text(4 * B + 777, 9)
    ranges = block_ranges(0, rec)
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", "131072")
    out, n, jobs, ix = compress(to_device(rec), [(0, len(rec))], linked=True, index=True, checkpoint_bytes=65536,
                                block_checksum=True)
    with ix, build(out, n, jobs, 1, True, 65536) as built:
        assert (built.jobs[0].status, built.jobs[0].reason) == (lz4ada.EXACT_PATH, lz4ada.BATCH_LINKED)
        assert frame_report(ix)[0] == (0, n, 0, len(rec), 0, 0, 0)
        check_delivered(deliver(ix, out[:n], ranges), ranges, [rec])


def d1_blocks(plain, frame):
    """The blocks after the first that hold a match reaching 65,529 or more
    back, before the block (quirk D1's shape)."""
    risky = set()
    for i, (stored, payload, _) in enumerate(dict_frame_blocks(frame)[4]):
        at = 0
        for lit, off, ml in ([] if stored or i == 0 else parse_block_linked(payload, plain, i, B)):
            at += lit
            if off >= 65529 and off > at:
                risky.add(i)
            at += ml
    return risky


def test_crafted_records():
    """Linked frames with offsets of exactly 65,535 across the boundary: a range
    delivers the record's bytes, or fails as a dictionary index's would -- and
    only where its chain holds such an offset."""
    recs = [rec for _, rec, _ in crafted()] + [pseudo_text(2 * B + 1, 4)]
    data, spans = laid_out(recs)
    ranges = [r for j, p in enumerate(recs) for r in block_ranges(j, p) if r[1] >= 0 and r[2] >= 0]
    out, n, jobs, ix = compress(to_device(data), spans, linked=True, index=True, checkpoint_bytes=65536)
    raw = to_host(out[:n])
    risky = [d1_blocks(p, raw[jobs[j].out_off:jobs[j].out_off + jobs[j].out_len]) for j, p in enumerate(recs)]
    assert any(risky) and not risky[-1]
    with ix:
        res = deliver(ix, out[:n], ranges)
    failed = 0
    for k, (j, off, m) in enumerate(ranges):
        want = recs[j][off:off + m]
        if res[k][0] == 0:
            assert res[k][3] == len(want) and res[k][4] == want, (k, ranges[k])
            continue
        failed += 1
        assert res[k][:2] == (lz4ada.EXACT_PATH, lz4ada.DEVFRAME_BLOCK) and res[k][3] == 0, (k, res[k][:4])
        touched = set(range(off // B, (min(off + m, len(recs[j])) - 1) // B + 1))  # K = 1: the chain is these
        assert touched & risky[j], (k, ranges[k], "a range failed whose chain holds no such offset")
    print(f"crafted records: {failed} of {len(ranges)} ranges failed")


# ------------------------------------------------------------------- dictionary

def test_the_index_keeps_its_own_dictionary():
    recs = index_records()[:3] + [record(13)]
    data, spans = laid_out(recs)
    ranges = [r for j, p in enumerate(recs) for r in block_ranges(j, p) if r[1] >= 0 and r[2] >= 0]
    for linked in (False, True):
        dt = to_device(text_dict(100000), 2)
        out, n, jobs, ix = compress(to_device(data), spans, (dt.data_ptr(), dt.numel()), dict_id=3, linked=linked,
                                    index=True, checkpoint_bytes=65536)
        dt.fill_(0x33)
        del dt
        torch.cuda.synchronize()
        with ix:
            check_delivered(deliver(ix, out[:n], ranges), ranges, recs)


def test_an_empty_dictionary_is_no_dictionary():
    recs = index_records()
    data, spans = laid_out(recs)
    t = to_device(data)
    ranges = [r for j, p in enumerate(recs) for r in block_ranges(j, p) if r[1] >= 0 and r[2] >= 0]
    for linked in (False, True):
        out, n, jobs, ix = compress(t, spans, linked=linked, index=True, checkpoint_bytes=65536)
        out0, n0, jobs0, ix0 = compress(t, spans, (None, 0), linked=linked, index=True, checkpoint_bytes=65536)
        with ix, ix0:
            assert to_host(out0) == to_host(out) and n0 == n
            same_index(ix0, ix, out[:n], ranges)


# ------------------------------------------------------------------ passes cut

def test_split_passes(monkeypatch, mixed_on_device):
    """LZ4ADA_BATCH_BYTES as tests/test_gpu_compress_linked.py sets it: the
    index of the cut call is the uncut call's."""
    data, spans, plains = MIXED
    dt = to_device(text_dict(65536))
    dd = (dt.data_ptr(), dt.numel())
    few = [s for s in spans if s[1] in LENGTHS or s[1] < 100]
    ranges = [(j, max(0, n - 70000), 70000) for j, (_, n) in enumerate(spans)]
    few_ranges = [r for j, (o, n) in enumerate(few) for r in block_ranges(j, data[o:o + n]) if r[1] >= 0 and r[2] >= 0]
    want = compress(mixed_on_device, spans, dd, dict_id=5, linked=True, index=True, checkpoint_bytes=65536, **ALL)
    want_few = compress(mixed_on_device, few, linked=True, index=True, checkpoint_bytes=65536)
    budget = 200 * KiB
    assert sum(-(-len(p) // 256) * 256 for p in plains) > 3 * budget
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", str(budget))
    got = compress(mixed_on_device, spans, dd, dict_id=5, linked=True, index=True, checkpoint_bytes=65536, **ALL)
    monkeypatch.setenv("LZ4ADA_BATCH_BYTES", "1")  # one record per pass
    got_few = compress(mixed_on_device, few, linked=True, index=True, checkpoint_bytes=65536)
    monkeypatch.delenv("LZ4ADA_BATCH_BYTES")
    for (out, n, jobs, ix), (wout, wn, wjobs, wix), rg in ((got, want, ranges), (got_few, want_few, few_ranges)):
        with ix, wix:
            assert to_host(out) == to_host(wout) and n == wn
            same_index(ix, wix, out[:n], rg)


def test_larger_blocks():
    """Blocks of 256 KiB: a record of 300,000 bytes, two of one block, an empty one."""
    plain = record(300000)
    data = b"\x00" * 5 + plain
    spans = [(5, 300000), (5, 4 * B), (7, 1000), (9, 0)]
    recs = [data[o:o + n] for o, n in spans]
    ranges = [r for j, p in enumerate(recs) for r in block_ranges(j, p, 4 * B) if r[1] >= 0 and r[2] >= 0]
    t = to_device(data)
    for linked in (False, True):
        out, n, jobs, ix = compress(t, spans, linked=linked, index=True, checkpoint_bytes=65536, block=256 * KiB, **ALL)
        with ix, build(out, n, jobs, len(spans), linked, 65536) as built:
            assert all(built.jobs[j].status == 0 for j in range(len(spans)))
            check_delivered(same_index(ix, built, out[:n], ranges), ranges, recs)
            assert len(lz4ada.seek_index_store_debug(ix)) == (65536 if linked else 0)


def test_a_frame_the_lone_block_rule_takes():
    """1 MiB blocks: noise is stored, and a frame of at most 24 blocks with a
    payload of 512 KiB or more belongs to the lone-block path
    (LZ4ADA_BATCH_BIG_BLOCK), here as at the build's index stage.  Its blocks
    and checkpoints leave the index, which then is the build's, bytes and all."""
    MiB = 1 << 20
    recs = [pseudo_text(70000, 1), noise(2 * MiB + 1000, 5), pseudo_text(MiB + 70000, 2), noise(MiB, 6), record(13)]
    data, spans = laid_out(recs)
    ranges = [r for j, p in enumerate(recs) for r in block_ranges(j, p, MiB) if r[1] >= 0 and r[2] >= 0]
    t = to_device(data)
    for linked in (False, True):
        out, n, jobs, ix = compress(t, spans, linked=linked, index=True, checkpoint_bytes=65536, block=MiB,
                                    block_checksum=True)
        with ix, build(out, n, jobs, len(spans), linked, 65536) as built:
            rep = frame_report(ix)
            assert [(r[5], r[6], r[3]) for r in rep] == [
                (0, 0, 70000), (lz4ada.EXACT_PATH, lz4ada.BATCH_BIG_BLOCK, 0), (0, 0, MiB + 70000),
                (lz4ada.EXACT_PATH, lz4ada.BATCH_BIG_BLOCK, 0), (0, 0, 13)]
            res = same_index(ix, built, out[:n], ranges)
            assert len(lz4ada.seek_index_store_debug(ix)) == (65536 if linked else 0)  # the text record's one
            taken = [k for k, r in enumerate(ranges) if r[0] in (0, 2, 4)]
            check_delivered([res[k] for k in taken], [ranges[k] for k in taken], recs)
            assert all(res[k][:2] == (lz4ada.EXACT_PATH, lz4ada.BATCH_BIG_BLOCK) for k in range(len(ranges))
                       if k not in taken)


# ----------------------------------------------------------- misuse and memory

def raw_call(t, n, jobs, out, cap, xopt, want_idx=True, njobs=1):
    ptr, got = ctypes.c_void_p(), ctypes.c_int64(-1)
    opt = lz4ada.CompressOptions(4, 0)
    st = lz4ada._lib.lz4ada_compress_frames_device_indexed(
        t.data_ptr(), n, jobs, njobs, ctypes.byref(opt), None, ctypes.byref(xopt) if xopt is not None else None,
        out.data_ptr(), cap, ctypes.byref(got), None, ctypes.byref(ptr) if want_idx else None, stream())
    return st, ptr.value, got.value


def test_misuse_and_memory():
    data = record(300)
    t = to_device(data)
    out = torch.full((1000 + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    jobs = lz4ada._compress_jobs([(0, 300)])
    bound = lz4ada.compress_frames_bound([300])
    for xopt in (lz4ada.CompressIndexOptions(0, 1, 0), lz4ada.CompressIndexOptions(2, 0, 0),
                 lz4ada.CompressIndexOptions(0x80000001, 0, 0), lz4ada.CompressIndexOptions(1, 0, -1)):
        assert raw_call(t, 300, jobs, out, 1000, xopt)[:2] == (6, None)  # LZ4ADA_ASSERTION_ERROR
    assert raw_call(t, 300, jobs, out, 1000, None, want_idx=False)[0] == 6
    st, ptr, got = raw_call(t, 300, jobs, out, bound - 1, None)
    assert (st, ptr, got) == (5, None, bound) and jobs[0].status == 5  # LZ4ADA_TOO_LITTLE_MEMORY
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "d_out was touched"
    st, ptr, got = raw_call(t, 300, jobs, out, bound, None)  # xopt NULL: {0, 0, 0}
    assert st == 0 and ptr and got == jobs[0].out_len
    assert to_host(out[:got]) == lz4ada.compress_frame_host(data) and bool((out[got:] == CANARY).all())
    lz4ada._lib.lz4ada_seek_index_free(ptr)
    st, ptr, got = raw_call(t, 300, jobs, out, 0, lz4ada.CompressIndexOptions(1, 0, 0), njobs=0)
    assert (st, got) == (0, 0) and ptr, "no job: an empty index"
    assert lz4ada._lib.lz4ada_seek_index_bytes(ptr) == 0
    lz4ada._lib.lz4ada_seek_index_free(ptr)


def test_ranges_on_a_moved_copy():
    recs = index_records()[:3]
    data, spans = laid_out(recs)
    ranges = [r for j, p in enumerate(recs) for r in block_ranges(j, p) if r[1] >= 0 and r[2] >= 0]
    frames, where, ix = lz4ada.compress_frames_tensor(to_device(data), spans, linked=True, index=True,
                                                      checkpoint_bytes=65536, block_checksum=True)
    with ix:
        assert [(j.in_off, j.in_len) for j in (ix.jobs[i] for i in range(len(recs)))] == where
        moved = to_device(to_host(frames), 3)
        assert moved.data_ptr() != frames.data_ptr()
        frames.fill_(0)
        check_delivered(deliver(ix, moved, ranges), ranges, recs)
