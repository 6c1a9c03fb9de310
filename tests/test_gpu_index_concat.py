"""The seek indexes of several compress calls laid into one
(lz4ada_seek_index_concat).  The yardstick is the index that one
compress call over all the records writes: the concat of the indexes of
consecutive groups of jobs must equal it array for array
(lz4ada_seek_index_arrays_debug), in what it reports, in what it selects and in
what every range through it delivers.  The second yardstick, where the parts'
frames lie apart, is lz4ada_seek_index_build* over the larger buffer.  The
helpers are test_gpu_compress_indexed.py's, copied; same_index also compares
the device arrays."""
import ctypes

import pytest
import torch

import lz4ada
from _compress_cases import KiB, MiB, noise, pseudo_text, record
from _compress_dict_cases import text_dict
from _compress_linked_cases import B, mixed_jobs, rows_record

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4 * KiB


def _jobs():
    """The mixed jobs (lengths 0, 1, 65,536, 65,537, ... among them) and, in
    their middle, a record of 200,000 bytes: four blocks, three checkpoints."""
    data, spans, _ = mixed_jobs()
    big = pseudo_text(200000, 21)
    spans = spans[:len(spans) // 2] + [(len(data) + 1, len(big))] + spans[len(spans) // 2:]
    data += b"\x55" + big
    return data, spans, [data[o:o + n] for o, n in spans]


MIXED = _jobs()
SHAPES = ["plain", "dict3", "dict1024", "dict65536", "linked", "linked_dict65536"]


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


def compress(t, spans, dd=None, dict_id=None, linked=False, checkpoint_bytes=65536, **kw):
    """One indexed call into a canary-filled buffer of bound + GUARD bytes ->
    (the buffer, bytes written, jobs, the index)."""
    bound = lz4ada.compress_frames_bound([n for _, n in spans], dict=dd, dict_id=dict_id, **kw)
    out = torch.full((bound + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    got = lz4ada.compress_frames_device(t.data_ptr() if t.numel() else None, t.numel(), spans, out.data_ptr(), bound,
                                        stream(), dict=dd, dict_id=dict_id, linked=linked, index=True,
                                        checkpoint_bytes=checkpoint_bytes, **kw)
    return (out,) + tuple(got)


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


def all_ranges(recs, blen=B):
    return [r for j, p in enumerate(recs) for r in block_ranges(j, p, blen) if r[1] >= 0 and r[2] >= 0]


def build(buf, spans, linked=False, checkpoint_bytes=65536, dt=None):
    return lz4ada.SeekIndex.build(buf.data_ptr(), buf.numel(), spans, stream(), linked=linked,
                                  checkpoint_bytes=checkpoint_bytes, dict=dt.data_ptr() if dt is not None else None,
                                  dict_len=dt.numel() if dt is not None else 0)


def frame_report(idx):
    return [(j.in_off, j.in_len, j.out_off, j.out_len, j.consumed, j.status, j.reason)
            for j in (idx.jobs[i] for i in range(idx.njobs))]


def deliver(idx, frames, ranges):
    got, arr = lz4ada.decode_ranges_tensor(idx, frames, ranges)
    got = to_host(got)
    return [(arr[k].status, arr[k].reason, arr[k].out_off, arr[k].out_len,
             got[arr[k].out_off:arr[k].out_off + arr[k].out_len]) for k in range(len(ranges))]


def same_index(ix, want, frames, ranges):
    """Everything two indexes over the same frames can be asked, and their
    device arrays."""
    a, b = lz4ada.seek_index_arrays_debug(ix), lz4ada.seek_index_arrays_debug(want)
    for name in b:
        assert a[name] == b[name], name
    assert ix.in_len == want.in_len and ix.njobs == want.njobs
    assert frame_report(ix) == frame_report(want)
    assert lz4ada.seek_index_debug(ix) == lz4ada.seek_index_debug(want)
    assert ix.device_bytes == want.device_bytes
    assert lz4ada.ranges_select_debug(ix, ranges) == lz4ada.ranges_select_debug(want, ranges)
    assert lz4ada.seek_index_store_debug(ix) == lz4ada.seek_index_store_debug(want)
    a, b = deliver(ix, frames, ranges), deliver(want, frames, ranges)
    for k in range(len(ranges)):
        assert a[k] == b[k], (k, ranges[k], a[k][:4], b[k][:4])
    return a


def check_delivered(res, ranges, recs):
    for k, (j, off, n) in enumerate(ranges):
        want = recs[j][off:off + n]
        assert res[k][0] == 0 and res[k][3] == len(want) and res[k][4] == want, (k, ranges[k], res[k][:4])


def shape_args(shape):
    """-> (keywords of compress, the dictionary's tensor or None)."""
    dl = int(shape.split("dict")[1]) if "dict" in shape else None
    dt = to_device(text_dict(dl), dl % 3) if dl else None
    return dict(dd=(dt.data_ptr(), dl) if dl else None, dict_id=5 if dl == 1024 else None,
                linked=shape.startswith("linked")), dt


def cut(spans, ngroups):
    n = len(spans)
    return [spans[n * g // ngroups:n * (g + 1) // ngroups] for g in range(ngroups)]


def parts_of(t, groups, **kw):
    """One indexed call per group -> ([(buffer, bytes, jobs, index)], the
    bases of the frames laid back to back, their total)."""
    parts = [compress(t, g, **kw) for g in groups]
    bases, at = [], 0
    for _, n, _, _ in parts:
        bases.append(at)
        at += n
    return parts, bases, at


def free_all(parts):
    for p in parts:
        p[3].free()


# ------------------------------------------------------------ 1. the yardstick

@pytest.mark.parametrize("shape", SHAPES)
def test_concat_equals_the_one_call(shape, mixed_on_device):
    data, spans, plains = MIXED
    kw, dt = shape_args(shape)
    ranges = all_ranges(plains)
    out, n, jobs, one = compress(mixed_on_device, spans, block_checksum=True, **kw)
    whole = to_host(out[:n])
    with one:
        for ngroups in (2, 3):
            parts, bases, total = parts_of(mixed_on_device, cut(spans, ngroups), block_checksum=True, **kw)
            assert b"".join(to_host(o[:m]) for o, m, _, _ in parts) == whole and total == n
            with lz4ada.SeekIndex.concat([p[3] for p in parts], bases, n, stream()) as cat:
                st = lz4ada.last_batch_stats()
                assert all(getattr(st, f) == 0 for f, _ in st._fields_)
                free_all(parts)
                res = same_index(cat, one, out[:n], ranges)
                delivered = [k for k in range(len(ranges)) if res[k][0] == 0]
                check_delivered([res[k] for k in delivered], [ranges[k] for k in delivered], plains)
                assert len(delivered) > len(ranges) * 9 // 10


# ----------------------------------------------------------- 2. associativity

def test_concat_is_associative(mixed_on_device):
    """Checkpoints every 131,072 bytes: K = 2."""
    data, spans, plains = MIXED
    kw, dt = shape_args("linked_dict65536")
    ranges = all_ranges(plains)
    parts, bases, n = parts_of(mixed_on_device, cut(spans, 3), checkpoint_bytes=131072, **kw)
    frames = to_device(b"".join(to_host(o[:m]) for o, m, _, _ in parts))
    x = [p[3] for p in parts]
    with lz4ada.SeekIndex.concat(x[:2], bases[:2], bases[2], stream()) as x12, \
            lz4ada.SeekIndex.concat([x12, x[2]], [0, bases[2]], n, stream()) as nested, \
            lz4ada.SeekIndex.concat(x, bases, n, stream()) as flat:
        assert 0 < len(lz4ada.seek_index_store_debug(flat)) < 65536 * sum(len(p) // B for p in plains)
        check = same_index(nested, flat, frames, ranges)
        assert any(r[0] == 0 and r[3] > 2 * B for r in check)
    free_all(parts)


# ------------------------------------ 3. gaps, and a build as the second yardstick

def index_records():
    return [pseudo_text(n, n + 3) for n in (2 * B + 1, B + 1024, 4 * B + 777, 3 * B)] + \
        [rows_record(), b"", record(1), record(13)]


def spread(chunks, gaps):
    """The byte strings laid into one buffer with gaps[i] canary bytes in front
    of the i-th -> (the buffer's bytes, where each lies)."""
    buf, where = b"", []
    for c, g in zip(chunks, gaps):
        buf += bytes([CANARY]) * g
        where.append(len(buf))
        buf += c
    return buf + bytes([CANARY]) * 17, where


@pytest.mark.parametrize("shape", ["plain", "dict65536", "linked", "linked_dict65536"])
def test_parts_apart_equal_a_build(shape):
    recs = index_records()
    groups = [recs[:3], recs[3:5], recs[5:]]
    kw, dt = shape_args(shape)
    kw.pop("dict_id")
    linked = kw["linked"]
    parts, chunks, spans, plains = [], [], [], []
    gaps = [1, 255, 4096]
    for g, group in enumerate(groups):
        data, where = laid_out(group)
        out, n, jobs, ix = compress(to_device(data), where, block_checksum=True, **kw)
        frames = [(jobs[i].out_off, jobs[i].out_len) for i in range(len(group))]
        if g == 1:
            # a built index whose jobs come in falling in_off: its pos is not the identity
            ix.free()
            frames = frames[::-1]
            group = group[::-1]
            ix = build(out[:n], frames, linked, dt=dt)
        parts.append(ix)
        chunks.append(to_host(out[:n]))
        spans.append(frames)
        plains += group
    buf, bases = spread(chunks, gaps)
    t = to_device(buf)
    whole_spans = [(b + o, m) for b, fr in zip(bases, spans) for o, m in fr]
    ranges = all_ranges(plains)
    with lz4ada.SeekIndex.concat(parts, bases, len(buf), stream()) as cat, \
            build(t, whole_spans, linked, dt=dt) as built:
        assert all(built.jobs[j].status == 0 and built.jobs[j].out_len == len(p) for j, p in enumerate(plains)), \
            "the build must accept every frame of this comparison"
        res = same_index(cat, built, t, ranges)
        check_delivered(res, ranges, plains)
        # the built part's jobs keep their numbers: job 3 is the rows record, job 4 the 3 B text
        assert frame_report(cat)[3][0] > frame_report(cat)[4][0] and frame_report(cat)[3][3] == len(rows_record())
    for p in parts:
        p.free()


# ------------------------------------------ 4. a frame the index did not take

def test_a_frame_the_index_did_not_take():
    """1 MiB blocks: 1 MiB of noise is stored and falls to the lone-block rule
    (LZ4ADA_BATCH_BIG_BLOCK), in the middle of the middle part."""
    groups = [[pseudo_text(70000, 1), record(13)], [pseudo_text(MiB + 70000, 2), noise(MiB, 6), pseudo_text(70000, 3)],
              [record(13), pseudo_text(200000, 4)]]
    recs = [p for g in groups for p in g]
    data, spans = laid_out(recs)
    t = to_device(data)
    ranges = all_ranges(recs, MiB)
    kw = dict(linked=True, block=MiB, block_checksum=True)
    out, n, jobs, one = compress(t, spans, **kw)
    parts, bases, total = parts_of(t, [spans[:2], spans[2:5], spans[5:]], **kw)
    with one, lz4ada.SeekIndex.concat([p[3] for p in parts], bases, n, stream()) as cat:
        free_all(parts)
        assert total == n
        rep = frame_report(cat)
        assert [(r[5], r[6], r[3]) for r in rep] == [(0, 0, len(p)) if j != 3 else
                                                     (lz4ada.EXACT_PATH, lz4ada.BATCH_BIG_BLOCK, 0)
                                                     for j, p in enumerate(recs)]
        arrays = lz4ada.seek_index_arrays_debug(cat)
        assert arrays["first"][3] == arrays["first"][4] and arrays["ckfirst"][3] == arrays["ckfirst"][4]
        assert arrays["nckpt"] == 1  # the text record of two blocks' one
        res = same_index(cat, one, out[:n], ranges)
        taken = [k for k, r in enumerate(ranges) if r[0] != 3]
        check_delivered([res[k] for k in taken], [ranges[k] for k in taken], recs)
        assert all(res[k][:2] == (lz4ada.EXACT_PATH, lz4ada.BATCH_BIG_BLOCK) and res[k][3] == 0
                   for k in range(len(ranges)) if k not in taken)
        assert cat.device_bytes == one.device_bytes


# ------------------------------------------- 5. linked and unlinked parts mixed

def test_linked_and_unlinked_parts():
    recs = index_records()
    groups = [recs[:2], recs[2:5], recs[5:]]
    parts, chunks, spans = [], [], []
    for g, group in enumerate(groups):
        data, where = laid_out(group)
        out, n, jobs, ix = compress(to_device(data), where, linked=g == 1, block_checksum=True)
        parts.append(ix)
        chunks.append(to_host(out[:n]))
        spans.append([(jobs[i].out_off, jobs[i].out_len) for i in range(len(group))])
    buf, bases = spread(chunks, [0, 0, 0])
    t = to_device(buf)
    ranges = all_ranges(recs)
    with lz4ada.SeekIndex.concat(parts, bases, len(buf), stream()) as cat, \
            build(t, [(b + o, m) for b, fr in zip(bases, spans) for o, m in fr], True) as built:
        assert all(built.jobs[j].status == 0 for j in range(len(recs)))
        arrays = lz4ada.seek_index_arrays_debug(cat)
        assert arrays["kgrp"] == [0, 0, 1, 1, 1, 0, 0, 0] and arrays["ckfirst"] == [0, 0, 0, 4, 6, 8, 8, 8, 8]
        check_delivered(same_index(cat, built, t, ranges), ranges, recs)
    for p in parts:
        p.free()


# ------------------------------------------------------------ 6. dictionaries

def test_dictionary_parts():
    recs = index_records()[:3] + [record(13)]
    data, spans = laid_out(recs)
    t = to_device(data)
    ranges = all_ranges(recs)
    d = text_dict(65536)
    da, db = to_device(d, 2), to_device(d, 5)  # equal bytes in two allocations
    dc = to_device(d[:30000] + bytes([d[30000] ^ 1]) + d[30001:], 1)
    a = compress(t, spans[:2], (da.data_ptr(), 65536), linked=True)
    b = compress(t, spans[2:], (db.data_ptr(), 65536), linked=True)
    c = compress(t, spans[2:], (dc.data_ptr(), 65536), linked=True)
    s = compress(t, spans[2:], (dc.data_ptr(), 1024), linked=True)
    plain = compress(t, spans[2:], linked=True)
    frames = to_device(to_host(a[0][:a[1]]) + to_host(b[0][:b[1]]))
    with lz4ada.SeekIndex.concat([a[3], b[3]], [0, a[1]], a[1] + b[1], stream()) as cat:
        da.fill_(0x33)
        db.fill_(0x44)
        torch.cuda.synchronize()
        check_delivered(deliver(cat, frames, ranges), ranges, recs)
    for other in (c, s, plain):  # a differing byte; another dict_used; a dictionary part beside a plain one
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.SeekIndex.concat([a[3], other[3]], [0, a[1]], a[1] + other[1], stream())
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.SeekIndex.concat([other[3], a[3]], [0, other[1]], a[1] + other[1], stream())
    # a refused call leaves the parts usable
    with lz4ada.SeekIndex.concat([a[3], b[3]], [0, a[1]], a[1] + b[1], stream()) as cat:
        check_delivered(deliver(cat, frames, ranges), ranges, recs)
    check_delivered(deliver(a[3], a[0][:a[1]], all_ranges(recs[:2])), all_ranges(recs[:2]), recs[:2])
    free_all([a, b, c, s, plain])


# --------------------------------------------- 7. repeated prefixes on the device

def test_three_hundred_parts():
    """One record of 40..140 bytes per part, with parts without a job and parts
    of one 0-byte record scattered among them: more frames than a workgroup has
    lanes, and prefixes that repeat."""
    lens = [40 + (37 * i) % 101 for i in range(300)]
    for i in range(0, 300, 7):
        lens[i] = None  # no job
    for i in list(range(3, 300, 11)) + [297, 298]:
        lens[i] = 0  # one record of 0 bytes: a frame without a block
    lens[0] = lens[1] = lens[299] = None
    recs = [pseudo_text(n, 500 + i) for i, n in enumerate(lens) if n is not None]
    data, spans = laid_out(recs)
    t = to_device(data)
    groups, at = [], 0
    for n in lens:
        groups.append([] if n is None else [spans[at]])
        at += n is not None
    kw = dict(linked=True, block_checksum=True)
    out, n, jobs, one = compress(t, spans, **kw)
    parts, bases, total = parts_of(t, groups, **kw)
    assert total == n and len(parts) == 300 and len(recs) > 256
    ranges = [(j, 0, len(p)) for j, p in enumerate(recs)] + [(j, len(p) // 2, 7) for j, p in enumerate(recs)]
    with one, lz4ada.SeekIndex.concat([p[3] for p in parts], bases, n, stream()) as cat:
        free_all(parts)
        check_delivered(same_index(cat, one, out[:n], ranges), ranges, recs)


# --------------------------------- 8. one part at a new base; the same part twice

def test_one_part_moved_and_named_twice():
    recs = index_records()
    data, spans = laid_out(recs)
    out, n, jobs, ix = compress(to_device(data), spans, linked=True, block_checksum=True)
    chunk = to_host(out[:n])
    frames = [(jobs[i].out_off, jobs[i].out_len) for i in range(len(recs))]
    with ix:
        buf, (base,) = spread([chunk], [777])
        t = to_device(buf)
        with lz4ada.SeekIndex.concat([ix], [base], len(buf), stream()) as cat, \
                build(t, [(base + o, m) for o, m in frames], True) as built:
            check_delivered(same_index(cat, built, t, all_ranges(recs)), all_ranges(recs), recs)
            with pytest.raises(lz4ada.AssertionFailure):
                lz4ada.decode_ranges_tensor(cat, out[:n], [(0, 0, 1)])  # the part's in_len is not the result's
        buf, bases = spread([chunk, chunk], [0, 255])
        t = to_device(buf)
        with lz4ada.SeekIndex.concat([ix, ix], bases, len(buf), stream()) as cat, \
                build(t, [(b + o, m) for b in bases for o, m in frames], True) as built:
            check_delivered(same_index(cat, built, t, all_ranges(recs + recs)), all_ranges(recs + recs), recs + recs)
        with pytest.raises(lz4ada.AssertionFailure):
            lz4ada.SeekIndex.concat([ix, ix], [0, n - 1], 2 * n, stream())


# ---------------------------------------------------------------- 9. lifetime

def test_the_result_owns_everything(mixed_on_device):
    data, spans, plains = MIXED
    kw, dt = shape_args("linked_dict65536")
    ranges = all_ranges(plains)
    parts, bases, n = parts_of(mixed_on_device, cut(spans, 3), block_checksum=True, **kw)
    frames = to_device(b"".join(to_host(o[:m]) for o, m, _, _ in parts))
    cat = lz4ada.SeekIndex.concat([p[3] for p in parts], bases, n, stream())
    want = deliver(cat, frames, ranges)
    free_all(parts)
    dt.fill_(0)
    del parts, dt
    lz4ada.release_device_cache()
    torch.cuda.synchronize()
    with cat:
        got = deliver(cat, frames, ranges)
        assert got == want
        delivered = [k for k in range(len(ranges)) if got[k][0] == 0]
        check_delivered([got[k] for k in delivered], [ranges[k] for k in delivered], plains)
        assert len(delivered) > len(ranges) * 9 // 10


# -------------------------------------------- 10. the writer's advantage survives

def test_past_the_linked_limit(monkeypatch):
    """The build refuses a linked frame over lz4ada_batch_linked_max(); the
    writer's index takes it, and so does a concat that holds it."""
    first = [pseudo_text(B + 1024, 3), record(13)]
    rec = pseudo_text(4 * B + 777, 9)
    monkeypatch.setenv("LZ4ADA_BATCH_LINKED_MAX", "131072")
    d1, s1 = laid_out(first)
    a = compress(to_device(d1), s1, linked=True, block_checksum=True)
    b = compress(to_device(rec), [(0, len(rec))], linked=True, block_checksum=True)
    buf = to_host(a[0][:a[1]]) + to_host(b[0][:b[1]])
    t = to_device(buf)
    with build(t, [(a[1], b[1])], True) as built:
        assert (built.jobs[0].status, built.jobs[0].reason) == (lz4ada.EXACT_PATH, lz4ada.BATCH_LINKED)
    with lz4ada.SeekIndex.concat([a[3], b[3]], [0, a[1]], len(buf), stream()) as cat:
        free_all([a, b])
        assert frame_report(cat)[2] == (a[1], b[1], 0, len(rec), 0, 0, 0)
        recs = first + [rec]
        check_delivered(deliver(cat, t, all_ranges(recs)), all_ranges(recs), recs)
