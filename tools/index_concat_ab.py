#!/usr/bin/env python3
"""What it costs to lay the seek indexes of several compress calls into one
(lz4ada_seek_index_concat) against building the index
over all the frames again.

Rows: section 22's four shapes, each written in 8 batches by 8 indexed
compress calls whose frames lie back to back: 4,096 records of 128 KiB of text,
linked; 4,096 records of repeating rows (153,600 bytes), linked; 65,536 records
of 4 KiB of text against a 64 KiB dictionary; and a store whose first batch is
one record of 256 MiB of text, linked, followed by 7 batches of 64 records of
128 KiB, which the build cannot index whole: it refuses the large record (a
linked frame over lz4ada_batch_linked_max()).  Arm R: lz4ada_seek_index_build_dict
over all the frames, what a caller does without the concat.  Arm M: the concat
of the 8 per-batch indexes.  Arm A: appending, the concat of a 7-batch index
with the 8th.  Then 1,024 random ranges of 4 KiB through the concat (M's) and
through the index one compress call over all the records writes, alternating;
both must deliver the same bytes.  One process; the arms alternate call by
call; median of --reps after --warmup warm-ups, device events around the
synchronous calls (an index is freed outside them).  64 KiB blocks, no flag,
the default checkpoint distance.

    tools/index_concat_ab.py [--out profiles/index_concat_ab.txt]
"""
import argparse
import ctypes
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
for name in ("LZ4ADA_BATCH_BYTES", "LZ4ADA_BATCH_LINKED", "LZ4ADA_BATCH_LINKED_MAX"):
    os.environ.pop(name, None)

import torch  # noqa: E402

import lz4ada  # noqa: E402
from _compress_cases import pseudo_text  # noqa: E402
from _compress_dict_cases import text_dict  # noqa: E402
from _compress_linked_cases import rows_record  # noqa: E402

KiB, MiB = 1 << 10, 1 << 20
BATCHES = 8


def on_device(piece, total):
    """`piece` repeated to `total` bytes, in device memory."""
    one = torch.frombuffer(bytearray(piece), dtype=torch.uint8).to("cuda:0")
    return one.repeat(total // len(piece) + 1)[:total].contiguous()


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), res


def stats(v):
    return statistics.median(v), min(v), max(v)


def fmt(name, s):
    return f"{name} {s[0]:8.3f} ms ({s[1]:.3f} - {s[2]:.3f})"


def written(t, batches, linked, dt):
    """The store: every batch by an indexed call of its own, back to back in
    one buffer -> (the buffer, bytes, the parts, their bases, every frame's span)."""
    every = [s for b in batches for s in b]
    out = torch.empty(lz4ada.compress_frames_bound([n for _, n in every]), dtype=torch.uint8, device="cuda:0")
    dd = (dt.data_ptr(), dt.numel()) if dt is not None else None
    parts, bases, frames, at = [], [], [], 0
    for spans in batches:
        n, jobs, ix = lz4ada.compress_frames_device(t.data_ptr(), t.numel(), spans, out.data_ptr() + at,
                                                    out.numel() - at, 0, dict=dd, linked=linked, index=True)
        parts.append(ix)
        bases.append(at)
        frames += [(at + jobs[i].out_off, jobs[i].out_len) for i in range(len(spans))]
        at += n
    return out, at, parts, bases, frames


def one_call(t, batches, linked, dt, out, n):
    """The yardstick: one indexed call over all the records; its frames are the store's."""
    every = [s for b in batches for s in b]
    dd = (dt.data_ptr(), dt.numel()) if dt is not None else None
    again = torch.empty(out.numel(), dtype=torch.uint8, device="cuda:0")
    m, jobs, ix = lz4ada.compress_frames_device(t.data_ptr(), t.numel(), every, again.data_ptr(), again.numel(), 0,
                                                dict=dd, linked=linked, index=True)
    if m != n or not torch.equal(again[:n], out[:n]):
        raise SystemExit("the batches' frames are not the one call's")
    return ix


def concat(parts, bases, n):
    """The C call alone (SeekIndex.concat also copies the parts' job reports)."""
    arr = (ctypes.c_void_p * len(parts))(*[p._ptr for p in parts])
    base = (ctypes.c_int64 * len(parts))(*bases)

    def call():
        ptr = ctypes.c_void_p()
        if lz4ada._lib.lz4ada_seek_index_concat(arr, base, len(parts), n, ctypes.byref(ptr), 0):
            raise SystemExit("the concat failed: " + lz4ada._thread_error())
        return lz4ada.SeekIndex(ptr.value, None, 0, n)
    return call


def arms(out, n, parts, bases, frames, linked, dt):
    L = lz4ada._lib
    count = len(frames)
    jobs = lz4ada._device_jobs(frames)
    sopt = lz4ada.SeekOptions(lz4ada.SEEK_LINKED if linked else 0, 0, 0)
    dd = lz4ada.DeviceDict(dt.data_ptr(), dt.numel(), 0, 0) if dt is not None else None
    seen = {}
    head = concat(parts[:-1], bases[:-1], bases[-1])()  # the store before its last batch
    merge, append = concat(parts, bases, n), concat([head, parts[-1]], [0, bases[-1]], n)

    def r():
        ptr = ctypes.c_void_p()
        if L.lz4ada_seek_index_build_dict(out.data_ptr(), n, jobs, count, ctypes.byref(sopt),
                                          ctypes.byref(dd) if dd else None, ctypes.byref(ptr), 0):
            raise SystemExit("the build failed: " + lz4ada._thread_error())
        idx = lz4ada.SeekIndex(ptr.value, jobs, count, n)
        seen.setdefault("R", (idx.device_bytes, sum(jobs[i].status == 0 for i in range(count))))
        return idx

    def m():
        idx = merge()
        seen.setdefault("M", idx.device_bytes)
        return idx

    def a():
        return append()

    return {"R": r, "M": m, "A": a}, seen, head


def alternate(calls, reps, warmup):
    times = {k: [] for k in calls}
    for i in range(warmup + reps):
        for k, call in calls.items():
            ms, idx = timed(call)
            idx.free()
            if i >= warmup:
                times[k].append(ms)
    return {k: stats(v) for k, v in times.items()}


def ranges_time(cat, one, out, n, frames_len, reps, warmup):
    """1,024 random 4 KiB ranges over the records, through both indexes."""
    rnd = random.Random(11)
    ranges = []
    for _ in range(1024):
        j = rnd.randrange(len(frames_len))
        ranges.append((j, rnd.randrange(max(frames_len[j] - 4 * KiB, 1)), 4 * KiB))
    got = {}
    times = {"concat": [], "one call": []}
    for i in range(warmup + reps):
        for k, idx in (("concat", cat), ("one call", one)):
            dst = torch.zeros(1024 * 4 * KiB, dtype=torch.uint8, device="cuda:0")
            arr, _ = lz4ada._frame_ranges(ranges)
            ms, _ = timed(lambda: lz4ada.decode_ranges_device(idx, out.data_ptr(), n, arr, dst.data_ptr(),
                                                              dst.numel(), 0))
            if i >= warmup:
                times[k].append(ms)
            got[k] = (dst, [(arr[q].status, arr[q].out_off, arr[q].out_len) for q in range(1024)])
    if got["concat"][1] != got["one call"][1] or not torch.equal(got["concat"][0], got["one call"][0]):
        raise SystemExit("the ranges through the concat are not those through the one call's index")
    good = sum(s == 0 for s, _, _ in got["concat"][1])
    return stats(times["concat"]), stats(times["one call"]), good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_concat_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lines = ["lz4ada_seek_index_concat over the indexes of 8 batches (M) and of a 7-batch index with the 8th (A) against "
             "lz4ada_seek_index_build_dict over all the frames (R) (tools/index_concat_ab.py)",
             f"one MI355X, one process, clocks as found; the arms alternate; median of {args.reps} after {args.warmup} "
             "warm-ups (min - max), device events around the synchronous calls; 64 KiB blocks, no flag, the default "
             "checkpoint distance (1 MiB); the ranges: 1,024 random ranges of 4 KiB, through M's index and through "
             "the index of one compress call over all the records, alternating, the same bytes from both",
             ""]
    text = pseudo_text(MiB, 77)
    rows = rows_record()

    def even(count, size):
        spans = [(i * size, size) for i in range(count)]
        return [spans[count * b // BATCHES:count * (b + 1) // BATCHES] for b in range(BATCHES)]

    big = [[(0, 256 * MiB)]] + [[(256 * MiB + (64 * b + i) * 128 * KiB, 128 * KiB) for i in range(64)]
                                for b in range(BATCHES - 1)]
    shapes = [("text 4,096 x 128 KiB, linked", lambda: on_device(text, 4096 * 128 * KiB), even(4096, 128 * KiB), True,
               False),
              ("rows 4,096 x 153,600, linked", lambda: on_device(rows, 4096 * len(rows)), even(4096, len(rows)), True,
               False),
              ("text 65,536 x 4 KiB, 64 KiB dictionary", lambda: on_device(text, 65536 * 4 * KiB), even(65536, 4 * KiB),
               False, True),
              ("text 1 x 256 MiB + 448 x 128 KiB, linked", lambda: on_device(text, 256 * MiB + 448 * 128 * KiB), big, True,
               False)]
    for name, make, batches, linked, dictionary in shapes:
        t = make()
        dt = torch.frombuffer(bytearray(text_dict(65536)), dtype=torch.uint8).to("cuda:0") if dictionary else None
        out, n, parts, bases, frames = written(t, batches, linked, dt)
        one = one_call(t, batches, linked, dt, out, n)
        calls, seen, head = arms(out, n, parts, bases, frames, linked, dt)
        tm = alternate(calls, args.reps, args.warmup)
        count = len(frames)
        line = (f"{name:42s} {count:>6d} frames, {n:>10d} bytes   {fmt('R', tm['R'])}   {fmt('M', tm['M'])}   "
                f"{fmt('A', tm['A'])}   index bytes R {seen['R'][0]} ({seen['R'][1]} of {count} frames taken")
        line += ": the build refuses the 256 MiB record)" if seen["R"][1] != count else ")"
        line += f"  M {seen['M']}  one call {one.device_bytes}"
        with concat(parts, bases, n)() as cat:
            lens = [s[1] for b in batches for s in b]
            rc, ro, good = ranges_time(cat, one, out, n, lens, args.reps, args.warmup)
        line += f"   ranges: {fmt('concat', rc)}   {fmt('one call', ro)}, {good} of 1,024 delivered"
        lines.append(line)
        print(line, flush=True)
        for ix in parts + [head, one]:
            ix.free()
        del calls, out, t, seen, parts, head, one
        lz4ada.release_device_cache()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
