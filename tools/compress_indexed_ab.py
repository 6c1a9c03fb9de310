#!/usr/bin/env python3
"""What the seek index costs when the compress call writes it
(lz4ada_compress_frames_device_indexed) against building
it over the frames just written.

Rows, from section 21's table: 4,096 records of 128 KiB of text, linked; 4,096
records of repeating rows (153,600 bytes), linked; 65,536 records of 4 KiB of
text against a 64 KiB dictionary; one record of 256 MiB of text, linked, which
the build refuses (a linked frame over lz4ada_batch_linked_max()), so that row
has no arm A and reports instead 1,024 random ranges of 4 KiB through the
writer's index.  Arm C: the existing compress call alone.  Arm A: that call
followed by the matching lz4ada_seek_index_build*, what a caller does today.
Arm B: the indexed call.  One process; the arms alternate call by call; median
of --reps after --warmup warm-ups, device events around the synchronous calls
(an index is freed outside them).  64 KiB blocks, no flag, the default
checkpoint distance.

    tools/compress_indexed_ab.py [--out profiles/compress_indexed_ab.txt]
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


def on_device(piece, total):
    """`piece` repeated to `total` bytes, in device memory."""
    one = torch.frombuffer(bytearray(piece), dtype=torch.uint8).to("cuda:0")
    return one.repeat(total // len(piece) + 1)[:total].contiguous()


def arms(t, count, size, linked, dt, with_build):
    """The three arms over arrays made once: nothing but the C-ABI calls is timed."""
    spans = [(i * size, size) for i in range(count)]
    bound = lz4ada.compress_frames_bound([size] * count)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda:0")
    jobs, frames = lz4ada._compress_jobs(spans), lz4ada._device_jobs(spans)
    opt = lz4ada.CompressOptions(4, 0)
    cd = lz4ada.CompressDict(dt.data_ptr(), dt.numel(), 0, 0) if dt is not None else None
    dd = lz4ada.DeviceDict(dt.data_ptr(), dt.numel(), 0, 0) if dt is not None else None
    xopt = lz4ada.CompressIndexOptions(lz4ada.COMP_INDEX_LINKED if linked else 0, 0, 0)
    sopt = lz4ada.SeekOptions(lz4ada.SEEK_LINKED if linked else 0, 0, 0)
    n = ctypes.c_int64()
    seen = {}
    L = lz4ada._lib

    def ok(st, what):
        if st:
            raise SystemExit(f"{what} failed: " + lz4ada._thread_error())

    def compress():
        if linked:
            st = L.lz4ada_compress_frames_device_linked(t.data_ptr(), t.numel(), jobs, count, ctypes.byref(opt),
                                                        ctypes.byref(cd) if cd else None, out.data_ptr(), bound,
                                                        ctypes.byref(n), 0)
        elif cd:
            st = L.lz4ada_compress_frames_device_dict(t.data_ptr(), t.numel(), jobs, count, ctypes.byref(opt),
                                                      ctypes.byref(cd), out.data_ptr(), bound, ctypes.byref(n), 0)
        else:
            st = L.lz4ada_compress_frames_device(t.data_ptr(), t.numel(), jobs, count, ctypes.byref(opt),
                                                 out.data_ptr(), bound, ctypes.byref(n), 0)
        ok(st, "the compress call")

    def taken():
        return sum(frames[i].status == 0 for i in range(count))

    def c():
        compress()
        seen["frames"] = n.value
        return None

    def a():
        compress()
        if "where" not in seen:  # (a warm-up: the frames' places do not change between calls)
            for i in range(count):
                frames[i].in_off, frames[i].in_len = jobs[i].out_off, jobs[i].out_len
            seen["where"] = True
        ptr = ctypes.c_void_p()
        ok(L.lz4ada_seek_index_build_dict(out.data_ptr(), n.value, frames, count, ctypes.byref(sopt),
                                          ctypes.byref(dd) if dd else None, ctypes.byref(ptr), 0), "the build")
        idx = lz4ada.SeekIndex(ptr.value, frames, count, n.value)
        if "A" not in seen:
            seen["A"] = (idx.device_bytes, taken())
        return idx

    def b():
        ptr = ctypes.c_void_p()
        ok(L.lz4ada_compress_frames_device_indexed(t.data_ptr(), t.numel(), jobs, count, ctypes.byref(opt),
                                                   ctypes.byref(cd) if cd else None, ctypes.byref(xopt),
                                                   out.data_ptr(), bound, ctypes.byref(n), frames, ctypes.byref(ptr),
                                                   0), "the indexed call")
        idx = lz4ada.SeekIndex(ptr.value, frames, count, n.value)
        if "B" not in seen:
            seen["B"] = (idx.device_bytes, taken())
        seen["index"], seen["n"] = idx, n.value
        return idx

    calls = {"C": c, "B": b}
    if with_build:
        calls = {"C": c, "A": a, "B": b}
    return calls, out, seen


def alternate(calls, reps, warmup):
    times = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            idx = call()
            b.record()
            b.synchronize()
            if idx is not None and not (k == "B" and r == warmup + reps - 1):
                idx.free()  # (the last B's is kept for the ranges)
            if r >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def ranges_time(idx, out, n, size, reps, warmup):
    """1,024 random 4 KiB ranges of the one frame through the index."""
    rnd = random.Random(11)
    ranges = [(0, rnd.randrange(size - 4 * KiB), 4 * KiB) for _ in range(1024)]
    dst, times = torch.empty(1024 * 4 * KiB, dtype=torch.uint8, device="cuda:0"), []
    arr, _ = lz4ada._frame_ranges(ranges)
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lz4ada.decode_ranges_device(idx, out.data_ptr(), n, arr, dst.data_ptr(), dst.numel(), 0)
        b.record()
        b.synchronize()
        if r >= warmup:
            times.append(a.elapsed_time(b))
    good = sum(arr[k].status == 0 for k in range(1024))
    return statistics.median(times), min(times), max(times), good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress_indexed_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lines = ["lz4ada_compress_frames_device_indexed (B) against the existing compress call alone (C) and followed by "
             "the matching lz4ada_seek_index_build* (A), of the same build (tools/compress_indexed_ab.py)",
             f"one MI355X, one process, clocks as found; the arms alternate; median of {args.reps} after {args.warmup} "
             "warm-ups (min - max), device events around the synchronous calls; 64 KiB blocks, no flag, the default "
             "checkpoint distance (1 MiB)",
             ""]
    text = pseudo_text(MiB, 77)
    rows = rows_record()
    shapes = [("text 4,096 x 128 KiB, linked", lambda: on_device(text, 4096 * 128 * KiB), 4096, 128 * KiB, True, False),
              ("rows 4,096 x 153,600, linked", lambda: on_device(rows, 4096 * len(rows)), 4096, len(rows), True, False),
              ("text 65,536 x 4 KiB, 64 KiB dictionary", lambda: on_device(text, 65536 * 4 * KiB), 65536, 4 * KiB, False,
               True),
              ("text 1 x 256 MiB, linked", lambda: on_device(text, 256 * MiB), 1, 256 * MiB, True, False)]
    for name, make, count, size, linked, dictionary in shapes:
        t = make()
        dt = torch.frombuffer(bytearray(text_dict(65536)), dtype=torch.uint8).to("cuda:0") if dictionary else None
        with_build = count > 1
        calls, out, seen = arms(t, count, size, linked, dt, with_build)
        tm = alternate(calls, args.reps, args.warmup)
        total = count * size

        def fmt(k):
            return f"{k} {tm[k][0]:8.3f} ms ({tm[k][1]:.3f} - {tm[k][2]:.3f})"

        line = f"{name:40s} {total:>10d} bytes -> {seen['frames']:>10d}   {fmt('C')}   "
        if with_build:
            line += (f"{fmt('A')}   {fmt('B')}   A - C {tm['A'][0] - tm['C'][0]:7.3f} ms   B - C "
                     f"{tm['B'][0] - tm['C'][0]:7.3f} ms   index bytes A {seen['A'][0]} ({seen['A'][1]} of {count} "
                     f"frames taken)  B {seen['B'][0]} ({seen['B'][1]} taken)")
        else:
            rt = ranges_time(seen["index"], out, seen["n"], size, args.reps, args.warmup)
            line += (f"(A: the build refuses the frame)   {fmt('B')}   B - C {tm['B'][0] - tm['C'][0]:7.3f} ms   "
                     f"index bytes B {seen['B'][0]} ({seen['B'][1]} taken)   1,024 random 4 KiB ranges "
                     f"{rt[0]:.3f} ms ({rt[1]:.3f} - {rt[2]:.3f}), {rt[3]} delivered")
        seen["index"].free()
        lines.append(line)
        print(line, flush=True)
        del calls, out, t, seen
        lz4ada.release_device_cache()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
