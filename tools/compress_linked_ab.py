#!/usr/bin/env python3
"""What linked blocks cost and gain lz4ada_compress_frames_device (DESIGN.md
section 21).

Rows: one record of 256 MiB of text; 4,096 records of 128 KiB of text; 4,096
records of repeating rows (400 rows of 48 noise bytes and 80 text bytes, three
times over: repeats that cross the 64 KiB boundaries); one record of 256 MiB of
random bytes, where every continuation block pays the seeding and finds
nothing; 65,536 records of 4 KiB of text, where there is no continuation block
and the linked call queues the unlinked call's launches (its bytes are compared:
they differ in FLG and HC of every header alone).  The text is one MiB of
pseudo-text repeated, a period no window sees twice.  Arm "unlinked":
lz4ada_compress_frames_device of the same build.  Arm "linked":
lz4ada_compress_frames_device_linked without a dictionary.  One process; the
arms alternate call by call; median of --reps after --warmup warm-ups, device
events around the synchronous call.  64 KiB blocks, no flag.

    tools/compress_linked_ab.py [--out profiles/compress_linked_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bo-lz4-ada_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.pop("LZ4ADA_BATCH_BYTES", None)
os.environ.pop("LZ4ADA_BATCH_LINKED", None)

import torch  # noqa: E402

import lz4ada  # noqa: E402
from _compress_cases import pseudo_text  # noqa: E402
from _compress_linked_cases import rows_record  # noqa: E402

KiB, MiB = 1 << 10, 1 << 20


def on_device(piece, total):
    """`piece` repeated to `total` bytes, in device memory."""
    one = torch.frombuffer(bytearray(piece), dtype=torch.uint8).to("cuda:0")
    return one.repeat(total // len(piece) + 1)[:total].contiguous()


def arms(t, count, size):
    spans = [(i * size, size) for i in range(count)]
    bound = lz4ada.compress_frames_bound([size] * count)
    out = {k: torch.empty(bound, dtype=torch.uint8, device="cuda:0") for k in ("unlinked", "linked")}
    jobs = lz4ada._compress_jobs(spans)
    opt = lz4ada.CompressOptions(4, 0)
    olen = {k: ctypes.c_int64() for k in out}
    stored = {}

    def unlinked():
        st = lz4ada._lib.lz4ada_compress_frames_device(t.data_ptr(), t.numel(), jobs, count, ctypes.byref(opt),
                                                       out["unlinked"].data_ptr(), bound,
                                                       ctypes.byref(olen["unlinked"]), 0)
        if st:
            raise SystemExit("the unlinked call failed: " + lz4ada._thread_error())
        stored.setdefault("unlinked", sum(jobs[i].stored_blocks for i in range(count)))

    def linked():
        st = lz4ada._lib.lz4ada_compress_frames_device_linked(t.data_ptr(), t.numel(), jobs, count, ctypes.byref(opt),
                                                              None, out["linked"].data_ptr(), bound,
                                                              ctypes.byref(olen["linked"]), 0)
        if st:
            raise SystemExit("the linked call failed: " + lz4ada._thread_error())
        stored.setdefault("linked", sum(jobs[i].stored_blocks for i in range(count)))

    return {"unlinked": unlinked, "linked": linked}, out, olen, stored


def alternate(calls, reps, warmup):
    times = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress_linked_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lines = ["lz4ada_compress_frames_device_linked against the unlinked call of the same build "
             "(tools/compress_linked_ab.py)",
             f"one MI355X, one process, clocks as found; the arms alternate; median of {args.reps} after {args.warmup} "
             "warm-ups (min - max), device events around the synchronous call; 64 KiB blocks, no flag, no dictionary",
             ""]
    text = pseudo_text(MiB, 77)
    rows = rows_record()
    torch.manual_seed(5)
    shapes = [("text 1 x 256 MiB", lambda: on_device(text, 256 * MiB), 1, 256 * MiB),
              ("text 4,096 x 128 KiB", lambda: on_device(text, 4096 * 128 * KiB), 4096, 128 * KiB),
              ("rows 4,096 x 153,600", lambda: on_device(rows, 4096 * len(rows)), 4096, len(rows)),
              ("random 1 x 256 MiB", lambda: torch.randint(0, 256, (256 * MiB,), dtype=torch.uint8, device="cuda:0"),
               1, 256 * MiB),
              ("text 65,536 x 4 KiB", lambda: on_device(text, 65536 * 4 * KiB), 65536, 4 * KiB)]
    for name, make, count, size in shapes:
        t = make()
        total = count * size
        calls, out, olen, stored = arms(t, count, size)
        tm = alternate(calls, args.reps, args.warmup)
        u, k = olen["unlinked"].value, olen["linked"].value
        line = (f"{name:21s} {total:>10d} bytes  unlinked -> {u:>10d} ({u / total:.3f}, {stored['unlinked']} stored) "
                f"{tm['unlinked'][0]:8.3f} ms ({tm['unlinked'][1]:.3f} - {tm['unlinked'][2]:.3f}) "
                f"{total / tm['unlinked'][0] / 1e6:7.2f} GB/s   linked -> {k:>10d} ({k / total:.3f}, {k / u:.3f} of "
                f"unlinked, {stored['linked']} stored) {tm['linked'][0]:8.3f} ms ({tm['linked'][1]:.3f} - "
                f"{tm['linked'][2]:.3f}) {total / tm['linked'][0] / 1e6:7.2f} GB/s   time x"
                f"{tm['linked'][0] / tm['unlinked'][0]:.3f}")
        if size <= 64 * KiB:  # no continuation block: the unlinked call's bytes but for FLG and HC
            differ = int((out["unlinked"][:u] != out["linked"][:k]).sum().item()) if u == k else -1
            line += f"   bytes that differ: {differ} (2 per record: {2 * count})"
        lines.append(line)
        print(line, flush=True)
        del calls, out, t
        lz4ada.release_device_cache()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
