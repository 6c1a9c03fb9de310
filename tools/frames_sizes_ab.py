#!/usr/bin/env python3
"""Exact sizes and the decode laid out by them against the decode laid out by
the bound.  Two batches in device memory: the 4,096
single-block 64 KiB frames of tools/frames_device_ab.py, and 4,096 frames with
a 4 MiB block maximum and 1-3 KiB of payload each (the frames of
tests/test_gpu_frames_sizes.py's decode that fits).  For each, between HIP
events around the synchronous calls, the arms alternating call by call in one
process, the median of --reps after --warmup warm-ups:

  sizes    lz4ada_frames_device_sizes alone;
  exact    lz4ada_decode_frames_device_opt with LZ4ADA_FRAMES_EXACT into a
           buffer of exactly the total;
  plain    lz4ada_decode_frames_device into a buffer of the bound;
  parent   the same call of --parent-lib, a build of the parent commit (first
           batch only): the yardstick for "no change without the flag", with
           the run-to-run spread ((max - min) / median) of both beside it.

Device memory: what the device has in use (hipMemGetInfo) after one call of
an arm over what it had before, the library's scratch released in between --
the scratch is grow-only, so that is the arm's peak, the caller's output
buffer included.

    tools/frames_sizes_ab.py [--parent-lib PATH] [--out profiles/frames_sizes_ab.txt]
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

import torch  # noqa: E402

import lz4ada  # noqa: E402
import lz4frame  # noqa: E402


def single_block_frames(n):
    out = []
    for i in range(n):
        comp, raw = lz4ada.gen_block(1, 0x4652 + i, 65536)
        out.append(lz4frame.build_frame([(comp, raw, False)], 64 << 10, content_cksum=True)[0])
    return out


def small_payload_frames(n):
    """One block of 1-3 KiB of payload under a 4 MiB block maximum, kinds mixed."""
    out = []
    for i in range(n):
        kind, size = [(0, 2000), (1, 4000), (3, 2500), (4, 40000), (5, 5000), (6, 2000)][i % 6]
        size += 37 * (i % 11)
        if kind == 6:
            raw = random.Random(i).randbytes(size)
            block = (raw, raw, True)
        else:
            block = (*lz4ada.gen_block(kind, 7000 + i, size), False)
        out.append(lz4frame.build_frame([block], 4 << 20, block_cksum=bool(i & 1), content_cksum=bool(i & 2))[0])
    return out


def alternate(arms, reps, warmup):
    """arms: {name: call}.  The calls alternate; -> {name: (median, min, max)} in ms."""
    times = {k: [] for k in arms}
    for r in range(warmup + reps):
        for k, call in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:.3f} - {t[2]:.3f})"


def spread(t):
    return 100 * (t[2] - t[1]) / t[0]


def in_use():
    free, total = torch.cuda.mem_get_info()
    return total - free


def measure(name, frames, parent, reps, warmup, lines):
    lib = lz4ada._lib
    data = b"".join(frames)
    spans, at = [], 0
    for f in frames:
        spans.append((at, len(f)))
        at += len(f)
    n = len(frames)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    bound, _ = lz4ada.frames_device_bound(t.data_ptr(), t.numel(), spans)
    total, _ = lz4ada.frames_device_sizes(t.data_ptr(), t.numel(), spans)
    jobs = lz4ada._device_jobs(spans)
    olen, tot = ctypes.c_int64(), ctypes.c_int64()
    stats = {}

    def decode(which, flags, out, arm):
        st = which.lz4ada_decode_frames_device_opt(t.data_ptr(), t.numel(), jobs, n, flags, out.data_ptr(),
                                                   out.numel(), ctypes.byref(olen), 0)
        if st or olen.value != total or any(jobs[i].status for i in range(n)):
            raise SystemExit(f"{name} {arm}: decode failed: {st}, {olen.value} bytes " + lz4ada._thread_error())
        if which is lib and arm not in stats:
            stats[arm] = lz4ada.last_batch_stats().passes

    def sizes():
        if lib.lz4ada_frames_device_sizes(t.data_ptr(), t.numel(), jobs, n, 0, ctypes.byref(tot), 0) or \
                tot.value != total:
            raise SystemExit(f"{name}: sizes failed: " + lz4ada._thread_error())

    # device memory, arm by arm, from a released scratch
    mem = {}
    for arm, flags, need in (("exact", lz4ada.FRAMES_EXACT, total), ("plain", 0, bound)):
        lib.lz4ada_release_device_cache()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = in_use()
        out = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda:0")
        decode(lib, flags, out, arm)
        mem[arm] = in_use() - before
        if arm == "exact":
            first = out[:total].cpu()
        elif not torch.equal(out[:total].cpu(), first):
            raise SystemExit(f"{name}: the two layouts decode to different bytes")
        del out
    out_exact = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda:0")
    out_plain = torch.empty(max(bound, 1), dtype=torch.uint8, device="cuda:0")
    arms = {"sizes": sizes,
            "exact": lambda: decode(lib, lz4ada.FRAMES_EXACT, out_exact, "exact"),
            "plain": lambda: decode(lib, 0, out_plain, "plain")}
    if parent is not None:
        arms["parent"] = lambda: decode(parent, 0, out_plain, "parent")
    r = alternate(arms, reps, warmup)

    lines.append(f"{name}: {n} frames, {len(data)} compressed -> {total} bytes; bound {bound} "
                 f"({bound / max(total, 1):.1f}x the total)")
    lines.append(f"  (a) sizes alone   lz4ada_frames_device_sizes          {fmt(r['sizes'])} ms")
    lines.append(f"  (b) exact decode  ..._device_opt, LZ4ADA_FRAMES_EXACT {fmt(r['exact'])} ms   "
                 f"passes {stats['exact']}, device memory {mem['exact'] / 2**20:.0f} MiB")
    lines.append(f"  (c) plain decode  lz4ada_decode_frames_device         {fmt(r['plain'])} ms   "
                 f"passes {stats['plain']}, device memory {mem['plain'] / 2**20:.0f} MiB, "
                 f"spread {spread(r['plain']):.1f} %")
    if parent is not None:
        lines.append(f"      parent commit the same call                       {fmt(r['parent'])} ms   "
                     f"spread {spread(r['parent']):.1f} %; plain / parent {r['plain'][0] / r['parent'][0]:.3f}")
    lines.append(f"  exact / plain {r['exact'][0] / r['plain'][0]:.2f}; sizes / plain {r['sizes'][0] / r['plain'][0]:.2f}")
    lines.append("")
    print("\n".join(lines[-7:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_sizes_ab.txt"))
    ap.add_argument("--parent-lib", default=None, help="liblz4ada_hip.so built from the parent commit")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.lz4ada_decode_frames_device_opt.argtypes = lz4ada._lib.lz4ada_decode_frames_device_opt.argtypes
        parent.lz4ada_decode_frames_device_opt.restype = ctypes.c_int
    lines = ["Exact sizes and the decode laid out by them against the decode laid out by the bound "
             "(tools/frames_sizes_ab.py)",
             f"one MI355X, one process, clocks as found; HIP events around the synchronous calls, the arms "
             f"alternating; median of {args.reps} after {args.warmup} warm-ups (min - max)", ""]
    measure(f"{args.frames} x 64 KiB", single_block_frames(args.frames), parent, args.reps, args.warmup, lines)
    measure(f"{args.frames} x 1-3 KiB payload, 4 MiB block maximum", small_payload_frames(args.frames), None,
            args.reps, args.warmup, lines)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
