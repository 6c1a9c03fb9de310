#!/usr/bin/env python3
"""Ranged decode through a seek index against decoding the whole frames and
slicing.  Frames in device memory, B.Indep, 64 KiB
mixed blocks with block checksums, once with and once without a content
checksum (which the whole-frame decode verifies and a range does not).  Between HIP events around the synchronous
calls, the arms alternating call by call in one process, the median of --reps
after --warmup warm-ups:

  A  one frame of 1,024 blocks, 4,096 ranges of 4 KiB at seeded random offsets;
  B  the same frame, one range covering all of it: the price of the slot and
     the gather, which the whole-frame decode does not pay;
  C  1,024 frames of 4 blocks, one range of 1 KiB in each.

  ranged    lz4ada_decode_ranges_device into a buffer of the clipped total;
  baseline  lz4ada_decode_frames_device_opt with LZ4ADA_FRAMES_EXACT over the
            whole frames into a buffer of their total, then the ranges' bytes
            picked out on the device by one torch gather over an index tensor
            built beforehand (B: no gather, the frame's bytes are the range's);
  build     lz4ada_seek_index_build + lz4ada_seek_index_free, reported apart:
            a reader pays it once per set of frames.

Both arms' bytes are compared once before anything is timed.

    tools/ranges_ab.py [--out profiles/ranges_ab.txt]
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

BLOCK = 65536


def blocks_of(nblocks, seed):
    return [(*lz4ada.gen_block(lz4ada.GEN_MIXED, seed + k, BLOCK), False) for k in range(nblocks)]


def frame_of(blocks, content_cksum):
    return lz4frame.build_frame(blocks, 64 << 10, block_cksum=True, content_cksum=content_cksum)[0]


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


def measure(name, frames, ranges, whole, reps, warmup, lines):
    """ranges: [(job, off, len)], every one inside its frame.  whole: the one
    range is all of the one frame (no gather in the baseline)."""
    lib = lz4ada._lib
    data = b"".join(frames)
    spans, at = [], 0
    for f in frames:
        spans.append((at, len(f)))
        at += len(f)
    n = len(frames)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    total, sized = lz4ada.frames_device_sizes(t.data_ptr(), t.numel(), spans)
    jobs = lz4ada._device_jobs(spans)
    olen = ctypes.c_int64()
    dec = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    idx = lz4ada.SeekIndex.build_tensor(t, spans)
    nblocks = sum(lz4ada.frame_index(f)[0].nblocks for f in frames)
    want = sum(r[2] for r in ranges)
    out = torch.empty(want, dtype=torch.uint8, device="cuda:0")
    arr, nr = lz4ada._frame_ranges(ranges)
    passes = {}

    def decode_whole():
        st = lib.lz4ada_decode_frames_device_opt(t.data_ptr(), t.numel(), jobs, n, lz4ada.FRAMES_EXACT,
                                                 dec.data_ptr(), dec.numel(), ctypes.byref(olen), 0)
        if st or olen.value != total or any(jobs[i].status for i in range(n)):
            raise SystemExit(f"{name}: whole decode failed: {st} " + lz4ada._thread_error())

    def baseline():
        decode_whole()
        return dec if whole else dec[pick]

    def ranged():
        st = lib.lz4ada_decode_ranges_device(idx._ptr, t.data_ptr(), t.numel(), arr, nr, out.data_ptr(),
                                             out.numel(), ctypes.byref(olen), 0)
        if st or olen.value != want or any(arr[i].status for i in range(nr)):
            raise SystemExit(f"{name}: ranged decode failed: {st} " + lz4ada._thread_error())
        passes.setdefault("ranged", lz4ada.last_batch_stats().passes)

    def build():
        lz4ada.SeekIndex.build(t.data_ptr(), t.numel(), spans).free()

    # where every range's bytes lie in the whole decode (rising in_off: the spans' order)
    decode_whole()
    base = [jobs[i].out_off for i in range(n)]
    if not whole:
        pick = torch.cat([torch.arange(base[j] + off, base[j] + off + ln, dtype=torch.int64)
                          for j, off, ln in ranges]).to("cuda:0")
    ranged()
    if not torch.equal(baseline().cpu(), out.cpu()):
        raise SystemExit(f"{name}: the two arms deliver different bytes")
    r = alternate({"ranged": ranged, "baseline": baseline, "build": build}, reps, warmup)
    lines.append(f"{name}: {n} frames, {nblocks} blocks, {len(data)} compressed -> {total} bytes; "
                 f"{nr} ranges, {want} bytes wanted")
    lines.append(f"  ranged    lz4ada_decode_ranges_device                 {fmt(r['ranged'])} ms   "
                 f"passes {passes['ranged']}")
    lines.append(f"  baseline  whole frames, LZ4ADA_FRAMES_EXACT" + ("          " if whole else ", + gather") +
                 f" {fmt(r['baseline'])} ms")
    lines.append(f"  build     lz4ada_seek_index_build + _free             {fmt(r['build'])} ms   "
                 f"index {idx.device_bytes} device bytes, {idx.device_bytes / max(nblocks, 1):.1f} per block")
    lines.append(f"  baseline / ranged {r['baseline'][0] / r['ranged'][0]:.2f}")
    lines.append("")
    idx.free()
    print("\n".join(lines[-6:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranges_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not lz4ada.device_available():
        raise SystemExit("no usable GPU: " + lz4ada._thread_error())
    lines = ["Ranged decode through a seek index against the whole frames decoded and sliced "
             "(tools/ranges_ab.py)",
             f"one MI355X, one process, clocks as found; HIP events around the synchronous calls, the arms "
             f"alternating; median of {args.reps} after {args.warmup} warm-ups (min - max)", ""]
    big, small = blocks_of(1024, 0x5200), [blocks_of(4, 0x6000 + 4 * i) for i in range(1024)]
    size = 1024 * BLOCK
    rng = random.Random(0x5241)
    scattered = [(0, rng.randrange(size - 4096), 4096) for _ in range(4096)]
    one_each = [(i, rng.randrange(4 * BLOCK - 1024), 1024) for i in range(1024)]
    # with a content checksum the whole-frame decode also hashes every decoded byte (a frame over
    # lz4ada_batch_hash_max() bytes on the host chain); a range never does: both are shown
    for cc in (True, False):
        tag = "content checksum" if cc else "no content checksum"
        one = [frame_of(big, cc)]
        measure(f"A  1 x 1,024 x 64 KiB, {tag}; 4,096 x 4 KiB", one, scattered, False, args.reps, args.warmup, lines)
        measure(f"B  1 x 1,024 x 64 KiB, {tag}; the whole frame", one, [(0, 0, size)], True, args.reps, args.warmup,
                lines)
        measure(f"C  1,024 x 4 x 64 KiB, {tag}; 1 KiB of each", [frame_of(b, cc) for b in small], one_each, False,
                args.reps, args.warmup, lines)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
